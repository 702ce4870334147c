"""Throughput of the search loop at epoch 384: no scrub, a scrub every 0.25 s, the same on a low-priority stream."""
import sys
import time

import torch

sys.path.insert(0, ".")
from nodexa_chain_core_amd import _core  # noqa: E402
from nodexa_chain_core_amd.miner.search import GpuSearchDevice, SearchPipeline, Work  # noqa: E402

height = 384 * _core.EPOCH_LENGTH + 123
hh = _core.sha256d(b"probe")
w = Work(hh, bytes(32), height, 1, 0, 0)
dev = GpuSearchDevice(0, dag_check=True, dag_scrub_s=0.25)
pipe = SearchPipeline(dev, watchdog_s=120)
n = 1 << 25
print("priority range", torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, "priority_range") else None)
try:
    low = torch.cuda.Stream(device=0, priority=1)
    print("low stream priority", low.priority)
except Exception as e:  # noqa: BLE001
    low = None
    print("no low priority stream:", e)
normal = dev.side
k = 0
for _ in range(4):
    pipe.step(w, k * n, n); k += 1


def run(label, scrub_s, side, steps=40):
    global k
    dev.dag_scrub_s = scrub_s
    dev.side = side
    s0 = dev.dag_scrubs
    ends = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = pipe.step(w, k * n, n); k += 1
        ends.append(r.end_ms)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    span = (ends[-1] - ends[1]) / 1e3
    print(label, "wall MH/s", round(steps * n / dt / 1e6, 3), "device MH/s", round((steps - 2) * n / span / 1e6, 3),
          "scrubs", dev.dag_scrubs - s0, "last_scrub_ms", round(dev.dag_last_scrub_ms, 3), flush=True)


for rep in range(2):
    run("off     ", 0.0, normal)
    run("scrub   ", 0.25, normal)
    if low is not None:
        run("scrublow", 0.25, low)
run("off     ", 0.0, normal)
pipe.drain()
