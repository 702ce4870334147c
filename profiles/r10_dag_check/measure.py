"""Digest rate, full audit time against the build, on one MI355X (profiles/r10_dag_check)."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from nodexa_chain_core_amd import _build  # noqa: E402

_build.build_all()
from nodexa_chain_core_amd import _core  # noqa: E402
from nodexa_chain_core_amd.ops.ethash import DeviceEpoch  # noqa: E402


def timed(fn, warm=2, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


out = {}
for epoch in (0, 384):
    t0 = time.perf_counter()
    e = DeviceEpoch(epoch, device=0, ctx=_core.get_epoch_context(epoch))
    ctx_s = time.perf_counter() - t0
    e.build()
    torch.cuda.synchronize()
    assert e.l1_matches()
    gib = e.dag_bytes / 2**30
    table = torch.empty(e.chunks, dtype=torch.int64, device="cuda")
    d = timed(lambda: e.digest(out=table))
    view = e.dag[:e.dag_bytes // 8 * 8].view(torch.int64)
    s = timed(lambda: torch.sum(view))
    want = _core.dag_digest(e.dag[:64 * 16384 * 3].cpu().numpy(), 0)
    got = [int(x) & (2**64 - 1) for x in table[:3].cpu().tolist()]
    b = timed(lambda: e.build(), warm=1, reps=3)
    a = timed(lambda: e.audit(), warm=1, reps=3)
    res = e.audit_result()
    out[str(epoch)] = {
        "dag_gib": round(gib, 3), "items": e.items512, "context_s": round(ctx_s, 2),
        "digest_ms_median_min_max": [round(x, 4) for x in d], "digest_tb_s": round(e.dag_bytes / d[0] / 1e9, 3),
        "torch_sum_ms_median_min_max": [round(x, 4) for x in s], "torch_sum_tb_s": round(e.dag_bytes / s[0] / 1e9, 3),
        "digest_matches_host_model": got == want,
        "build_ms_median_min_max": [round(x, 3) for x in b], "audit_ms_median_min_max": [round(x, 3) for x in a],
        "audit_clean": [res.mismatches, res.checked],
    }
    print(epoch, json.dumps(out[str(epoch)]), flush=True)
    del e, table, view
    torch.cuda.empty_cache()
with open("dag_measure.json", "w") as f:
    json.dump(out, f, indent=1)
