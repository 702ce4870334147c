#!/usr/bin/env python3
"""Block connection with the legacy signature hashes on the host against on the GPU (-gpusighash).

Seeded blocks at sizes a node meets: a payments block (about 6000 one-input transactions) and a
consolidation block (about 60 transactions of 200 inputs, close to 2 MB). For each, the block is
connected with deferred signatures and the verdicts are fetched, alternately with the flag off
(connect_block + ops/secp.verify_batch: hashes on the host) and on (connect_block(defer_sighash)
+ ops/sighash.verify_block_sigs), after a warm-up, several repeats in the same process. The time
is a host clock around work that ends in the verdict download. The kernel alone is timed with
device events; the bytes it hashes are summed from the job table.

A GPU tool, not a test: it fails without a GPU. One JSON document on stdout (and in --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import struct
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs_ms": [round(x, 3) for x in xs]}


def probe_block(name, blk, view, height, info, repeats, warmup, threads):
    import torch

    from nodexa_chain_core_amd import core
    from nodexa_chain_core_amd.ops import runtime, secp, sighash

    _core = core()
    flags = _core.BLOCK_SCRIPT_VERIFY_FLAGS

    def run(on: bool):
        t0 = time.perf_counter()
        res, undo = _core.connect_block(blk, height, view, True, True, None, 0, flags, threads, defer_sighash=on)
        t1 = time.perf_counter()
        assert res.ok, res.reject
        verdicts = sighash.verify_block_sigs(res) if on else secp.verify_batch(res.sig_items())
        t2 = time.perf_counter()
        assert all(verdicts) and len(verdicts) == info["sigs"]
        assert _core.disconnect_block(blk, undo, view)  # not timed: the view is as before
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, res

    for _ in range(warmup):
        run(False)
        run(True)
    off, on = [], []
    for _ in range(repeats):
        c, v, _r = run(False)
        off.append((c, v))
        c, v, res = run(True)
        on.append((c, v))
    assert res.num_device_hashes == info["device_sigs"]

    # the kernel alone, and what it reads and hashes
    arena, jobs, secp_jobs, n_dev, n_host = res.sighash_pack()
    recs = list(struct.iter_unpack("<10I", jobs))
    msg_bytes = sum(sum(r[4:8]) for r in recs)
    block_bytes = sum(((sum(r[4:8]) + 9 + 63) // 64) * 64 for r in recs)
    kern_ms = []
    if n_dev:
        dev = torch.device("cuda", torch.cuda.current_device())
        d_arena, d_jobs = sighash._upload_jobs(arena, jobs, res.num_sigs, dev)
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        k = runtime.static_kernel("sighash", "sighash_gather_batch")
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            runtime.hip().launch_sighash_gather(k, d_arena.data_ptr(), d_jobs.data_ptr(), n_dev, 0, d_secp.data_ptr(),
                                                runtime.current_stream_handle())
            e1.record()
            e1.synchronize()
            if i >= warmup:
                kern_ms.append(e0.elapsed_time(e1))
    tot_off, tot_on = [c + v for c, v in off], [c + v for c, v in on]
    out = {
        "block": name, "txs": len(blk.vtx) - 1, "inputs": info["inputs"], "sigs": info["sigs"],
        "block_bytes": 80 + sum(len(tx.serialize(True)) for tx in blk.vtx),
        "device_sighashes": n_dev, "host_sighashes": n_host, "arena_bytes": len(arena),
        "host_hash_bytes": msg_bytes, "kernel_block_bytes": block_bytes, "threads": threads,
        "flag_off": {"total": _stats(tot_off), "connect": _stats([c for c, _ in off]),
                     "verify": _stats([v for _, v in off])},
        "flag_on": {"total": _stats(tot_on), "connect": _stats([c for c, _ in on]),
                    "verify": _stats([v for _, v in on])},
    }
    if kern_ms:
        out["kernel"] = _stats(kern_ms)
        out["kernel"]["gb_per_s"] = round(block_bytes / (statistics.median(kern_ms) * 1e-3) / 1e9, 2)
    lo_off, hi_off, lo_on, hi_on = min(tot_off), max(tot_off), min(tot_on), max(tot_on)
    out["verdict"] = ("on faster" if hi_on < lo_off else "off faster" if hi_off < lo_on else
                      "no difference beyond the spread of the repeats")
    out["speedup_median"] = round(statistics.median(tot_off) / statistics.median(tot_on), 3)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--payments", type=int, default=6000, help="one-input transactions of the payments block")
    ap.add_argument("--consolidations", type=int, default=60)
    ap.add_argument("--inputs", type=int, default=200, help="inputs per consolidation transaction")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        print("sighash_probe: no GPU present", file=sys.stderr)
        return 2
    from nodexa_chain_core_amd import _build

    _build.build_all()
    from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block

    results = []
    for name, n_txs, n_in in (("payments", a.payments, 1), ("consolidation", a.consolidations, a.inputs)):
        blk, view, height, info = make_consolidation_block(n_txs, n_in, seed=7)
        results.append(probe_block(name, blk, view, height, info, a.repeats, a.warmup, a.threads))
        print(json.dumps(results[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "blocks": results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
