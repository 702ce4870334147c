#!/usr/bin/env python3
"""Block connection with the signature hashes on the host against on the GPU (-gpusighash=0|1|2).

Seeded blocks at sizes a node meets: a payments block (about 6000 one-input transactions), a
consolidation block (about 60 transactions of 200 inputs, close to 2 MB), and the same shape with
the forms mixed (NONE, SINGLE, ANYONECANPAY, every fourth input P2WPKH). For each, the block is
connected with deferred signatures and the verdicts are fetched, the three values of the flag
alternated in one process: 0 (connect_block + ops/secp.verify_batch: hashes on the host), 1
(connect_block(defer_sighash) + ops/sighash.verify_block_sigs: the legacy ALL form on the GPU) and
2 (defer_all_forms too: every form), after a warm-up, several repeats. The time is a host clock
around work that ends in the verdict download. Each kernel alone is timed with device events; the
bytes it hashes are summed from the job table.

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


def _time_kernel(launch, warmup, repeats):
    import torch

    ms = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def _faster(a, b, name_a, name_b):
    """Which of two lists of repeats is faster beyond their min-max ranges."""
    return (f"{name_a} faster" if max(a) < min(b) else f"{name_b} faster" if max(b) < min(a) else
            "no difference beyond the spread of the repeats")


def probe_block(name, blk, view, height, info, repeats, warmup, threads):
    import torch

    from nodexa_chain_core_amd import core
    from nodexa_chain_core_amd.ops import runtime, secp, sighash

    _core = core()
    flags = _core.BLOCK_SCRIPT_VERIFY_FLAGS

    def run(mode: int):  # the value of -gpusighash
        t0 = time.perf_counter()
        res, undo = _core.connect_block(blk, height, view, True, True, None, 0, flags, threads,
                                        defer_sighash=mode > 0, defer_all_forms=mode == 2)
        t1 = time.perf_counter()
        assert res.ok, res.reject
        verdicts = sighash.verify_block_sigs(res) if mode else secp.verify_batch(res.sig_items())
        t2 = time.perf_counter()
        assert all(verdicts) and len(verdicts) == info["sigs"]
        assert _core.disconnect_block(blk, undo, view)  # not timed: the view is as before
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, res

    for _ in range(warmup):
        for mode in (0, 1, 2):
            run(mode)
    runs = {0: [], 1: [], 2: []}
    last = {}
    for _ in range(repeats):
        for mode in (0, 1, 2):
            c, v, last[mode] = run(mode)
            runs[mode].append((c, v))
    res, res2 = last[1], last[2]
    assert res.num_device_hashes == info["device_sigs"]

    # the kernels alone, and what they read and hash
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = runtime.current_stream_handle()
    arena, jobs, secp_jobs, n_dev, n_host = res.sighash_pack()
    recs = list(struct.iter_unpack("<10I", jobs))
    msg_bytes = sum(sum(r[4:8]) for r in recs)
    block_bytes = sum(((sum(r[4:8]) + 9 + 63) // 64) * 64 for r in recs)
    kern_ms = []
    if n_dev:
        d_arena, d_jobs = sighash._upload_jobs(arena, jobs, res.num_sigs, dev)
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        k = runtime.static_kernel("sighash", "sighash_gather_batch")
        kern_ms = _time_kernel(lambda: runtime.hip().launch_sighash_gather(
            k, d_arena.data_ptr(), d_jobs.data_ptr(), n_dev, 0, d_secp.data_ptr(), stream), warmup, repeats)
    arena2, segs2, jobs2, secp_jobs2, n_dev2, n_host2 = res2.sighash_pack_var()
    seg_len = [r[1] for r in struct.iter_unpack("<2I", segs2)]
    lens2 = [sum(seg_len[f:f + n]) for f, n, _, _ in struct.iter_unpack("<4I", jobs2)]
    block_bytes2 = sum(((n + 9 + 63) // 64) * 64 for n in lens2)
    kern2_ms = []
    if n_dev2:
        d_arena2, d_segs2, d_jobs2 = sighash._upload_var(arena2, segs2, jobs2, res2.num_sigs, dev)
        d_secp2 = torch.frombuffer(bytearray(secp_jobs2), dtype=torch.int32).to(dev)
        k2 = runtime.static_kernel("sighash_var", "sighash_gather_var")
        kern2_ms = _time_kernel(lambda: runtime.hip().launch_sighash_gather_var(
            k2, d_arena2.data_ptr(), d_segs2.data_ptr(), len(seg_len), d_jobs2.data_ptr(), n_dev2, 0,
            d_secp2.data_ptr(), stream), warmup, repeats)

    def section(mode):
        return {"total": _stats([c + v for c, v in runs[mode]]), "connect": _stats([c for c, _ in runs[mode]]),
                "verify": _stats([v for _, v in runs[mode]])}

    tot = {m: [c + v for c, v in runs[m]] for m in runs}
    out = {
        "block": name, "txs": len(blk.vtx) - 1, "inputs": info["inputs"], "sigs": info["sigs"],
        "block_bytes": 80 + sum(len(tx.serialize(True)) for tx in blk.vtx),
        "device_sighashes": n_dev, "host_sighashes": n_host, "arena_bytes": len(arena),
        "host_hash_bytes": msg_bytes, "kernel_block_bytes": block_bytes, "threads": threads,
        "flag_off": section(0), "flag_on": section(1),
        "flag_2": dict(section(2), device_sighashes=n_dev2, host_sighashes=n_host2, device_v0=res2.num_device_v0,
                       device_partial=res2.num_device_partial, arena_bytes=len(arena2), segments=len(seg_len),
                       host_hash_bytes=sum(lens2), kernel_block_bytes=block_bytes2),
    }
    if kern_ms:
        out["kernel"] = _stats(kern_ms)
        out["kernel"]["gb_per_s"] = round(block_bytes / (statistics.median(kern_ms) * 1e-3) / 1e9, 2)
    if kern2_ms:
        out["kernel_var"] = _stats(kern2_ms)
        out["kernel_var"]["gb_per_s"] = round(block_bytes2 / (statistics.median(kern2_ms) * 1e-3) / 1e9, 2)
    out["verdict"] = _faster(tot[1], tot[0], "on", "off")
    out["verdict_2_vs_0"] = _faster(tot[2], tot[0], "2", "0")
    out["verdict_2_vs_1"] = _faster(tot[2], tot[1], "2", "1")
    out["speedup_median"] = round(statistics.median(tot[0]) / statistics.median(tot[1]), 3)
    out["speedup_median_2"] = round(statistics.median(tot[0]) / statistics.median(tot[2]), 3)
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
    mixed = dict(hash_types=(1, 0x81, 2, 3, 0x82, 0x83), witness_every=4)
    for name, n_txs, n_in, kw in (("payments", a.payments, 1, {}), ("consolidation", a.consolidations, a.inputs, {}),
                                  ("mixed forms", a.consolidations, a.inputs, mixed)):
        blk, view, height, info = make_consolidation_block(n_txs, n_in, seed=7, **kw)
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
