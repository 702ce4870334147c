#!/usr/bin/env python3
"""Period-agnostic KawPow search (kawpow_search_any) against the per-period compiled kernel.

One process, one GPU run, through the project's own searcher and search device:

  compile     wall time of one period's `hipcc --genco` with the production defines (a cache
              directory of its own, so nothing is reused); `--compile-only` stops here (no GPU)
  throughput  generic and compiled kernel alternated A/B over `--windows` windows each of `--batch`
              nonces at `--epoch` (hip events), MH/s, MH/s per GHz at the end-of-run clock, ratio
  resources   VGPRs, LDS bytes and waves per SIMD of kawpow_search_any from its code object
  cold        hashes completed in the first N seconds after set_block to an uncached period,
              -kawpowjit=auto against wait (N = the compile time measured above)

    python tools/kawpow_anyperiod_probe.py --epoch 384 --out profile.json
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resources() -> dict:
    """kawpow_search_any's register / LDS use from the code object's metadata note."""
    from nodexa_chain_core_amd import _build
    from nodexa_chain_core_amd.ops import jump_slots

    path = os.path.join(_build.PKG, "kernels", "kawpow_anyperiod.hsaco")
    tool = os.path.join(jump_slots.LLVM, "llvm-readelf")
    if not (os.path.exists(path) and os.path.exists(tool)):
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        notes = subprocess.run([tool, "--notes", jump_slots._code_object(path, tmp)], capture_output=True,
                               text=True, check=True).stdout
    # amdhsa.kernels: one list entry per kernel, its own keys at four spaces of indent
    entry = next(b for b in re.split(r"\n  - ", notes) if re.search(r"\.name:\s+kawpow_search_any\s", b))
    vals = {k: int(v) for k, v in re.findall(r"^ {0,4}\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    vgprs, lds = vals.get("vgpr_count", 0), vals.get("group_segment_fixed_size", 0)
    alloc = -(-max(vgprs, 1) // 8) * 8  # gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8
    by_lds = 160 * 1024 // max(lds, 1)  # workgroups per CU; a 256-thread one puts one wave on each SIMD
    return {"vgprs": vgprs, "sgprs": vals.get("sgpr_count", 0), "lds_bytes": lds,
            "scratch_bytes": vals.get("private_segment_fixed_size", 0),
            "waves_per_simd": min(8, 512 // alloc, by_lds)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--epoch", type=int, default=384)
    ap.add_argument("--batch", type=int, default=1 << 25)
    ap.add_argument("--windows", type=int, default=8, help="timed windows per kernel")
    ap.add_argument("--cold-batch", type=int, default=1 << 22, help="window of the cold-switch run")
    ap.add_argument("--limit", type=float, default=300.0, help="seconds after which no new phase starts")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t_start = time.monotonic()
    out: dict = {"epoch": a.epoch}

    from nodexa_chain_core_amd import _core
    from nodexa_chain_core_amd.ops import jit

    def emit(key, val):
        out[key] = val
        print(json.dumps({key: val}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    height = a.epoch * 7500 + 4000
    dag_bytes = _core.full_dataset_num_items(a.epoch) * 128
    defines = jit.defines_for(dag_bytes)
    cache = tempfile.mkdtemp(prefix="kawpow_probe_cache_")
    jit.CACHE_DIR = cache
    times = []
    for k in range(3):  # three different periods, none of them cached
        t0 = time.perf_counter()
        jit.compile_period(height // 3 + 100 + k, defines)
        times.append(round(time.perf_counter() - t0, 3))
    compile_s = statistics.median(times)
    emit("compile", {"defines": list(defines), "seconds": times, "median_s": compile_s, "cpus": os.cpu_count()})
    emit("resources", resources())
    if a.compile_only:
        return 0

    import torch

    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, SearchPipeline, Work
    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher
    from nodexa_chain_core_amd.utils import gpuinfo

    torch.cuda.set_device(0)
    ep = DeviceEpoch(a.epoch, device=0)
    ep.build()
    torch.cuda.synchronize()
    header = _core.sha256d(b"anyperiod probe")
    s = {"jit": KawpowSearcher(ep, height, jit_mode="wait"), "generic": KawpowSearcher(ep, height, jit_mode="off")}
    g = s["generic"].block
    assert s["jit"].block == g
    n = a.batch // g * g

    # both kernels must agree before either is timed: one window, a target that ~8 nonces pass
    target = (1 << 64) // (n // 8)
    found = {}
    for kind, sr in s.items():
        sr.launch(header, 1 << 40, n, target)
        found[kind] = {(x.nonce, x.mix_hash, x.final_hash) for x in sr.collect()}
    emit("agree", {"shares": len(found["jit"]), "equal": found["jit"] == found["generic"]})
    if found["jit"] != found["generic"]:
        return 1

    ms = {"jit": [], "generic": []}
    order = ["generic", "jit"]
    for r in range(a.windows + 1):  # round 0 warms both up
        for kind in order if r % 2 == 0 else order[::-1]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            s[kind].launch(header, (r + 2) * n, n, 0)
            e1.record()
            e1.synchronize()
            assert s[kind].kernel_kind == kind
            if r:
                ms[kind].append(e0.elapsed_time(e1))
        if time.monotonic() - t_start > a.limit:
            break
    sclk = gpuinfo.snapshot(0).get("sclk_mhz") or 0
    tp = {"window": n, "granule": g, "windows_each": len(ms["jit"]), "sclk_mhz_end": sclk}
    for kind in ms:
        mhs = [n / (t / 1e3) / 1e6 for t in ms[kind]]
        tp[kind] = {"median_mhs": round(statistics.median(mhs), 2), "min_mhs": round(min(mhs), 2),
                    "max_mhs": round(max(mhs), 2),
                    "mhs_per_ghz": round(statistics.median(mhs) / (sclk / 1e3), 2) if sclk else None}
    tp["generic_over_jit"] = round(tp["generic"]["median_mhs"] / tp["jit"]["median_mhs"], 4)
    emit("throughput", tp)
    del s
    if time.monotonic() - t_start > a.limit:
        return 0

    # cold period switch: a period nobody compiled, a search device per mode, pipelined windows
    # for N = compile_s seconds from the moment the first window is submitted (submit -> set_block)
    cold = {"seconds": compile_s, "window": a.cold_batch // g * g}
    boundary = bytes(32)  # no share passes: nothing but hashing
    for i, mode in enumerate(("wait", "auto")):
        h2 = height + 3 * (500 + i)  # two different uncached periods of the same epoch
        dev = GpuSearchDevice(0, jit_mode=mode)
        dev.epochs[a.epoch] = ep
        pipe = SearchPipeline(dev)
        work = Work(header, boundary, h2, job_id=1, flags=0)
        done, start, kinds, first_at = 0, 0, {"jit": 0, "generic": 0}, None
        t0 = time.perf_counter()
        while True:
            res = pipe.step(work, start, cold["window"])  # the first call sets the block (wait: compiles)
            start += cold["window"]
            now = time.perf_counter() - t0
            if res is not None and now <= compile_s:
                done += res.hashes
                kinds[res.kernel] += 1
                first_at = first_at if first_at is not None else round(now, 3)
            if now > compile_s:
                break
        pipe.drain()
        fut = dev.searchers[a.epoch].chooser.pending(h2 // 3)
        cold[mode] = {"hashes": done, "mhs": round(done / compile_s / 1e6, 2), "windows": kinds,
                      "first_result_s": first_at, "compile_still_pending": fut is not None and not fut.done()}
        dev.close()
    emit("cold_switch", cold)
    return 0


if __name__ == "__main__":
    sys.exit(main())
