#!/usr/bin/env python3
"""Connecting a block of mempool-verified transactions with and without the script-execution cache
(-scriptcache=0|1).

A regtest node takes N seeded transactions through accept_to_mempool, mines them into one block and
connects it. Two shapes from utils/synth_block: payments (6000 one-input transactions) and
consolidation (60 transactions of 200 inputs). The timed parts are the `_activate` walk that connects
the stored block (and, inside it, the ConnectTip of that block alone: the walk also takes the block's
transactions out of the mempool, which costs the same either way) and accept_to_mempool per
transaction, because the flag adds a pass under the block's flags there. -scriptcache=0 and 1
alternate in one process, warm-ups first; the yardstick is the flag-off setting of the same process.

With --gpusigs=off it needs no GPU (the host path); with --gpusigs=on it fails without one, and
--gpusighash picks the deferred path. The hard conditions are counters, asserted in every run with
the flag on: all N transactions hit, gpu_sigs does not move, the signature cache is not touched
during the connect. One JSON document on stdout (and in --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WITNESS_COMMITMENT_HEADER = b"\x6a\x24\xaa\x21\xa9\xed"


def _stats(xs, unit="ms", digits=3):
    return {f"median_{unit}": round(statistics.median(xs), digits), f"min_{unit}": round(min(xs), digits),
            f"max_{unit}": round(max(xs), digits), f"runs_{unit}": [round(x, digits) for x in xs]}


def _differs(a, b):
    return ("faster" if max(a) < min(b) else "slower" if max(b) < min(a) else
            "no difference beyond the spread of the repeats")


def _new_state():
    from nodexa_chain_core_amd.chain.state import REGTEST_KAWPOW_FROM_GENESIS, ChainState, make_params

    st = ChainState(make_params("regtest", REGTEST_KAWPOW_FROM_GENESIS), None)
    st.min_relay_fee = 0  # the seeded transactions pay 1000 per input
    return st


def _solve(_core, blk):
    ctx = _core.get_epoch_context(0)
    h = blk.header
    for n in range(256):  # regtest target 2^255
        fin, mix = _core.kawpow_hash(ctx, h.height, h.kawpow_header_hash()[::-1], n)
        if fin[0] < 0x80:
            h.nonce64, h.mix_hash = n, mix[::-1]
            blk.header = h
            return blk
    raise RuntimeError("no nonce found")


def run_once(synth, view, flag: int, gpusigs: str, mode: int):
    """One node: fill the mempool, mine, connect -> the times and counters of this run."""
    from nodexa_chain_core_amd import core
    from nodexa_chain_core_amd.miner.assembler import BlockAssembler

    _core = core()
    txs = list(synth.vtx[1:])
    st = _new_state()
    for tx in txs:
        for vin in tx.vin:
            value, spk, _, _ = view.get(vin.prevout.hash, vin.prevout.n)
            st.coins.add(vin.prevout.hash, vin.prevout.n, value, spk, 1, False)
    st.script_cache = bool(flag)
    st.gpu_signatures = gpusigs
    st.gpu_sighash, st.gpu_sighash_forms = mode >= 1, "all" if mode == 2 else "legacy-all"
    _core.scriptcache_clear()
    _core.sigcache_clear()
    sc0 = _core.scriptcache_stats()
    t0 = time.perf_counter()
    for tx in txs:
        ok, why, _ = st.accept_to_mempool(tx)
        assert ok, why
    accept_us = (time.perf_counter() - t0) * 1e6 / len(txs)
    # a fixed time: every run mines the same block, so the UTXO hashes can be compared
    now = st.params.genesis.header.time + 600
    blk = _solve(_core, BlockAssembler(st).create_new_block(b"\x51", now=now).block)
    assert len(blk.vtx) == 1 + len(txs), f"the assembler took {len(blk.vtx) - 1} of {len(txs)} transactions"
    real = st._activate
    st._activate = lambda: {}  # store only
    r = st.process_new_block(blk)
    assert r.ok, r.reject
    st._activate = real
    tip_ms = []
    connect_one = st._connect_one

    def timed_connect_one(block, idx):
        t = time.perf_counter()
        out = connect_one(block, idx)
        tip_ms.append((time.perf_counter() - t) * 1e3)
        return out

    st._connect_one = timed_connect_one
    sig0, sc1, before = _core.sigcache_stats(), _core.scriptcache_stats(), dict(st.sig_stats)
    if gpusigs == "on":
        import torch

        torch.cuda.synchronize()
    t0 = time.perf_counter()
    with st.lock:
        failed = st._activate()
    walk_ms = (time.perf_counter() - t0) * 1e3
    assert not failed and st.height() == 1, (failed, st.height())
    moved = {k: st.sig_stats[k] - before[k] for k in before}
    sig1, sc2 = _core.sigcache_stats(), _core.scriptcache_stats()
    if flag:
        assert moved["script_cache_txs"] == len(txs), moved          # all N transactions hit
        assert moved["gpu_sigs"] == 0 and moved["gpu_batches"] == 0   # nothing left for the device
        assert (sig1["hits"], sig1["misses"]) == (sig0["hits"], sig0["misses"])  # the signature cache is not touched
        assert sc1["entries"] == len(txs) and sc2["entries"] == 0
    else:
        assert sc2 == sc0 and moved["script_cache_txs"] == 0          # the cache never moves
    return {"walk_ms": walk_ms, "connect_tip_ms": sum(tip_ms), "accept_us": accept_us, "moved": moved,
            "sigcache_hits": sig1["hits"] - sig0["hits"], "utxo": st.coins.stats()[3].hex()}


def probe_shape(name, n_txs, n_in, repeats, warmup, gpusigs, mode):
    from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block

    synth, view, _, info = make_consolidation_block(n_txs, n_in, seed=7)
    for _ in range(warmup):
        for flag in (0, 1):
            run_once(synth, view, flag, gpusigs, mode)
    runs = {0: [], 1: []}
    for _ in range(repeats):
        for flag in (0, 1):
            runs[flag].append(run_once(synth, view, flag, gpusigs, mode))
    assert len({r["utxo"] for f in runs for r in runs[f]}) == 1  # the same UTXO set either way

    def section(flag):
        rs = runs[flag]
        return {"walk": _stats([r["walk_ms"] for r in rs]), "connect_tip": _stats([r["connect_tip_ms"] for r in rs]),
                "accept_per_tx": _stats([r["accept_us"] for r in rs], "us", 1), "counters": rs[-1]["moved"],
                "sigcache_hits_in_connect": rs[-1]["sigcache_hits"]}

    out = {"shape": name, "txs": n_txs, "inputs": info["inputs"], "sigs": info["sigs"], "gpusigs": gpusigs,
           "gpusighash": mode, "flag_off": section(0), "flag_on": section(1)}
    for key in ("walk_ms", "connect_tip_ms", "accept_us"):
        on, off = [r[key] for r in runs[1]], [r[key] for r in runs[0]]
        out[f"{key}_on_vs_off"] = _differs(on, off)
        out[f"{key}_ratio_on_over_off"] = round(statistics.median(on) / statistics.median(off), 3)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gpusigs", choices=("on", "off"), default="off")
    ap.add_argument("--gpusighash", type=int, choices=(0, 1, 2), default=0)
    ap.add_argument("--payments", type=int, default=6000, help="one-input transactions of the payments block")
    ap.add_argument("--consolidations", type=int, default=60)
    ap.add_argument("--inputs", type=int, default=200, help="inputs per consolidation transaction")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nodexa_chain_core_amd import _build

    device = "none"
    if a.gpusigs == "on":
        import torch

        if not torch.cuda.is_available():
            print("script_cache_probe: --gpusigs=on and no GPU present", file=sys.stderr)
            return 2
        _build.build_all()
        device = torch.cuda.get_device_name(0)
    else:
        _build.build_core()
    results = []
    for name, n_txs, n_in in (("payments", a.payments, 1), ("consolidation", a.consolidations, a.inputs)):
        if n_txs <= 0:
            continue
        results.append(probe_shape(name, n_txs, n_in, a.repeats, a.warmup, a.gpusigs, a.gpusighash))
        print(json.dumps(results[-1]), flush=True)
    doc = {"device": device, "repeats": a.repeats, "warmup": a.warmup, "shapes": results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
