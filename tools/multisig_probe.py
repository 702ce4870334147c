#!/usr/bin/env python3
"""Connecting stored blocks of multisig spends with the CHECKMULTISIG pairing resolved on the host
re-check path against on the GPU (-gpumultisig).

Two seeded regtest chains of the shapes of tools/sig_window_probe.py (512 blocks of one 24-input
transaction, 64 blocks of one 200-input transaction) whose inputs are all P2SH 2-of-3, the signing
pair cycling through the three subsets by input: two inputs of three are signed by a pair other
than the last two keys, which a deferring checker without -gpumultisig sends back to the host. The
timed part is the one `_activate` walk that connects the stored blocks. The settings (-gpumultisig
0 and 1, -gpusigwindow 0 and 16384, -gpusighash 0 and 2) alternate in one process, warm-ups first.
Then the kernels of a window alone, with device events: the gather, the verifier, sig_group_resolve
and sig_window_verdicts.

--flags 0 runs the settings without -gpumultisig only, through nothing but the interface a tree
without the flag has: with --cache DIR holding the chains built by a run of this tree, that is the
same measurement on the commit before it.

A GPU tool, not a test: it fails without a GPU. One JSON document on stdout (and in --out).
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WINDOWS = (0, 16384)
MODES = (0, 2)
WITNESS_COMMITMENT_HEADER = b"\x6a\x24\xaa\x21\xa9\xed"


def _stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "runs_ms": [round(x, 3) for x in xs]}


def _differs(a, b):
    return ("faster" if max(a) < min(b) else "slower" if max(b) < min(a) else
            "no difference beyond the spread of the repeats")


def _new_state():
    from nodexa_chain_core_amd.chain.state import REGTEST_KAWPOW_FROM_GENESIS, ChainState, make_params

    st = ChainState(make_params("regtest", REGTEST_KAWPOW_FROM_GENESIS), None)
    st.gpu_signatures = "off"
    return st


def build_chain(n_blocks: int, n_inputs: int, seed0: int):
    """-> (coins, raws): the outputs the chain spends, [(txid, n, value, scriptPubKey)], and its
    serialized blocks: the assembler's coinbase and header around one seeded synth_block transaction
    of `n_inputs` 2-of-3 inputs, mined on the previous block."""
    from nodexa_chain_core_amd import core
    from nodexa_chain_core_amd.miner.assembler import BlockAssembler
    from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block

    _core = core()
    st = _new_state()
    act = st.params.kawpow_activation_time
    ctx = _core.get_epoch_context(0)
    coins, raws = [], []
    for k in range(n_blocks):
        synth, view, _, _ = make_consolidation_block(1, n_inputs, seed=seed0 + k, multisig_every=1,
                                                     multisig_signers="cycle")
        for tx in synth.vtx[1:]:
            for vin in tx.vin:
                value, spk, _, _ = view.get(vin.prevout.hash, vin.prevout.n)
                coins.append((vin.prevout.hash, vin.prevout.n, value, spk))
                st.coins.add(vin.prevout.hash, vin.prevout.n, value, spk, 1, False)
        blk = BlockAssembler(st).create_new_block(b"\x51").block
        blk.vtx = [blk.vtx[0]] + list(synth.vtx[1:])
        vtx = list(blk.vtx)
        cb = vtx[0]
        outs = list(cb.vout)
        outs[blk.witness_commitment_index()] = _core.TxOut(
            0, WITNESS_COMMITMENT_HEADER + _core.sha256d(blk.witness_merkle_root() + bytes(32)))
        cb.vout = outs
        blk.vtx = [cb] + vtx[1:]
        h = blk.header
        h.merkle_root = blk.merkle_root()[0]
        for n in range(256):  # regtest target 2^255
            fin, mix = _core.kawpow_hash(ctx, h.height, h.kawpow_header_hash()[::-1], n)
            if fin[0] < 0x80:
                h.nonce64, h.mix_hash = n, mix[::-1]
                break
        blk.header = h
        r = st.process_new_block(blk)
        assert r.ok, r.reject
        raws.append(blk.serialize(act))
    return coins, raws


def cached_chain(cache, n_blocks, n_inputs, seed0):
    path = os.path.join(cache, f"multisig_chain_{n_blocks}x{n_inputs}_{seed0}.pickle") if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    got = build_chain(n_blocks, n_inputs, seed0)
    if path:
        os.makedirs(cache, exist_ok=True)
        with open(path, "wb") as f:
            pickle.dump(got, f)
    return got


def connect_once(coins, blocks, flag: int, window: int, mode: int):
    """One activation walk over the stored chain -> (ms, sig_stats, UTXO hash)."""
    import torch

    st = _new_state()
    for txid, n, value, spk in coins:
        st.coins.add(txid, n, value, spk, 1, False)
    real = st._activate
    st._activate = lambda: {}  # store only
    for blk in blocks:
        r = st.process_new_block(blk, check_pow=False)
        assert r.ok, r.reject
    st._activate = real
    st.gpu_signatures = "on"
    st.gpu_sig_window = window
    st.gpu_sighash, st.gpu_sighash_forms = mode >= 1, "all" if mode == 2 else "legacy-all"
    if flag:
        st.gpu_multisig = 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with st.lock:
        failed = st._activate()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert not failed and st.height() == len(blocks), (failed, st.height())
    return ms, dict(st.sig_stats), st.coins.stats()[3]


def arena_bytes(coins, blocks, flag: int, mode: int) -> int:
    """What the blocks' packers lay out for the device under -gpusighash=`mode`, summed."""
    from nodexa_chain_core_amd import core

    _core = core()
    if mode == 0:
        return 0
    view = _core.CoinsView()
    for txid, n, value, spk in coins:
        view.add(txid, n, value, spk, 1, False)
    total = 0
    kw = {"defer_multisig": True} if flag else {}
    for k, blk in enumerate(blocks):
        res, _ = _core.connect_block(blk, k + 1, view, True, True, None, 0, _core.BLOCK_SCRIPT_VERIFY_FLAGS, 1,
                                     defer_sighash=True, defer_all_forms=mode == 2, **kw)
        assert res.ok, res.reject
        total += len((res.sighash_pack_var() if mode == 2 else res.sighash_pack())[0])
    return total


def probe_chain(name, coins, raws, flags, repeats, warmup):
    from nodexa_chain_core_amd import core

    _core = core()
    act = _new_state().params.kawpow_activation_time
    blocks = [_core.Block.deserialize(raw, act) for raw in raws]
    settings = [(f, w, m) for m in MODES for w in WINDOWS for f in flags]
    runs = {s: [] for s in settings}
    rechecks = {s: [] for s in settings}
    stats, utxo = {}, set()
    for i in range(warmup + repeats):
        for s in settings:
            ms, st, h = connect_once(coins, blocks, *s)
            utxo.add(h)
            if i >= warmup:
                runs[s].append(ms)
                rechecks[s].append(st["host_rechecks"])
                stats[s] = st
    assert len(utxo) == 1  # every setting ends with the same UTXO set
    n_inputs = sum(len(tx.vin) for b in blocks for tx in b.vtx[1:])
    out = {"chain": name, "blocks": len(blocks), "inputs": n_inputs, "block_bytes": sum(len(r) for r in raws),
           "settings": []}
    for f, w, m in settings:
        row = dict(_stats(runs[(f, w, m)]), gpumultisig=f, gpusigwindow=w, gpusighash=m,
                   host_rechecks=sorted(set(rechecks[(f, w, m)])), entries=stats[(f, w, m)]["gpu_sigs"],
                   groups=stats[(f, w, m)].get("gpu_multisig_groups", 0),
                   device_passes=stats[(f, w, m)]["gpu_batches"], arena_bytes=arena_bytes(coins, blocks, f, m))
        if f and (0, w, m) in runs:
            base = runs[(0, w, m)]
            row["speedup_median_vs_flag_0"] = round(statistics.median(base) / statistics.median(runs[(f, w, m)]), 2)
            row["verdict_vs_flag_0"] = _differs(runs[(f, w, m)], base)
            assert row["host_rechecks"] == [0], row  # the condition: nothing goes back to the host
        out["settings"].append(row)
    return out


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


def probe_kernels(repeats, warmup, n_inputs=24, sizes=(96, 4032, 16320, 65472)):
    """Device time of sighash_gather_var, secp_verify_batch, sig_group_resolve and
    sig_window_verdicts over windows of 24-input 2-of-3 blocks (four entries per input, every hash
    left to the device) holding about `sizes` entries."""
    import numpy as np
    import torch

    from nodexa_chain_core_amd import core
    from nodexa_chain_core_amd.ops import runtime, secp, sighash
    from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block

    _core = core()
    h = runtime.hip()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = runtime.current_stream_handle()
    distinct = []  # few distinct blocks, repeated: the kernels do not care
    for k in range(16):
        blk, view, height, _ = make_consolidation_block(1, n_inputs, seed=9100 + k, multisig_every=1,
                                                        multisig_signers="cycle")
        res, _ = _core.connect_block(blk, height, view, True, True, None, 0, _core.BLOCK_SCRIPT_VERIFY_FLAGS, 1,
                                     defer_sighash=True, defer_all_forms=True, defer_multisig=True)
        assert res.ok and res.num_sigs == 4 * n_inputs and len(res.sig_groups) == n_inputs
        distinct.append(res)
    out = []
    for n in sizes:
        results = [distinct[k % len(distinct)] for k in range(n // (4 * n_inputs))]
        mode, arena, segs, jobs, secp_jobs, sig_begin, n_dev, _ = _core.sig_window_pack(results)
        table = _core.sig_window_groups(results)
        total = sig_begin[-1]
        _core.sig_group_check(total, table)
        ng = len(table) // sighash.GROUP_BYTES
        d_arena, d_segs, d_jobs = sighash._upload_var(arena, segs, jobs, total, dev)
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        d_groups = torch.frombuffer(bytearray(table), dtype=torch.int32).to(dev)
        verdicts = torch.empty(total, dtype=torch.int32, device=dev)
        gtab = secp._gen_table(dev)
        sb = np.asarray(sig_begin, dtype=np.uint32)
        d_begin = torch.from_numpy(sb.view(np.int32).copy()).to(dev)
        records = torch.empty((len(results), 4), dtype=torch.int32, device=dev)
        kg = runtime.static_kernel("sighash_var", "sighash_gather_var")
        kv = runtime.static_kernel("secp256k1_verify", "secp_verify_batch")
        kp = runtime.static_kernel("sig_group", "sig_group_resolve")
        kr = runtime.static_kernel("sig_window", "sig_window_verdicts")
        gather = _time_kernel(lambda: h.launch_sighash_gather_var(
            kg, d_arena.data_ptr(), d_segs.data_ptr(), len(segs) // sighash.SEG_BYTES, d_jobs.data_ptr(), n_dev, 0,
            d_secp.data_ptr(), stream), warmup, repeats)
        verify = _time_kernel(lambda: h.launch_secp_verify(kv, d_secp.data_ptr(), total, gtab.data_ptr(),
                                                           verdicts.data_ptr(), stream), warmup, repeats)
        raw = verdicts.cpu().numpy().view(np.uint32).tolist()
        # the kernel works in place: after its first launch the repeats walk verdicts that are all 1
        # (the shortest walks). Timed again below over the verifier's raw output, restored each time
        resolve = _time_kernel(lambda: h.launch_sig_group_resolve(kp, verdicts.data_ptr(), d_groups.data_ptr(), ng,
                                                                  stream), warmup, repeats)
        assert verdicts.cpu().numpy().view(np.uint32).tolist() == _core.sig_group_resolve_model(raw, table) == [1] * total
        d_raw = torch.tensor(raw, dtype=torch.int32, device=dev)
        first = []
        for _ in range(repeats):
            verdicts.copy_(d_raw)
            first += _time_kernel(lambda: h.launch_sig_group_resolve(kp, verdicts.data_ptr(), d_groups.data_ptr(), ng,
                                                                     stream), 0, 1)
        recs = _time_kernel(lambda: h.launch_sig_window_verdicts(kr, verdicts.data_ptr(), d_begin.data_ptr(),
                                                                 len(results), records.data_ptr(), stream),
                            warmup, repeats)
        assert records.cpu().numpy().view(np.uint32).tolist() == [[4 * n_inputs, 0, 0, 0xffffffff]] * len(results)
        out.append({"blocks": len(results), "entries": total, "groups": ng, "arena_bytes": len(arena),
                    "valid_pairs": raw.count(1), "sighash_gather_var": _stats(gather), "secp_verify_batch": _stats(verify),
                    "sig_group_resolve": _stats(resolve), "sig_group_resolve_on_raw_verdicts": _stats(first),
                    "sig_window_verdicts": _stats(recs), "group_table_bytes": len(table)})
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", default="512x24", help="blocks x inputs of the small-block chain")
    ap.add_argument("--large", default="64x200", help="blocks x inputs of the large-block chain")
    ap.add_argument("--flags", default="0,1", help="-gpumultisig settings to run")
    ap.add_argument("--cache", default=None, help="directory that keeps the built chains")
    ap.add_argument("--build-only", action="store_true", help="build (and cache) the chains, then stop: needs no GPU")
    ap.add_argument("--sections", default="chains,kernels", help="which parts to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    flags = tuple(int(x) for x in a.flags.split(","))
    from nodexa_chain_core_amd import _build

    _build.build_core()
    from nodexa_chain_core_amd import core

    core().sigcache_set_max_bytes(0)  # as for blocks relayed by peers: no signature known from the mempool
    chains = []
    for name, spec, seed0 in (("small blocks", a.small, 300_000),
                              ("large blocks", a.large, 400_000)) if "chains" in sections else ():
        n_blocks, n_inputs = (int(x) for x in spec.split("x"))
        chains.append((f"{name} ({n_blocks} x {n_inputs} 2-of-3 inputs)",
                       *cached_chain(a.cache, n_blocks, n_inputs, seed0)))
    if a.build_only:
        return 0
    import torch

    if not torch.cuda.is_available():
        print("multisig_probe: no GPU present", file=sys.stderr)
        return 2
    _build.build_all()
    doc = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "flags": list(flags),
           "chains": []}
    for name, coins, raws in chains:
        doc["chains"].append(probe_chain(name, coins, raws, flags, a.repeats, a.warmup))
        print(json.dumps(doc["chains"][-1]), flush=True)
    if "kernels" in sections:
        doc["kernels"] = probe_kernels(a.repeats, a.warmup)
        print(json.dumps(doc["kernels"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
