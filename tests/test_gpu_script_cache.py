"""The script-execution cache (-scriptcache) in front of the GPU batch on a real MI355X: blocks whose
deferred signatures have holes in them (cached transactions leave no signature, template, forms
entry or CHECKMULTISIG group) through every deferred path, a block with nothing left for the device,
a bad signature among hits, and a window whose middle block is fully cached."""
import pytest

import script_cache_util as S
import sig_window_util as W

pytestmark = pytest.mark.gpu

# (-gpusighash, -gpumultisig)
PATHS = ((0, 0), (1, 0), (2, 0), (2, 1))


def _set_path(st, sighash_mode, multisig, window=0):
    st.gpu_signatures = "on"
    st.gpu_sighash, st.gpu_sighash_forms = sighash_mode >= 1, "all" if sighash_mode == 2 else "legacy-all"
    st.gpu_multisig = multisig
    st.gpu_sig_window = window


@pytest.fixture(autouse=True)
def _clean_caches(core):
    # the bound is process-wide and every Node sets it (a test with -maxsigcachesize=0 leaves 0)
    core.scriptcache_set_max_bytes(16 << 20)
    core.sigcache_set_max_bytes(32 << 20)
    yield
    core.scriptcache_clear()
    core.sigcache_clear()


@pytest.fixture(scope="module")
def blocks(core):
    """One block of 8 transactions on the base. Positions 0, 3 and 7 (first, interior, last) never
    saw a mempool: a 2-of-3 P2SH input signed by its keys 1 and 3, a P2WPKH input and a legacy input
    signed SINGLE|ANYONECANPAY. The other five were accepted by the node that assembled the block.
    "bad" is the same block with the signature of transaction 3 corrupted. The references are what a
    -scriptcache=0 node on the host makes of both."""
    fx = S.make_base(core)
    cached = [S.pay(core, fx, n) for n in (2, 4, 7, 5, 11)]  # P2PKH and P2WPKH
    fresh3 = {0: S.pay_multisig(core, fx, 0, signers=(0, 2)), 3: S.pay(core, fx, 15), 7: S.pay(core, fx, 6, 0x83)}
    builder = S.fresh(fx)
    S.accept(builder, cached)
    good = S.assemble(core, builder, edit=S.put_at(fresh3))
    bad = S.assemble(core, builder, edit=S.put_at({**fresh3, 3: S.corrupt(S.pay(core, fx, 15))}))
    vtx = S.block_of(core, fx, good).vtx
    assert len(vtx) == 9 and [vtx[1 + p].txid() for p in (0, 3, 7)] == [fresh3[p].txid() for p in (0, 3, 7)]
    ref = S.fresh(fx)
    assert all(s.ok for s in W.feed(ref, [good]))
    ref_bad = S.fresh(fx)
    bad_state = W.feed(ref_bad, [bad])[0]
    assert not bad_state.ok and bad_state.reject.startswith("mandatory-script-verify-flag-failed (")
    return {"fx": fx, "cached": cached, "fresh": [fresh3[p] for p in (0, 3, 7)], "good": good, "bad": bad,
            "tip": ref.coins.best_block, "utxo": ref.coins.stats(), "bad_reject": (bad_state.reject, bad_state.dos),
            "scratch": S.fresh(fx)}


def _uncached_entries(core, blocks, sighash_mode, multisig):
    """What the three uncached transactions alone leave for the batch: the deferred entries of the
    block reduced to them, connected without the cache (and taken off the scratch view again)."""
    st = blocks["scratch"]
    small = S.block_of(core, blocks["fx"], blocks["good"])
    vtx = list(small.vtx)
    small.vtx = [vtx[0], vtx[1], vtx[4], vtx[8]]
    res, undo = core.connect_block(small, S.N_BASE + 1, st.coins, True, True, None, 0, core.BLOCK_SCRIPT_VERIFY_FLAGS,
                                   4, defer_sighash=sighash_mode >= 1, defer_all_forms=sighash_mode == 2,
                                   defer_multisig=bool(multisig), script_cache=False, sigcache=False)
    assert res.ok, res.reject
    assert core.disconnect_block(small, undo, st.coins)
    return res.num_sigs


def _node(core, blocks, in_mempool, sighash_mode, multisig):
    core.scriptcache_clear()
    core.sigcache_clear()  # under -gpusighash=0 the signature cache would answer for what it has seen
    st = S.fresh(blocks["fx"], script_cache=True)
    S.accept(st, in_mempool)
    assert core.scriptcache_stats()["entries"] == len(in_mempool)
    _set_path(st, sighash_mode, multisig)
    return st


@pytest.mark.parametrize("sighash_mode,multisig", PATHS)
def test_every_deferred_path_skips_the_cached_transactions(gpu, core, blocks, sighash_mode, multisig):
    want = _uncached_entries(core, blocks, sighash_mode, multisig)
    assert want >= 4  # two signatures at least for the 2-of-3, one for each of the others
    st = _node(core, blocks, blocks["cached"], sighash_mode, multisig)
    before = dict(st.sig_stats)
    assert all(s.ok for s in W.feed(st, [blocks["good"]]))
    d = {k: st.sig_stats[k] - before[k] for k in before}
    assert d["gpu_sigs"] == want and d["gpu_batches"] == 1
    assert d["script_cache_txs"] == 5 and d["script_cache_blocks"] == 1
    assert d["gpu_sighashes"] + d["host_sighashes"] == want
    if multisig:  # signed by keys 1 and 3: the pairing walk on the device finds them
        assert d["gpu_multisig_groups"] == 1 and d["host_rechecks"] == 0
    else:         # signature k against key k only: the host settles that input
        assert d["host_rechecks"] == 1
    assert st.height() == S.N_BASE + 1 and st.coins.best_block == blocks["tip"]
    assert st.coins.stats() == blocks["utxo"]
    assert core.scriptcache_stats()["entries"] == 0  # erased once the block was final


def test_a_fully_cached_block_starts_no_device_pass(gpu, core, blocks):
    st = _node(core, blocks, blocks["cached"] + blocks["fresh"], 2, 1)
    before = dict(st.sig_stats)
    assert all(s.ok for s in W.feed(st, [blocks["good"]]))
    d = {k: st.sig_stats[k] - before[k] for k in before}
    assert d["gpu_batches"] == d["gpu_sigs"] == d["host_rechecks"] == 0 and d["script_cache_txs"] == 8
    assert st.coins.best_block == blocks["tip"] and st.coins.stats() == blocks["utxo"]


@pytest.mark.parametrize("sighash_mode,multisig", ((0, 0), (2, 1)))
def test_a_bad_signature_among_hits_is_refused(gpu, core, blocks, sighash_mode, multisig):
    st = _node(core, blocks, blocks["cached"], sighash_mode, multisig)
    before = dict(st.sig_stats)
    state = W.feed(st, [blocks["bad"]])[0]
    assert not state.ok and (state.reject, state.dos) == blocks["bad_reject"]
    assert st.sig_stats["host_rechecks"] > before["host_rechecks"]
    assert st.sig_stats["gpu_batches"] == before["gpu_batches"] + 1
    assert st.height() == S.N_BASE and st.sig_stats["script_cache_txs"] == before["script_cache_txs"]
    flags = core.BLOCK_SCRIPT_VERIFY_FLAGS
    assert all(core.scriptcache_contains(tx.wtxid(), flags) for tx in blocks["cached"])  # nothing erased


@pytest.mark.parametrize("sighash_mode,multisig", ((0, 0), (2, 1)))
def test_window_with_a_fully_cached_middle_block(gpu, core, blocks, sighash_mode, multisig):
    fx = blocks["fx"]
    core.scriptcache_clear()
    st = S.fresh(fx, script_cache=True)
    per_block = [[S.pay(core, fx, n) for n in ns] for ns in ((8, 3), (9, 19), (10, 23, 12))]
    raws = []
    for txs in per_block:  # three stored blocks, connected on the host
        S.accept(st, txs)
        raws.append(S.assemble(core, st))
        assert all(s.ok for s in W.feed(st, raws[-1:]))
    hashes = [S.block_hash(core, fx, raw) for raw in raws]
    utxo = st.coins.stats()
    _set_path(st, sighash_mode, multisig, window=64)
    assert st.sig_window_verifier is None and st._sig_window_on()
    st.invalidate_block(hashes[0])
    assert st.height() == S.N_BASE and len(st.mempool) == 7
    # the node forgets all but the middle block's transactions
    st.clear_mempool()
    core.scriptcache_clear()
    core.sigcache_clear()
    S.accept(st, per_block[1])
    before = dict(st.sig_stats)
    st.reconsider_block(hashes[0])
    d = {k: st.sig_stats[k] - before[k] for k in before}
    assert st.height() == S.N_BASE + 3 and st.coins.best_block == hashes[2] and st.coins.stats() == utxo
    assert d["gpu_windows"] == 1 and d["window_blocks"] == 3 and d["window_rollbacks"] == 0
    assert d["window_sigs"] == d["gpu_sigs"] == 2 + 3  # one signature per input of blocks 1 and 3
    assert d["script_cache_txs"] == 2 and d["script_cache_blocks"] == 1 and d["host_rechecks"] == 0
    assert core.scriptcache_stats()["entries"] == 0
