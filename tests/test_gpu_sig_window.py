"""One signature batch per window of blocks on a real MI355X: sig_window_verdicts against its host
model, ops/sighash.verify_window against the per-block paths in every -gpusighash mode, and a chain
state that connects and refuses blocks with -gpusigwindow."""
import pytest

import sig_window_util as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def patterns():
    return W.verdict_patterns()


def test_verdict_records_match_the_model(gpu, core, patterns):
    from nodexa_chain_core_amd.ops import sighash

    sb = W.sig_begin_of(W.SIZES)
    for name, verdicts in patterns:
        want = core.sig_window_verdicts_model(verdicts, sb)
        assert want == W.records_ref(verdicts, sb), name
        assert sighash.verdict_records(verdicts, sb) == want, name  # byte for byte
        assert sighash.verdict_records(verdicts, sb) == want, name  # deterministic


def test_verdict_records_shapes(gpu, core):
    """More than one workgroup (four blocks each), a block of tens of thousands of signatures, empty
    blocks at both ends, a table that starts past 0, and no block at all."""
    from nodexa_chain_core_amd.ops import sighash

    sizes = (0,) + tuple((k * 37) % 131 for k in range(9)) + (60_000, 0, 5, 0)
    sb = W.sig_begin_of(sizes)
    verdicts = [(1, 1, 1, 0, 2, 1, 9)[(k * 11 + k // 64) % 7] for k in range(sb[-1])]
    assert sighash.verdict_records(verdicts, sb) == core.sig_window_verdicts_model(verdicts, sb)
    ones = [1] * sb[-1]
    ones[sb[10] + 59_999] = 0  # the last signature of the large block
    got = sighash.verdict_records(ones, sb)
    assert got == core.sig_window_verdicts_model(ones, sb)
    assert W.RECORD.unpack_from(got, 16 * 10) == (59_999, 1, 0, 59_999)
    assert sighash.verdict_records([0, 1, 2, 1], [1, 3, 4]) == core.sig_window_verdicts_model([0, 1, 2, 1], [1, 3, 4])
    assert sighash.verdict_records([], [0, 0, 0]) == W.RECORD.pack(0, 0, 0, W.NONE) * 2
    assert sighash.verdict_records([1, 1], [0]) == b""
    with pytest.raises(ValueError):
        sighash.verdict_records([1, 1], [0, 3])
    with pytest.raises(ValueError):
        sighash.verdict_records([1, 1], [0, 2, 1])


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_verify_window_matches_the_blocks(gpu, core, mode):
    from nodexa_chain_core_amd.ops import secp, sighash

    bad_block, bad_input = 3, 21  # a P2PKH input signed ALL: hashed on the device in modes 1 and 2
    results, infos = W.five_blocks(core, mode, bad=(bad_block, bad_input))
    got = sighash.verify_window(results)
    if mode == 0:
        want = [secp.verify_batch(r.sig_items()) for r in results]
    else:
        want = [sighash.verify_block_sigs(r) for r in results]
    assert got == want
    assert got == [[bool(core.secp_verify(*it)) for it in r.sig_items()] for r in results]
    bad_sig = infos[bad_block]["bad_sig"]
    assert [[k for k, v in enumerate(b) if not v] for b in got] == [[], [], [], [bad_sig], []]
    records = sighash.window_records(results)
    sizes = [r.num_sigs for r in results]
    assert records[bad_block] == (sizes[bad_block] - 1, 1, 0, bad_sig)
    assert [records[b] for b in (0, 1, 2, 4)] == [(sizes[b], 0, 0, W.NONE) for b in (0, 1, 2, 4)]
    # all valid, the block without signatures first; and a window without any signature
    results, _ = W.five_blocks(core, mode, order=(2, 0, 1, 3, 4))
    assert sighash.verify_window(results) == [[True] * r.num_sigs for r in results]
    assert sighash.verify_window(results[:1]) == [[]] and sighash.window_records(results[:1]) == [(0, 0, 0, W.NONE)]
    assert sighash.verify_window([]) == []


@pytest.fixture(scope="module")
def chains(core):
    base, chain = W.build_chain(core)
    return {"base": base, "good": chain,
            "bad5": W.variant(core, W.new_state().params, chain, {5: W.corrupt_signature})}


def _node(chains, window, sighash_mode):
    st = W.new_state()
    W.feed(st, chains["base"])
    st.gpu_signatures = "on"
    st.gpu_sig_window = window
    st.gpu_sighash, st.gpu_sighash_forms = sighash_mode >= 1, "all" if sighash_mode == 2 else "legacy-all"
    return st


@pytest.mark.parametrize("sighash_mode", (0, 2))
def test_chain_state_connects_and_refuses_with_a_window(gpu, core, chains, sighash_mode):
    off = _node(chains, 0, sighash_mode)
    assert all(s.ok for s in W.feed(off, chains["good"], one_walk=True))
    on = _node(chains, 64, sighash_mode)
    assert on.sig_window_verifier is None and on._sig_window_on()
    assert all(s.ok for s in W.feed(on, chains["good"], one_walk=True))
    assert on.height() == off.height() == W.N_BASE + 8 and on.coins.stats() == off.coins.stats()
    s = on.sig_stats
    assert (s["gpu_windows"], s["window_blocks"], s["window_sigs"], s["window_rollbacks"]) == (1, 8, 21, 0)
    assert s["gpu_sigs"] == 21 and s["host_rechecks"] == 0 and off.sig_stats["gpu_windows"] == 0
    assert s["gpu_sighashes"] == (21 if sighash_mode == 2 else 0) == off.sig_stats["gpu_sighashes"]
    # the variant with a corrupted signature in block 5: both end at block 4
    off = _node(chains, 0, sighash_mode)
    W.feed(off, chains["bad5"], one_walk=True)
    on = _node(chains, 64, sighash_mode)
    W.feed(on, chains["bad5"], one_walk=True)
    assert on.height() == off.height() == W.N_BASE + 4 and on.coins.stats() == off.coins.stats()
    assert on.sig_stats["window_rollbacks"] == 1 and on.sig_stats["host_rechecks"] == 1
    assert on.chain.tip().hash == off.chain.tip().hash
