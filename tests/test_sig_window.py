"""One signature batch per window of blocks (-gpusigwindow), without a GPU: the window packer against
the per-block packers and the kernels' host models, the host definition of the per-block records,
and ChainState's speculative / final connection through a host verifier."""
import pytest

import sig_window_util as W
from test_node_rpc import client, node_factory  # noqa: F401 — shared fixture

MODES = (0, 1, 2)


# ---------------------------------------------------------------- pack
def _per_block(core, res, mode):
    """(arena, segs, jobs, secp_jobs, n_dev, n_host, digests) of one block, from the packer of its mode."""
    if mode == 0:
        return b"", b"", b"", core.secp_pack_jobs(res.sig_items()), 0, res.num_sigs, b""
    if mode == 1:
        arena, jobs, secp_jobs, n_dev, n_host = res.sighash_pack()
        return arena, b"", jobs, secp_jobs, n_dev, n_host, core.sighash_gather_model(arena, jobs)
    arena, segs, jobs, secp_jobs, n_dev, n_host = res.sighash_pack_var()
    return arena, segs, jobs, secp_jobs, n_dev, n_host, core.sighash_var_model(arena, segs, jobs)


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (2, 0, 1, 3, 4)], ids=["empty-third", "empty-first"])
@pytest.mark.parametrize("mode", MODES)
def test_pack_is_the_concatenation_of_the_blocks(core, mode, order):
    results, infos = W.five_blocks(core, mode, order)
    sizes = [r.num_sigs for r in results]
    assert min(s for s in sizes if s) >= 2 and max(sizes) >= 40 and sizes.count(0) == 1
    got_mode, arena, segs, jobs, secp_jobs, sig_begin, n_dev, n_host = core.sig_window_pack(results)
    per = [_per_block(core, r, mode) for r in results]
    assert got_mode == mode
    assert sig_begin == W.sig_begin_of(sizes)
    assert secp_jobs == b"".join(p[3] for p in per)
    assert (n_dev, n_host) == (sum(p[4] for p in per), sum(p[5] for p in per)) and n_dev + n_host == sig_begin[-1]
    assert len(arena) == sum(len(p[0]) for p in per)
    if mode == 0:
        assert arena == segs == jobs == b"" and n_dev == 0
        return
    assert n_dev > 0
    rec = W.JOB if mode == 1 else W.VAR_JOB
    assert len(jobs) == n_dev * rec.size
    if mode == 1:
        assert segs == b""
        core.sighash_check_jobs(len(arena), jobs, sig_begin[-1])
        digests = core.sighash_gather_model(arena, jobs)
    else:
        assert len(segs) == sum(len(p[1]) for p in per)
        core.sighash_var_check(len(arena), segs, jobs, sig_begin[-1])
        digests = core.sighash_var_model(arena, segs, jobs)
    assert digests == b"".join(p[6] for p in per)  # row for row
    # every job fills the entry of its own block
    k = 0
    for b, p in enumerate(per):
        for j in range(len(p[2]) // rec.size):
            mine, theirs = rec.unpack_from(jobs, k * rec.size), rec.unpack_from(p[2], j * rec.size)
            assert mine[-2] == theirs[-2] + sig_begin[b] and mine[-1] == theirs[-1]
            assert sig_begin[b] <= mine[-2] < sig_begin[b + 1]
            k += 1
    assert k == n_dev


def test_pack_of_nothing(core):
    assert core.sig_window_pack([]) == (0, b"", b"", b"", b"", [0], 0, 0)
    results, _ = W.five_blocks(core, 2, order=(2,))
    assert core.sig_window_pack(results + results) == (0, b"", b"", b"", b"", [0, 0, 0], 0, 0)


def test_pack_refuses_mixed_modes_and_an_arena_over_the_limit(core):
    a, _ = W.five_blocks(core, 1, order=(0, 2))
    b, _ = W.five_blocks(core, 2, order=(1,))
    h, _ = W.five_blocks(core, 0, order=(3,))
    for mix in (a + b, b + a, h + a, b + h):
        with pytest.raises(ValueError, match="different"):
            core.sig_window_pack(mix)
    # a block without signatures fits a window of any mode
    empty = [a[1]]
    assert core.sig_window_pack(empty + b)[0] == 2 and core.sig_window_pack(h + empty)[0] == 0
    assert core.SIG_WINDOW_ARENA_LIMIT + core.SIGHASH_ARENA_SLACK == 1 << 31
    results, _ = W.five_blocks(core, 2)
    arena_len = len(core.sig_window_pack(results)[1])
    core.sig_window_pack(results, arena_len + 1)
    with pytest.raises(ValueError, match="limit"):
        core.sig_window_pack(results, arena_len)  # the arena reaches the limit with the last block
    with pytest.raises(ValueError, match="limit"):
        core.sig_window_pack(results, 16)


# ---------------------------------------------------------------- records model
@pytest.mark.parametrize("name,verdicts", W.verdict_patterns(), ids=[n for n, _ in W.verdict_patterns()])
def test_records_model(core, name, verdicts):
    sb = W.sig_begin_of(W.SIZES)
    got = core.sig_window_verdicts_model(verdicts, sb)
    assert len(got) == len(W.SIZES) * core.SIG_WINDOW_RECORD_BYTES == len(W.SIZES) * 16
    assert got == W.records_ref(verdicts, sb)
    rows = [W.RECORD.unpack_from(got, 16 * b) for b in range(len(W.SIZES))]
    assert [r[0] + r[1] + r[2] for r in rows] == list(W.SIZES)
    for b in (0, 5):
        assert rows[b] == (0, 0, 0, core.SIG_WINDOW_NONE)
    if name == "all-valid":
        assert all(r == (n, 0, 0, W.NONE) for r, n in zip(rows, W.SIZES))
    if name.startswith("invalid-"):
        b = int(name.rsplit("-", 1)[1])
        want = 0 if "first" in name else W.SIZES[b] - 1
        assert rows[b] == (W.SIZES[b] - 1, 1, 0, want)
        assert all(r[3] == W.NONE for k, r in enumerate(rows) if k != b)
    if name == "ask-host":
        assert [r[2] for r in rows] == [0, 0, 2, 0, 1, 0, 2] and [r[3] for r in rows][2::2] == [5, 0, 64]
        assert all(r[1] == 0 for r in rows)
    if name == "out-of-range":
        assert [r[1] for r in rows] == [0, 0, 0, 1, 0, 0, 2] and rows[3][3] == 63 and rows[6][3] == 1


def test_records_model_refuses_a_bad_prefix_table(core):
    with pytest.raises(ValueError):
        core.sig_window_verdicts_model([1, 1, 1], [0, 2, 1, 3])
    with pytest.raises(ValueError):
        core.sig_window_verdicts_model([1, 1, 1], [0, 4])
    with pytest.raises(ValueError):
        core.sig_window_verdicts_model([1], [])
    assert core.sig_window_verdicts_model([], [0]) == b""
    assert core.sig_window_verdicts_model([0, 1], [1, 2]) == W.RECORD.pack(1, 0, 0, W.NONE)


# ---------------------------------------------------------------- state machine
@pytest.fixture(scope="module")
def chains(core):
    base, chain = W.build_chain(core)
    params = W.new_state().params
    return {"base": base, "good": chain, "params": params,
            "bad5": W.variant(core, params, chain, {5: W.corrupt_signature}),
            "cb6": W.variant(core, params, chain, {6: W.overpay_community}),
            "bad3cb6": W.variant(core, params, chain, {3: W.corrupt_signature, 6: W.overpay_community})}


class _Events:
    """connect_tip heights, the UTXO hash at each (inside a window the set already holds the window's
    later blocks, all verified), the verifier calls answered by then, and the undo record."""

    def __init__(self, st, calls):
        self.st, self.calls, self.tips = st, calls, []

    def connect_tip(self, block, index, undo):
        self.tips.append((index.height, self.st.coins.stats()[3], len(self.calls), bytes(undo)))


def _run(core, chains, which, window, n_blocks=W.N_CHAIN, datadir=None, verifier=None, flush_interval=None):
    """A node at the base, then the first `n_blocks` of chain `which` in one activation walk. The
    runs without a window are the references: made once, shared, and left unchanged."""
    memo = chains.setdefault("runs", {})
    if not window and datadir is None and (which, n_blocks) in memo:
        return memo[(which, n_blocks)]
    st = W.new_state(datadir)
    W.feed(st, chains["base"])
    assert st.height() == W.N_BASE
    calls = []
    if window:
        st.gpu_signatures = "on"
        st.gpu_sig_window = window
        st.sig_window_verifier = verifier or W.host_verifier(core, calls)
    if flush_interval is not None:
        st.flush_interval = flush_interval
    ev = _Events(st, calls)
    st.register(ev)
    states = W.feed(st, chains[which][:n_blocks], one_walk=True)
    if not window and datadir is None:
        memo[(which, n_blocks)] = (st, ev, calls, states)
    return st, ev, calls, states


def _block_hashes(core, chains, which):
    hc = core.HeaderChain(chains["params"])
    act = chains["params"].kawpow_activation_time
    return [hc.block_hash(core.Block.deserialize(raw, act).header) for raw in chains[which]]


def _undo_records(st, hashes):
    out, prev = [], st.chain.find(hashes[0]).prev_hash
    for h in hashes:
        out.append(st.undo.read(h, prev))
        prev = h
    return out


def test_window_all_valid(core, chains):
    seq, seq_ev, _, _ = _run(core, chains, "good", 0)
    st, ev, calls, states = _run(core, chains, "good", 1000)
    assert all(s.ok for s in states)
    assert st.height() == seq.height() == W.N_BASE + 8 and st.coins.best_block == seq.coins.best_block
    assert st.coins.stats() == seq.coins.stats()
    hashes = _block_hashes(core, chains, "good")
    assert _undo_records(st, hashes) == _undo_records(seq, hashes) and None not in _undo_records(st, hashes)
    # one window: one verifier call over the 8 blocks, block 7 without signatures
    assert calls == [[3, 3, 3, 3, 3, 3, 0, 3]]
    assert [t[0] for t in ev.tips] == [W.N_BASE + k for k in range(1, 9)]
    assert all(t[2] == 1 for t in ev.tips)  # none fired before the verifier returned
    # each event carried the undo record it carries without a window
    assert [t[3] for t in ev.tips] == [t[3] for t in seq_ev.tips]
    # the documented difference: inside a window the UTXO set an event finds already holds the
    # window's later (verified) blocks; only the window's last block finds it as the sequential node does.
    # A listener that needs it exact says so (test_window_ends_where_a_listener_needs_the_exact_state)
    assert all(a[1] != b[1] for a, b in zip(ev.tips[:-1], seq_ev.tips[:-1]))
    assert len({t[1] for t in ev.tips}) == 8  # the best block moves with every event
    assert ev.tips[-1][1] == seq_ev.tips[-1][1]
    s = st.sig_stats
    assert (s["gpu_windows"], s["window_blocks"], s["window_sigs"], s["window_rollbacks"]) == (1, 8, 21, 0)
    assert s["gpu_batches"] == 1 and s["gpu_sigs"] == 21 and s["host_rechecks"] == 0
    assert seq.sig_stats["gpu_windows"] == 0 and seq.sig_stats["gpu_sigs"] == 0


@pytest.mark.parametrize("mode", (1, 2))
def test_window_defers_the_hashes_as_the_flag_says(core, chains, mode):
    seq, _, _, _ = _run(core, chains, "good", 0)
    seen = []

    def verifier(results):
        seen.append([(r.all_forms, r.num_device_hashes, r.num_sigs) for r in results])
        assert core.sig_window_pack(results)[0] == mode
        return W.host_verifier(core)(results)

    st = W.new_state()
    W.feed(st, chains["base"])
    st.gpu_signatures, st.gpu_sig_window, st.sig_window_verifier = "on", 1000, verifier
    st.gpu_sighash, st.gpu_sighash_forms = True, "all" if mode == 2 else "legacy-all"
    assert all(s.ok for s in W.feed(st, chains["good"], one_walk=True))
    assert st.coins.stats() == seq.coins.stats()
    assert len(seen) == 1 and all(af == (mode == 2) for af, _, _ in seen[0])
    n_dev = sum(d for _, d, _ in seen[0])
    # mode 1 leaves the legacy ALL-form hashes to the device, mode 2 all of them
    assert (n_dev == 21) if mode == 2 else (0 < n_dev < 21)
    assert st.sig_stats["gpu_sighashes"] == n_dev and st.sig_stats["host_sighashes"] == 21 - n_dev


def test_window_with_a_corrupted_signature_in_block_5(core, chains):
    seq, _, _, seq_states = _run(core, chains, "bad5", 0)
    at4, _, _, _ = _run(core, chains, "good", 0, n_blocks=4)
    st, ev, calls, states = _run(core, chains, "bad5", 1000)
    assert st.height() == seq.height() == W.N_BASE + 4
    assert st.coins.stats() == seq.coins.stats() == at4.coins.stats()
    hashes = _block_hashes(core, chains, "bad5")
    assert st.coins.best_block == hashes[3]
    assert st.chain.tip().hash == hashes[3]  # 5 and its descendants are out of the best chain
    assert calls == [[3, 3, 3, 3, 3, 3, 0, 3]]
    assert st.sig_stats["window_rollbacks"] == 1 and st.sig_stats["host_rechecks"] == 1
    assert [t[0] for t in ev.tips] == [W.N_BASE + k for k in range(1, 5)]  # no event for a block >= 5
    for h in hashes[4:]:
        assert h not in st.undo.pos  # and no undo write
    assert _undo_records(st, hashes[:4]) == _undo_records(seq, hashes[:4])
    assert states[-1].ok  # block 8 itself is stored; the walk's failure is block 5's
    # the node goes on from block 4: the good blocks 5..8 connect on top
    assert all(s.ok for s in W.feed(st, chains["good"][4:]))
    full, _, _, _ = _run(core, chains, "good", 0)
    assert st.coins.stats() == full.coins.stats()


def test_window_reports_block_5_as_the_per_block_path_does(core, chains):
    """Block 5 as the walk's last block: process_new_block returns its state."""
    seq, _, _, seq_states = _run(core, chains, "bad5", 0, n_blocks=5)
    st, _, calls, states = _run(core, chains, "bad5", 1000, n_blocks=5)
    assert calls == [[3, 3, 3, 3, 3]] and st.sig_stats["window_rollbacks"] == 1  # found by the window
    assert not states[-1].ok and (states[-1].reject, states[-1].dos) == (seq_states[-1].reject, seq_states[-1].dos)
    assert states[-1].reject.startswith("mandatory-script-verify-flag-failed (") and states[-1].dos == 100
    assert st.height() == seq.height() == W.N_BASE + 4 and st.coins.stats() == seq.coins.stats()


def test_window_with_a_bad_coinbase_amount_in_block_6(core, chains):
    seq, _, _, seq_states = _run(core, chains, "cb6", 0, n_blocks=6)
    st, ev, calls, states = _run(core, chains, "cb6", 1000, n_blocks=6)
    assert st.height() == seq.height() == W.N_BASE + 5 and st.coins.stats() == seq.coins.stats()
    assert not states[-1].ok and states[-1].reject == seq_states[-1].reject == "bad-cb-community-autonomous-amount"
    assert calls == [[3, 3, 3, 3, 3]]  # the window before it was verified first
    assert st.sig_stats["window_rollbacks"] == 0
    assert [t[0] for t in ev.tips] == [W.N_BASE + k for k in range(1, 6)]
    # and with the blocks after it stored too
    st8, _, _, _ = _run(core, chains, "cb6", 1000)
    assert st8.height() == W.N_BASE + 5 and st8.coins.stats() == seq.coins.stats()


def test_window_an_earlier_bad_signature_wins(core, chains):
    seq, _, _, _ = _run(core, chains, "bad3cb6", 0)
    st, ev, calls, _ = _run(core, chains, "bad3cb6", 1000)
    assert st.height() == seq.height() == W.N_BASE + 2 and st.coins.stats() == seq.coins.stats()
    assert calls == [[3, 3, 3, 3, 3]]  # blocks 1..5, closed by block 6's failure
    assert st.sig_stats["window_rollbacks"] == 1
    assert [t[0] for t in ev.tips] == [W.N_BASE + 1, W.N_BASE + 2]
    hashes = _block_hashes(core, chains, "bad3cb6")
    assert st.chain.tip().hash == hashes[1]


class _NeedsExact(_Events):
    """A listener that reads the UTXO set and the asset state at some heights' connect_tip."""

    def __init__(self, st, calls, heights):
        super().__init__(st, calls)
        self.heights, self.asked = set(heights), []

    def needs_exact_state(self, block, index):
        self.asked.append(index.height)
        return index.height in self.heights


class _Broken(_Events):
    def needs_exact_state(self, block, index):
        raise RuntimeError("no answer")


def test_window_ends_where_a_listener_needs_the_exact_state(core, chains):
    seq, seq_ev, _, _ = _run(core, chains, "good", 0)
    by_height = {t[0]: t[1] for t in seq_ev.tips}
    st = W.new_state()
    W.feed(st, chains["base"])
    calls = []
    st.gpu_signatures, st.gpu_sig_window, st.sig_window_verifier = "on", 1000, W.host_verifier(core, calls)
    ev = _NeedsExact(st, calls, (W.N_BASE + 2, W.N_BASE + 5))
    st.register(ev)
    assert all(s.ok for s in W.feed(st, chains["good"], one_walk=True))
    assert ev.asked == [W.N_BASE + k for k in range(1, 9)]
    assert calls == [[3, 3], [3, 3, 3], [3, 0, 3]]  # blocks 2 and 5 are the last of their windows
    seen = {t[0]: t[1] for t in ev.tips}
    for h in (W.N_BASE + 2, W.N_BASE + 5, W.N_BASE + 8):
        assert seen[h] == by_height[h]  # the UTXO set of exactly that block, as on the sequential node
    assert seen[W.N_BASE + 1] != by_height[W.N_BASE + 1]
    assert st.coins.stats() == seq.coins.stats()
    # a listener whose answer fails counts as asking: every block is its own window
    st2 = W.new_state()
    W.feed(st2, chains["base"])
    calls2 = []
    st2.gpu_signatures, st2.gpu_sig_window, st2.sig_window_verifier = "on", 1000, W.host_verifier(core, calls2)
    ev2 = _Broken(st2, calls2)
    st2.register(ev2)
    W.feed(st2, chains["good"], one_walk=True)
    assert calls2 == [[3]] * 7  # the block without signatures is a window that asks the verifier nothing
    assert [t[1] for t in ev2.tips] == [t[1] for t in seq_ev.tips]


def test_reward_snapshot_inside_a_windowed_walk_is_the_sequential_one(core, chains):
    """wallet/rewards.py takes its snapshot in connect_tip from the asset state of that moment: a
    height with a snapshot request ends its window, so the state read is that block's."""
    from nodexa_chain_core_amd.wallet.rewards import Rewards

    class Recording(Rewards):
        def __init__(self, state):
            super().__init__(state, None, None, None)
            self.taken = []

        def take_snapshot(self, name, height):
            tip_height = self.state.chain.find(self.state.coins.best_block).height
            self.taken.append((name, height, tip_height, self.state.coins.stats()[3],
                               sorted(self.state.assets.balances())))
            return super().take_snapshot(name, height)

    def walk(window):
        st = W.new_state()
        W.feed(st, chains["base"])
        calls = []
        if window:
            st.gpu_signatures, st.gpu_sig_window, st.sig_window_verifier = "on", window, W.host_verifier(core, calls)
        r = Recording(st)
        assert not r.needs_exact_state(None, st.chain.find(st.coins.best_block))
        r.schedule("TOKEN", W.N_BASE + 4)
        r.schedule("OTHER", W.N_BASE + 4)
        r.schedule("TOKEN", W.N_BASE + 6)
        st.register(r)
        assert all(s.ok for s in W.feed(st, chains["good"], one_walk=True))
        return r.taken, calls

    seq_taken, _ = walk(0)
    win_taken, calls = walk(1000)
    assert [(n, h, t) for n, h, t, _, _ in seq_taken] == [("OTHER", W.N_BASE + 4, W.N_BASE + 4),
                                                          ("TOKEN", W.N_BASE + 4, W.N_BASE + 4),
                                                          ("TOKEN", W.N_BASE + 6, W.N_BASE + 6)]
    assert win_taken == seq_taken  # the same UTXO set and asset balances at each snapshot
    assert calls == [[3, 3, 3, 3], [3, 3], [0, 3]]


def test_window_of_8_signatures(core, chains):
    seq, seq_ev, _, _ = _run(core, chains, "good", 0)
    st, ev, calls, _ = _run(core, chains, "good", 8)
    assert calls == [[3, 3, 3], [3, 3, 3], [0, 3]]
    assert st.coins.stats() == seq.coins.stats() and st.height() == W.N_BASE + 8
    assert [(t[0], t[3]) for t in ev.tips] == [(t[0], t[3]) for t in seq_ev.tips]
    assert [t[2] for t in ev.tips] == [1, 1, 1, 2, 2, 2, 3, 3]
    assert st.sig_stats["gpu_windows"] == 3 and st.sig_stats["window_blocks"] == 8
    # the bad block in the second window: the first one stays, the walk ends at 4
    bad, _, calls, _ = _run(core, chains, "bad5", 8)
    at4, _, _, _ = _run(core, chains, "good", 0, n_blocks=4)
    assert calls == [[3, 3, 3], [3, 3, 3]] and bad.coins.stats() == at4.coins.stats()


def test_window_total_below_the_batch_minimum_stays_on_the_host(core, chains):
    st = W.new_state()
    W.feed(st, chains["base"])
    calls = []
    st.gpu_signatures, st.gpu_sig_window, st.sig_window_verifier = "auto", 1000, W.host_verifier(core, calls)
    W.feed(st, chains["good"][:3], one_walk=True)  # 9 signatures < GPU_SIG_BATCH_MIN
    assert st.height() == W.N_BASE + 3 and calls == [] and st.sig_stats["gpu_windows"] == 0
    W.feed(st, chains["good"][3:], one_walk=True)  # 12 more: still below; -gpusigs=on takes any
    assert st.height() == W.N_BASE + 8 and calls == []
    st2, _, calls2, _ = _run(core, chains, "good", 1000, n_blocks=2)
    assert calls2 == [[3, 3]]


def test_window_never_flushes_an_unverified_block(core, chains, tmp_path):
    seq, seq_ev, _, _ = _run(core, chains, "good", 0)
    by_height = {t[0]: t[1] for t in seq_ev.tips}
    flushed = []
    st2 = W.new_state(str(tmp_path / "b"))
    W.feed(st2, chains["base"])
    st2.flush()
    # from here on every block asks for a flush
    st2.gpu_signatures, st2.gpu_sig_window, st2.flush_interval = "on", 8, 1
    calls = []
    st2.sig_window_verifier = W.host_verifier(core, calls)
    real = st2.flush

    def flush():
        tip = st2.coins_tip()
        flushed.append((tip.height, st2.coins.stats()[3], len(calls)))
        real()

    st2.flush = flush
    W.feed(st2, chains["good"], one_walk=True)
    assert st2.height() == W.N_BASE + 8
    # a flush only at the end of a verified window, with exactly that block's UTXO set
    assert [f[0] - W.N_BASE for f in flushed] == [3, 6, 8] and [f[2] for f in flushed] == [1, 2, 3]
    assert all(f[1] == by_height[f[0]] for f in flushed)
    st2.close()
    again = W.new_state(str(tmp_path / "b"))
    assert again.height() == W.N_BASE + 8 and again.coins.stats() == seq.coins.stats()
    again.close()


def test_window_verifier_that_raises(core, chains):
    at3, _, _, _ = _run(core, chains, "good", 0, n_blocks=3)
    n = []

    def verifier(results):
        n.append(len(results))
        if len(n) == 2:
            raise RuntimeError("device lost")
        return W.host_verifier(core)(results)

    st = W.new_state()
    W.feed(st, chains["base"])
    st.gpu_signatures, st.gpu_sig_window, st.sig_window_verifier = "on", 8, verifier
    ev = _Events(st, n)
    st.register(ev)
    with pytest.raises(RuntimeError, match="device lost"):
        W.feed(st, chains["good"], one_walk=True)
    # the first window is final, the second one is rolled back: the UTXO set is at block 3
    assert st.height() == W.N_BASE + 3 and st.coins.stats() == at3.coins.stats()
    assert [t[0] - W.N_BASE for t in ev.tips] == [1, 2, 3]
    # and the node recovers once the verifier does
    st.sig_window_verifier = W.host_verifier(core)
    with st.lock:
        st._activate()
    full, _, _, _ = _run(core, chains, "good", 0)
    assert st.height() == W.N_BASE + 8 and st.coins.stats() == full.coins.stats()


def test_gpusigwindow_flag(core, node_factory):
    import torch

    st = W.new_state()
    assert st.gpu_sig_window == 0 and st.sig_window_verifier is None and not st._sig_window_on()
    assert {"gpu_windows", "window_blocks", "window_sigs", "window_rollbacks"} <= set(st.sig_stats)
    st.gpu_sig_window = 64
    assert not st._sig_window_on()  # -gpusigs=off: nothing to act on
    st.gpu_signatures = "on"
    st.sig_window_verifier = lambda results: [[] for _ in results]
    assert st._sig_window_on()
    # as -gpusighash: a node that does not take the GPU batch (no GPU here, or the batch switched off
    # where there is one) ignores the flag and connects its blocks on the host
    sigs = "-gpusigs=off" if torch.cuda.is_available() else "-gpusigs=on"
    node, addr = node_factory((sigs, "-gpusigwindow=64", "-maxsigcachesize=0"))
    assert node.state.gpu_sig_window == 64 and not node.state._sig_window_on()
    c = client(node)
    w = c.getnewaddress()
    c.generatetoaddress(101, w)
    c.sendtoaddress(c.getnewaddress(), 1.0)
    c.generatetoaddress(1, w)
    assert c.getblockcount() == 102 and c.getrawmempool() == []
    info = c.getgpuinfo()[0]["block_sigs"]
    assert info == node.state.sig_stats and info["gpu_windows"] == info["window_rollbacks"] == 0


def test_records_kernel_keeps_to_registers(tmp_path):
    """sig_window_verdicts reduces across lanes in registers: the compiler's resource report for the
    gfx950 code object shows no scratch, no spills and no LDS, at full occupancy."""
    import os
    import re
    import subprocess

    from nodexa_chain_core_amd import _build

    hipcc = os.path.join(_build.ROCM, "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    kdir = os.path.join(_build.HIPDIR, "kernels")
    r = subprocess.run([hipcc, "--genco", "--offload-arch=" + _build.ARCH, "-O3", "-std=c++17",
                        "-mcode-object-version=5", "-I" + kdir, "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(kdir, "sig_window.hip"), "-o", str(tmp_path / "sig_window.hsaco")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rep = r.stderr[r.stderr.index("Function Name: sig_window_verdicts"):]
    usage = {k.strip(): v for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\w+) \[-Rpass", rep)}
    assert usage["ScratchSize [bytes/lane]"] == "0" and usage["Dynamic Stack"] == "False"
    assert usage["VGPRs Spill"] == "0" and usage["SGPRs Spill"] == "0" and usage["LDS Size [bytes/block]"] == "0"
    assert int(usage["VGPRs"]) <= 32 and usage["Occupancy [waves/SIMD]"] == "8"
