"""-gpumultisig on the host: the group table's check and model against an oracle of CHECKMULTISIG's
walk, connect_block(defer_multisig=True) over every shape, signer subset, script kind and
-gpusighash mode, the fallbacks, the failures, the window's table and ChainState with a host
verifier. The kernel itself is test_gpu_sig_groups.py's."""
import hashlib

import pytest
import sig_groups_util as G
import sig_window_util as W
from test_node_rpc import client, node_factory  # noqa: F401 — shared fixture

from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block


# ---------------------------------------------------------------- 1. the model against the oracle
@pytest.fixture(scope="module")
def exhaustive5():
    return G.exhaustive(5)


def test_model_exhaustive_up_to_5_keys(core, exhaustive5):
    x = exhaustive5
    assert len(x.groups) > 1200 and {G.OK, G.FAIL} <= set(x.want)
    assert core.sig_group_resolve_model(x.v, x.table()) == x.want


def test_model_seeded_shapes(core):
    x = G.seeded()
    assert {(m, n) for _, m, n in x.groups} == set(G.SEEDED_SHAPES)
    assert G.pairs(8, 15) == core.SIG_GROUP_MAX_PAIRS == 64
    got = core.sig_group_resolve_model(x.v, x.table())
    assert got == x.want
    # every outcome occurs, and the sentinels around the groups are as they were
    assert {G.OK, G.FAIL, G.ASK} <= {x.want[first] for first, _, _ in x.groups}
    assert got.count(G.SENTINEL) == x.v.count(G.SENTINEL) > len(x.groups) // 2


def test_model_ignores_what_the_walk_never_reads(core):
    # 2-of-3, w = 2: entries (s0,k0) (s0,k1) (s1,k1) (s1,k2). s0 matches k0, s1 matches k1: the walk
    # reads entries 0 and 2 only, so a 2 (or anything else) in entries 1 and 3 changes nothing
    for junk in (2, 0, 1, 0xffffffff):
        assert core.sig_group_resolve_model([1, junk, 1, junk], G.table([(0, 2, 3)])) == [1, 1, 1, 1]
    # s0 fails k0, matches k1; s1 then needs k2: entry 2 is never read
    assert core.sig_group_resolve_model([0, 1, 2, 1], G.table([(0, 2, 3)])) == [1, 1, 1, 1]
    # a 2 the walk does read asks the host, and a failed walk before it does not
    assert core.sig_group_resolve_model([0, 1, 0, 2], G.table([(0, 2, 3)])) == [2, 2, 2, 2]
    assert core.sig_group_resolve_model([0, 0, 2, 2], G.table([(0, 2, 3)])) == [0, 0, 0, 0]
    # 3 and 0xffffffff are failed checks, not valid ones
    assert core.sig_group_resolve_model([3, 0xffffffff], G.table([(0, 1, 2)])) == [0, 0]
    assert core.sig_group_resolve_model([3, 1], G.table([(0, 1, 2)])) == [1, 1]


def test_model_empty_table_and_the_stop_rule(core):
    assert core.sig_group_resolve_model([], b"") == []
    assert core.sig_group_resolve_model([0, 2, 7], b"") == [0, 2, 7]
    # the walk stops as soon as fewer keys than signatures are left: 2-of-2 with the first pair
    # invalid fails without reading the second (a 2 there is not reached)
    assert core.sig_group_resolve_model([0, 2], G.table([(0, 2, 2)])) == [0, 0]
    # and it goes on while as many keys as signatures are left: 1-of-2, the first key failing
    assert core.sig_group_resolve_model([0, 1], G.table([(0, 1, 2)])) == [1, 1]
    # groups back to back, the last one ending at the last verdict
    assert core.sig_group_resolve_model([1, 0, 0, 5], G.table([(0, 1, 1), (1, 1, 2), (3, 1, 1)])) == [1, 0, 0, 0]


# ---------------------------------------------------------------- 2. the check
@pytest.mark.parametrize("name,n,groups", [
    ("no-signature", 8, [(0, 0, 3)]),
    ("more-signatures-than-keys", 8, [(0, 3, 2)]),
    ("21-keys", 64, [(0, 21, 21)]),
    ("21-keys-one-signature", 64, [(0, 1, 21)]),
    ("65-pairs", 128, [(0, 5, 17)]),       # 5 x 13
    ("10-of-20", 128, [(0, 10, 20)]),      # 110 pairs
    ("past-the-verdicts", 5, [(2, 2, 3)]),
    ("past-the-verdicts-by-first", 4, [(0xfffffffe, 2, 3)]),
    ("overlap", 16, [(0, 2, 3), (3, 2, 3)]),
    ("descend", 16, [(4, 2, 3), (0, 2, 3)]),
    ("same-first", 16, [(4, 1, 1), (4, 1, 1)]),
])
def test_check_refuses(core, name, n, groups):
    with pytest.raises(ValueError):
        core.sig_group_check(n, G.table(groups))
    with pytest.raises(ValueError):
        core.sig_group_resolve_model([1] * min(n, 128), G.table(groups))


def test_check_refuses_a_truncated_table_and_takes_the_limits(core):
    t = G.table([(0, 2, 3)])
    assert len(t) == core.SIG_GROUP_BYTES == 16
    for cut in (1, 15, 17):
        with pytest.raises(ValueError):
            core.sig_group_check(8, (t + t)[:cut])
    core.sig_group_check(4, t)
    core.sig_group_check(0, b"")
    core.sig_group_check(64 + 20 + 20, G.table([(0, 8, 15), (64, 1, 20), (84, 20, 20)]))
    core.sig_group_check(8, G.table([(0, 2, 3), (4, 2, 3)]))  # adjacent


# ---------------------------------------------------------------- 3. connect_block
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("m,n,signers", G.SHAPES, ids=[f"{m}of{n}-by-{''.join(map(str, s))}" for m, n, s in G.SHAPES])
def test_connect_block_groups(core, m, n, signers, kind):
    w = n - m + 1
    plain = None
    for mode in (0, 1, 2):
        blk, view, height, info = G.shape_block(m, n, signers, kind)
        spent = {(t, i): view.get(vin.prevout.hash, vin.prevout.n) for t, tx in enumerate(blk.vtx) if t
                 for i, vin in enumerate(tx.vin)}
        res, _ = G.connect(core, blk, view, height, mode, defer_multisig=True)
        assert res.ok, res.reject
        items = res.sig_items()
        # 5 multisig inputs of m * w entries, 5 P2PKH inputs of one
        assert res.num_sigs == len(items) == len(res.sig_at) == 5 * m * w + 5
        assert len(res.sig_groups) == 5 and all((gm, gn) == (m, n) for _, gm, gn in res.sig_groups)
        assert G.untable(res.sig_group_table()) == res.sig_groups
        core.sig_group_check(res.num_sigs, res.sig_group_table())
        in_group = set()
        for first, _, _ in res.sig_groups:
            t, i = res.sig_at[first]
            assert all(res.sig_at[first + k] == (t, i) for k in range(m * w))
            in_group |= set(range(first, first + m * w))
            vin = blk.vtx[t].vin[i]
            code, sigs, keys, sv = G.multisig_parts(core, vin, spent[(t, i)][1])
            assert len(sigs) == m and len(keys) == n
            for a in range(m):
                sig = sigs[m - 1 - a]  # the walk starts from the top of the stack
                msg = core.signature_hash(code, blk.vtx[t].serialize(True), i, sig[-1], spent[(t, i)][0], sv)
                for d in range(w):
                    assert items[first + a * w + d] == (keys[n - 1 - (a + d)], sig[:-1], msg)
        assert len(in_group) == 5 * m * w
        # every message, deferred or not, is the reference's
        for k, (t, i) in enumerate(res.sig_at):
            if k not in in_group:
                vin = blk.vtx[t].vin[i]
                sig = G.pushes(vin.script_sig)[0]
                assert items[k][2] == core.signature_hash(spent[(t, i)][1], blk.vtx[t].serialize(True), i, sig[-1],
                                                          spent[(t, i)][0], 0)
        if mode == 2:
            assert res.num_device_hashes > 5 * m * w  # every deferrable form, the groups' included
        if mode == 0:
            assert res.num_device_hashes == 0
        # whichever keys signed: the per-entry verdicts resolve to all valid
        raw = [int(core.secp_verify(*it)) for it in items]
        assert G.resolved(core, res) == [1] * res.num_sigs
        assert sum(raw) == 5 * m + 5  # one valid pair per signature: distinct keys
        # with the flag off nothing differs from a call without the keyword
        blk, view, height, _ = G.shape_block(m, n, signers, kind)
        off, _ = G.connect(core, blk, view, height, mode, defer_multisig=False)
        blk, view, height, _ = G.shape_block(m, n, signers, kind)
        base, _ = G.connect(core, blk, view, height, mode)
        assert off.ok and base.ok and off.sig_groups == base.sig_groups == [] and off.sig_group_table() == b""
        assert off.sig_items() == base.sig_items() and off.sig_at == base.sig_at and off.num_sigs == 5 * m + 5
        assert off.num_device_hashes == base.num_device_hashes
        if mode == 1:
            assert off.sighash_pack() == base.sighash_pack()
        if mode == 2:
            assert off.sighash_pack_var() == base.sighash_pack_var()
        if tuple(signers) != tuple(range(n - m, n)):
            # the gap this closes: signature k against key k only, and some of those pairs fail
            assert not all(core.secp_verify(*it) for it in off.sig_items())
        plain = plain or off.sig_items()
        assert off.sig_items() == plain  # the same entries in every mode


@pytest.mark.parametrize("mode", (1, 2))
def test_packers_share_a_groups_ranges(core, mode):
    """The entries of a group that sign with one hash type name the same arena ranges; the digests are
    the messages; and the arena grows by one code per group, not per pair."""
    blk, view, height, _ = make_consolidation_block(2, 6, seed=71, hash_types=(1, 0x81, 3), multisig_every=1,
                                                    multisig_mn=(2, 4), multisig_signers="cycle")
    res, _ = G.connect(core, blk, view, height, mode, defer_multisig=True)
    assert res.ok and len(res.sig_groups) == 12 and res.num_sigs == 12 * 6
    msgs = [it[2] for it in res.sig_items()]
    if mode == 1:
        arena, jobs, secp_jobs, n_dev, n_host = res.sighash_pack()
        recs = [W.JOB.unpack_from(jobs, o) for o in range(0, len(jobs), W.JOB.size)]
        digests = core.sighash_gather_model(arena, jobs)
        ranges = {r[8]: r[:8] for r in recs}
        out_index = [r[8] for r in recs]
    else:
        arena, segs, jobs, secp_jobs, n_dev, n_host = res.sighash_pack_var()
        core.sighash_var_check(len(arena), segs, jobs, res.num_sigs)
        recs = [W.VAR_JOB.unpack_from(jobs, o) for o in range(0, len(jobs), W.VAR_JOB.size)]
        digests = core.sighash_var_model(arena, segs, jobs)
        ranges = {r[2]: r[:2] for r in recs}
        out_index = [r[2] for r in recs]
    assert n_dev == len(recs) and n_dev + n_host == res.num_sigs and n_dev >= 4 * 6
    for j, k in enumerate(out_index):
        assert digests[32 * j:32 * j + 32] == msgs[k]
    shared = 0
    for first, m, n in res.sig_groups:
        ks = [k for k in range(first, first + G.pairs(m, n)) if k in ranges]
        assert len(ks) in (0, G.pairs(m, n))  # one hash type per input here
        assert len({ranges[k] for k in ks}) <= 1
        shared += len(ks)
    assert shared == n_dev
    # against the same block with the walk's pairing (2 entries per input, each with its own code)
    blk, view, height, _ = make_consolidation_block(2, 6, seed=71, hash_types=(1, 0x81, 3), multisig_every=1,
                                                    multisig_mn=(2, 4))
    off, _ = G.connect(core, blk, view, height, mode)
    off_arena = (off.sighash_pack() if mode == 1 else off.sighash_pack_var())[0]
    assert off.num_sigs == 24 and len(arena) < len(off_arena)


# ---------------------------------------------------------------- 4. fallbacks
@pytest.mark.parametrize("kind", ("p2wsh", "bare"))
def test_10_of_20_is_not_grouped(core, kind):
    results = []
    for kw in ({"defer_multisig": True}, {}):
        blk, view, height, _ = make_consolidation_block(1, 2, seed=72, multisig_every=1, multisig_mn=(10, 20),
                                                        multisig_kind=kind)
        res, _ = G.connect(core, blk, view, height, 0, **kw)
        assert res.ok, res.reject
        results.append(res)
    on, base = results
    assert on.sig_groups == [] and on.num_sigs == 20
    assert on.sig_items() == base.sig_items() and on.sig_at == base.sig_at
    assert all(core.secp_verify(*it) for it in on.sig_items())  # the last ten keys signed


def _keys(core, n, tag):
    out = []
    for k in range(n):
        sec = hashlib.sha256(f"sig-groups-{tag}-{k}".encode()).digest()
        out.append((sec, core.secp_pubkey_create(sec, True)))
    return out


def test_an_empty_signature_is_not_grouped(core):
    keys = _keys(core, 3, "empty")
    # 2-of-3 NOT: one real and one empty signature fail the opcode, which the script asks for
    spk = b"\x52" + b"".join(core.script_push_data(p) for _, p in keys) + b"\x53\xae\x91"
    results = []
    for kw in ({"defer_multisig": True}, {}):
        blk, view, height = G.one_input_block(
            core, spk, lambda sign: b"\x00\x00" + core.script_push_data(sign(keys[2][0])))
        res, _ = G.connect(core, blk, view, height, 0, **kw)
        assert res.ok, res.reject
        results.append(res)
    on, base = results
    assert on.sig_groups == [] and on.num_sigs == 1 and on.sig_items() == base.sig_items()
    assert on.sig_items()[0][0] == keys[2][1]


def test_a_key_with_a_bad_header_is_not_grouped(core):
    keys = _keys(core, 3, "header")
    odd = b"\x05" + keys[0][1][1:]  # passes the block's encoding rules, fails CPubKey::IsValid
    spk = b"\x52" + b"".join(core.script_push_data(p) for p in (odd, keys[1][1], keys[2][1])) + b"\x53\xae"
    results = []
    for kw in ({"defer_multisig": True}, {}):
        blk, view, height = G.one_input_block(
            core, spk, lambda sign: b"\x00" + core.script_push_data(sign(keys[1][0])) + core.script_push_data(sign(keys[2][0])))
        res, _ = G.connect(core, blk, view, height, 0, **kw)
        assert res.ok, res.reject
        results.append(res)
    on, base = results
    assert on.sig_groups == [] and on.num_sigs == 2 and on.sig_items() == base.sig_items()
    # the same script with a sound key is grouped: the fallback is the key's doing
    spk = b"\x52" + b"".join(core.script_push_data(p) for _, p in keys) + b"\x53\xae"
    blk, view, height = G.one_input_block(
        core, spk, lambda sign: b"\x00" + core.script_push_data(sign(keys[1][0])) + core.script_push_data(sign(keys[2][0])))
    res, _ = G.connect(core, blk, view, height, 0, defer_multisig=True)
    assert res.ok and res.sig_groups == [(0, 2, 3)] and res.num_sigs == 4


def test_defer_multisig_needs_defer_sigs(core):
    blk, view, height, _ = G.shape_block(2, 3, (0, 1), "p2sh")
    res, _ = core.connect_block(blk, height, view, True, False, defer_multisig=True)
    assert res.ok and res.num_sigs == 0 and res.sig_groups == []  # verified on the host, any signers


# ---------------------------------------------------------------- 5. failures
def _connect_state(core, blk, view, height, multisig):
    """What ChainState does with a block's deferred signatures, on the host: resolved verdicts, then
    verify_input_host for the inputs of the entries that are not valid. -> (rechecked inputs, reject)"""
    res, undo = G.connect(core, blk, view, height, 0, defer_multisig=multisig)
    assert res.ok, res.reject
    verdicts = G.resolved(core, res)
    inputs = sorted({res.sig_at[k] for k, v in enumerate(verdicts) if v != 1})
    reject = None
    for t, i in inputs:
        value, spk, _, _ = core.block_undo_coin(undo, t, i)
        ok, err = core.verify_input_host(blk, t, i, value, spk, core.BLOCK_SCRIPT_VERIFY_FLAGS)
        if not ok:
            reject = reject or f"mandatory-script-verify-flag-failed ({err})"
    return res, verdicts, inputs, reject


@pytest.mark.parametrize("what", ("corrupted", "reversed"))
def test_a_failing_group_is_all_zero_and_rechecked(core, what):
    # 6 inputs of 2-of-3 P2SH, every signer subset; input 4 of transaction 1 is broken
    blk, view, height, _ = make_consolidation_block(1, 6, seed=73, multisig_every=1, multisig_signers="cycle")
    if what == "corrupted":
        G.corrupt_multisig_signature(core, blk, 1, 4)
    else:
        G.reverse_signatures(core, blk, 1, 4)
    res, verdicts, inputs, reject = _connect_state(core, blk, view, height, True)
    assert res.sig_groups == [(4 * k, 2, 3) for k in range(6)]
    assert verdicts == [1] * 16 + [0] * 4 + [1] * 4
    assert inputs == [(1, 4)] and reject.startswith("mandatory-script-verify-flag-failed (")
    # the host-only connect says the same
    blk, view, height, _ = make_consolidation_block(1, 6, seed=73, multisig_every=1, multisig_signers="cycle")
    (G.corrupt_multisig_signature if what == "corrupted" else G.reverse_signatures)(core, blk, 1, 4)
    host, _ = core.connect_block(blk, height, view, True, False)
    assert not host.ok and host.reject == reject


# ---------------------------------------------------------------- 6. the window's table
def _five(core, mode):
    results = []
    for b, (n_txs, n_in) in enumerate(W.FIVE):
        blk, view, height, _ = make_consolidation_block(
            n_txs, n_in, seed=80 + b, hash_types=W.HASH_TYPES, witness_every=4, multisig_every=3 if b != 1 else 0,
            multisig_signers="cycle", multisig_kind=G.KINDS[b % 3])
        res, _ = G.connect(core, blk, view, height, mode, defer_multisig=True)
        assert res.ok, res.reject
        results.append(res)
    return results


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_window_groups_are_the_blocks_tables_rebased(core, mode):
    results = _five(core, mode)
    assert [bool(r.sig_groups) for r in results] == [False, False, False, True, True]
    pack = core.sig_window_pack(results)
    sig_begin = pack[5]
    assert sig_begin == [0] + [sum(r.num_sigs for r in results[:b + 1]) for b in range(5)]
    want = [(sig_begin[b] + first, m, n) for b, r in enumerate(results) for first, m, n in r.sig_groups]
    got = core.sig_window_groups(results)
    assert G.untable(got) == want and len(want) == 10 + 3  # every third input that is not a fourth
    core.sig_group_check(sig_begin[-1], got)
    raw = [[int(core.secp_verify(*it)) for it in r.sig_items()] for r in results]
    per_block = [core.sig_group_resolve_model(v, r.sig_group_table()) for v, r in zip(raw, results)]
    assert core.sig_group_resolve_model(sum(raw, []), got) == sum(per_block, [])
    assert sum(per_block, []) == [1] * sig_begin[-1] and 0 in sum(raw, [])
    assert core.sig_window_groups([]) == b"" and core.sig_window_groups(results[:3]) == b""
    # the packed window hashes what the blocks hash
    if mode:
        arena, segs, jobs = pack[1], pack[2], pack[3]
        digests = core.sighash_var_model(arena, segs, jobs) if mode == 2 else core.sighash_gather_model(arena, jobs)
        st = W.VAR_JOB if mode == 2 else W.JOB
        msgs = [it[2] for r in results for it in r.sig_items()]
        for j, o in enumerate(range(0, len(jobs), st.size)):
            k = st.unpack_from(jobs, o)[2 if mode == 2 else 8]
            assert digests[32 * j:32 * j + 32] == msgs[k]


# ---------------------------------------------------------------- 7. ChainState
@pytest.fixture(scope="module")
def chains(core):
    base, chain, first_try = G.build_chain(core)
    params = W.new_state().params
    return {"base": base, "good": chain, "first_try": first_try, "params": params,
            "bad2": W.variant(core, params, chain, {2: lambda c, b: G.corrupt_multisig_signature(c, b, 1, 3)}),
            "rev1": W.variant(core, params, chain, {1: lambda c, b: G.reverse_signatures(c, b, 1, 0)})}


def _node(core, chains, multisig, window, sighash_mode=0, calls=None):
    st = W.new_state()
    W.feed(st, chains["base"])
    assert st.height() == W.N_BASE and st.gpu_multisig == 0
    st.gpu_signatures, st.gpu_sig_window, st.gpu_multisig = "on", window, multisig
    st.gpu_sighash, st.gpu_sighash_forms = sighash_mode >= 1, "all" if sighash_mode == 2 else "legacy-all"
    st.sig_window_verifier = G.group_verifier(core, calls)
    return st


@pytest.mark.parametrize("sighash_mode", (0, 2))
def test_chain_state_connects_every_signer_subset_without_a_recheck(core, chains, sighash_mode):
    host = W.new_state()
    W.feed(host, chains["base"])
    assert all(s.ok for s in W.feed(host, chains["good"], one_walk=True))
    assert host.height() == W.N_BASE + G.N_CHAIN and host.sig_stats["host_rechecks"] == 0
    n_inputs = G.N_OUT
    first_try = sum(chains["first_try"])
    assert 0 < first_try < n_inputs
    calls_on, calls_off = [], []
    on = _node(core, chains, 1, 1000, sighash_mode, calls_on)
    assert all(s.ok for s in W.feed(on, chains["good"], one_walk=True))
    off = _node(core, chains, 0, 1000, sighash_mode, calls_off)
    assert all(s.ok for s in W.feed(off, chains["good"], one_walk=True))
    assert on.sig_stats["host_rechecks"] == 0
    assert off.sig_stats["host_rechecks"] == n_inputs - first_try
    for st in (on, off):
        assert st.height() == host.height() and st.chain.tip().hash == host.chain.tip().hash
        assert st.coins.best_block == host.coins.best_block and st.coins.stats() == host.coins.stats()
    # one window each; with the flag every input is a group, without it none is
    assert [len(c) for c in calls_on] == [G.N_CHAIN] and all(g == G.PER_BLOCK for _, g in calls_on[0])
    assert all(g == 0 for _, g in calls_off[0])
    entries = sum(n for n, _ in calls_on[0])
    assert on.sig_stats["gpu_multisig_groups"] == n_inputs and on.sig_stats["gpu_multisig_entries"] == entries
    assert on.sig_stats["gpu_sigs"] == entries > off.sig_stats["gpu_sigs"]
    assert off.sig_stats["gpu_multisig_groups"] == off.sig_stats["gpu_multisig_entries"] == 0
    assert on.sig_stats["gpu_sighashes"] == (entries if sighash_mode == 2 else 0)


def test_chain_state_small_batch_branch_resolves_groups(core):
    """-gpusigs=auto with a window below the batch minimum: the host answers per entry and the model
    resolves the groups, so no input is rechecked there either; no counter moves, as before."""
    st = W.new_state()
    st.gpu_signatures, st.gpu_sig_window, st.gpu_multisig = "auto", 1000, 1
    blk, view, height, _ = make_consolidation_block(1, 3, seed=74, multisig_every=1, multisig_signers="cycle")
    res, undo = G.connect(core, blk, view, height, 0, defer_multisig=True)
    assert res.ok and len(res.sig_groups) == 3 and res.num_sigs == 12
    assert [bool(core.secp_verify(*it)) for it in res.sig_items()].count(False) == 6
    before = dict(st.sig_stats)
    assert st._verify_window([(blk, None, res, undo)]) == [[True] * 12]
    assert st.sig_stats == before


@pytest.mark.parametrize("which,bad_block", (("bad2", 2), ("rev1", 1)))
@pytest.mark.parametrize("window", (1, 1000))
def test_chain_state_rejects_as_the_host_does(core, chains, which, bad_block, window):
    host = W.new_state()
    W.feed(host, chains["base"])
    host_states = W.feed(host, chains[which][:bad_block])
    assert not host_states[-1].ok and host.height() == W.N_BASE + bad_block - 1
    on = _node(core, chains, 1, window)  # a window of one signature closes at every block
    states = W.feed(on, chains[which][:bad_block], one_walk=window > 1)
    assert not states[-1].ok
    assert (states[-1].reject, states[-1].dos) == (host_states[-1].reject, host_states[-1].dos)
    assert states[-1].reject.startswith("mandatory-script-verify-flag-failed (")
    assert on.height() == host.height() and on.coins.stats() == host.coins.stats()
    assert on.sig_stats["host_rechecks"] == 1 and on.sig_stats["window_rollbacks"] == 1


def test_gpumultisig_flag(core, node_factory):
    st = W.new_state()
    assert st.gpu_multisig == 0
    assert {"gpu_multisig_groups", "gpu_multisig_entries"} <= set(st.sig_stats)
    assert st.sig_stats["gpu_multisig_groups"] == st.sig_stats["gpu_multisig_entries"] == 0
    # a node without the GPU batch has nothing for the flag to act on and connects on the host
    node, _ = node_factory(("-gpusigs=off", "-gpumultisig=1", "-maxsigcachesize=0"))
    assert node.state.gpu_multisig == 1
    c = client(node)
    w = c.getnewaddress()
    c.generatetoaddress(101, w)
    c.sendtoaddress(c.getnewaddress(), 1.0)
    c.generatetoaddress(1, w)
    assert c.getblockcount() == 102
    info = c.getgpuinfo()[0]["block_sigs"]
    assert info == node.state.sig_stats and info["gpu_multisig_groups"] == info["gpu_multisig_entries"] == 0


# ---------------------------------------------------------------- 8. the default fixtures
def _digest(blk, view):
    return hashlib.sha256(b"".join(tx.serialize(True) for tx in blk.vtx)).hexdigest(), view.stats()[3].hex()


@pytest.mark.parametrize("kw,block_hash,utxo_hash", [
    (dict(n_txs=3, inputs_per_tx=4, seed=1, multisig_every=2),
     "04a633f6cb70b4ae0106d21e76e8a822a3ecdfb3e2cc1d829ce6d5fa80833676",
     "38f41be64fb786df5638cb20201699a9bf66e0d93de4b9c86522d6100d37e7c8"),
    (dict(n_txs=2, inputs_per_tx=(2, 6), seed=7, hash_types=(1, 2, 3, 0x81), witness_every=3, multisig_every=2),
     "ef1843cfd23b1c6521c010dcf8159336c8259ce17b8922120be361568d07bd19",
     "a53903cf480a6239142b50619439e1d02aa15d108563af01b1928d520948cfb0"),
    (dict(n_txs=2, inputs_per_tx=5, seed=3, multisig_every=1, bad_at=3),
     "788bce15c1084ea5f6f321450fe17b582ab69dc119bbe8eea8c740eb72368d59",
     "c6953d4fd451c2a58c2becd3017d27da10cf9a80df0c66720218a5039fcb98d9"),
], ids=["2of3-every-2", "mixed-forms", "bad-at-3"])
def test_default_fixtures_are_the_parents(core, kw, block_hash, utxo_hash):
    """SHA-256 over the block's transactions and the UTXO hash of its view, computed on the commit
    before -gpumultisig: the new keyword arguments change nothing by default."""
    blk, view, _, info = make_consolidation_block(**kw)
    assert _digest(blk, view) == (block_hash, utxo_hash)
    if kw.get("bad_at") is not None:
        assert info["bad_sig"] == 3 * 2 + 1


def test_kernel_keeps_to_registers(tmp_path):
    """sig_group_resolve is one lane per group in registers: the compiler's resource report for the
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
                        os.path.join(kdir, "sig_group.hip"), "-o", str(tmp_path / "sig_group.hsaco")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rep = r.stderr[r.stderr.index("Function Name: sig_group_resolve"):]
    usage = {k.strip(): v for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\w+) \[-Rpass", rep)}
    assert usage["ScratchSize [bytes/lane]"] == "0" and usage["Dynamic Stack"] == "False"
    assert usage["VGPRs Spill"] == "0" and usage["SGPRs Spill"] == "0" and usage["LDS Size [bytes/block]"] == "0"
    assert int(usage["VGPRs"]) <= 32 and usage["Occupancy [waves/SIMD]"] == "8"
