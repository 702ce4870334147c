"""Every form of signature hash on a real MI355X (hip/kernels/sighash_var.hip, ops/sighash.py):
sighash_gather_var against its host model on the seeded edge set (aligned, misaligned, shuffled),
the z limbs and kind it writes into the packed secp jobs of a mixed block, that block through
gather + batch ECDSA, and a node that connects its blocks with -gpusighash=2."""
import random
import struct

import pytest

import sighash_forms_util as F
from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block
from test_node_rpc import client
from test_p2p import _node

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(core):
    return F.edge_cases(core)


@pytest.fixture(scope="module")
def want(core, cases):
    """The model's digests of the Python-packed edge set (and the tables), computed once."""
    arena, segs, jobs, job_case = F.pack_cases(cases)
    model = core.sighash_var_model(arena, segs, jobs)
    assert model == F.expected_digests(cases, job_case)
    return arena, segs, jobs, job_case, model


def _differ(got, model, cases, job_case):
    bad = [k for k in range(len(job_case)) if got[32 * k:32 * k + 32] != model[32 * k:32 * k + 32]]
    return f"{len(bad)} of {len(job_case)} differ, first: job {bad[0]} {job_case[bad[0]] is not None and cases[job_case[bad[0]]][1:]}" if bad else ""


def test_digests_var_match_the_model(gpu, core, cases, want):
    from nodexa_chain_core_amd.ops import sighash

    arena, segs, jobs, job_case, model = want
    n = len(job_case)
    assert n > 3 * 256 and n % 256  # more than three workgroups, the last one partly filled
    got = sighash.digests_var(arena, segs, jobs).tobytes()
    assert len(got) == 32 * n and not _differ(got, model, cases, job_case)


def test_digests_var_on_a_misaligned_arena(gpu, core, cases, want):
    from nodexa_chain_core_amd.ops import sighash

    _, _, _, job_case, model = want
    arena, segs, jobs, jc = F.pack_cases(cases, shift=1)  # every offset moves by one
    assert jc == job_case and len(arena) % 4
    got = sighash.digests_var(arena, segs, jobs).tobytes()
    assert not _differ(got, model, cases, job_case)


def test_digests_var_with_the_jobs_shuffled(gpu, core, cases, want):
    """Forms mixed inside each wave, out_index a permutation: row out_index holds job k's digest."""
    from nodexa_chain_core_amd.ops import sighash

    arena, segs, jobs, job_case, model = want
    n = len(job_case)
    order = list(range(n))
    random.Random(13).shuffle(order)
    recs = [F.JOB.unpack_from(jobs, k * F.JOB.size) for k in range(n)]
    shuffled = b"".join(F.JOB.pack(*recs[k]) for k in order)  # job k still writes row k, from another lane
    got = sighash.digests_var(arena, segs, shuffled).tobytes()
    assert not _differ(got, model, cases, job_case)
    # and a permuted output: lane j (job j) writes row perm[j]
    perm = order
    permuted = b"".join(F.JOB.pack(r[0], r[1], perm[k], r[3]) for k, r in enumerate(recs))
    got = sighash.digests_var(arena, segs, permuted).tobytes()
    assert all(got[32 * perm[k]:32 * perm[k] + 32] == model[32 * k:32 * k + 32] for k in range(n))


def test_malformed_tables_never_reach_the_device(gpu, core, want):
    from nodexa_chain_core_amd.ops import sighash

    arena, segs, jobs, _, _ = want
    first = F.JOB.unpack_from(jobs, 0)
    with pytest.raises(ValueError):
        sighash.digests_var(arena, F.SEG.pack(len(arena) - 3, 4) + segs[F.SEG.size:], jobs)  # a segment one byte out
    with pytest.raises(ValueError):
        sighash.digests_var(arena, segs, F.JOB.pack(len(segs) // F.SEG.size - 1, 2, 0, first[3]))  # past the table
    with pytest.raises(ValueError):
        sighash.digests_var(arena, segs, F.JOB.pack(0, 9, 0, first[3]))  # more than 8 segments
    with pytest.raises(ValueError):
        sighash.digests_var(arena, segs, F.JOB.pack(first[0], first[1], 1, first[3]))  # output 1 of 1


FIXTURE = dict(n_txs=12, inputs_per_tx=(1, 40), seed=11, hash_types=(1, 0x81, 2, 3, 0x82, 0x83, 0), witness_every=4,
               multisig_every=5)


def _connect(core, **kw):
    blk, view, height, info = make_consolidation_block(**FIXTURE, **kw)
    res, _ = core.connect_block(blk, height, view, True, True, None, 0, core.BLOCK_SCRIPT_VERIFY_FLAGS, 8,
                                defer_sighash=True, defer_all_forms=True)
    assert res.ok and res.num_sigs == info["sigs"] and res.all_forms
    return res, info


def test_gather_var_fills_the_secp_jobs(gpu, core):
    from nodexa_chain_core_amd.ops import sighash

    res, info = _connect(core)
    arena, segs, jobs, secp_jobs, n_dev, n_host = res.sighash_pack_var()
    assert n_dev + n_host == info["sigs"] and res.num_device_v0 > 16 and res.num_device_partial > 64
    # a job array larger than the job count: the tail is uploaded INVALID and must stay so
    sz = core.SECP_JOB_BYTES
    invalid = bytearray(sz)
    struct.pack_into("<I", invalid, 5 * 32, core.SECP_KIND_INVALID)
    tail = bytes(invalid) * 37
    got = sighash.gather_var_into_secp(arena, segs, jobs, secp_jobs + tail)
    assert got[:res.num_sigs * sz] == core.secp_pack_jobs(res.sig_items())
    assert got[res.num_sigs * sz:] == tail


# inputs of the fixture by what signs them: input g has hash type FIXTURE["hash_types"][g % 7], is
# P2WPKH when 4 divides g + 1 and P2SH multisig when 5 divides g + 1
@pytest.mark.parametrize("bad_at,sv,form", [(96, 0, "single|acp"), (7, 1, "all"), (2, 0, "none")])
def test_block_verdicts_match_the_host(gpu, core, bad_at, sv, form):
    from nodexa_chain_core_amd.ops import sighash

    ht = FIXTURE["hash_types"][bad_at % 7]
    assert ((bad_at + 1) % 4 == 0) == bool(sv) and (sv or (bad_at + 1) % 5) and core.sighash_form(sv, ht) == form
    res, info = _connect(core, bad_at=bad_at)
    items = res.sig_items()
    got = sighash.verify_block_sigs(res)
    want = [core.secp_verify(*it) for it in items]
    assert got == want
    assert [k for k, v in enumerate(got) if not v] == [info["bad_sig"]]
    jobs = res.sighash_pack_var()[2]
    device_rows = {F.JOB.unpack_from(jobs, k * F.JOB.size)[2] for k in range(len(jobs) // F.JOB.size)}
    assert info["bad_sig"] in device_rows  # its hash came from the device


def _sync(ca, cb):
    for h in range(cb.getblockcount() + 1, ca.getblockcount() + 1):
        assert cb.submitblock(ca.getblock(ca.getblockhash(h), 0)) is None


def test_node_connects_blocks_with_every_form_on_the_gpu(gpu, core, tmp_path):
    a = _node(core, tmp_path, "a", ["-gpusigs=on", "-gpusighash=2", "-maxsigcachesize=0"])
    b = _node(core, tmp_path, "b", ["-gpusigs=on", "-gpusighash=0", "-maxsigcachesize=0"])
    try:
        ca, cb = client(a), client(b)
        st = a.state
        assert st.gpu_sighash is True and st.gpu_sighash_forms == "all"
        assert b.state.gpu_sighash is False and b.state.gpu_sighash_forms == "legacy-all"
        w = ca.getnewaddress()
        ca.generatetoaddress(101, w)
        # split the mature coinbase: 24 outputs of 2.0, 24 of 3.0, and one to a witness address
        wit = ca.addwitnessaddress(ca.getnewaddress())
        pay = {ca.getnewaddress(): 2.0 for _ in range(24)}
        pay.update({ca.getnewaddress(): 3.0 for _ in range(24)})
        pay[wit] = 4.0
        split = ca.sendmany("", pay)
        ca.generatetoaddress(1, w)
        ext = core.base58check_encode(bytes([42]) + bytes(range(1, 21)))
        vout = ca.getrawtransaction(split, True)["vout"]
        by_value = lambda x: [{"txid": split, "vout": v["n"]} for v in vout if v["value"] == x]  # noqa: E731
        twos, threes, fours = by_value(2.0), by_value(3.0), by_value(4.0)
        assert (len(twos), len(threes), len(fours)) == (24, 24, 1)
        # 24 inputs signed NONE; 24 inputs into 24 outputs signed SINGLE|ANYONECANPAY; one P2SH-P2WPKH spend
        raw = ca.createrawtransaction(twos, {ext: 47.9})
        ca.sendrawtransaction(ca.signrawtransaction(raw, [], [], "NONE")["hex"])
        outs = {core.base58check_encode(bytes([42]) + bytes([k]) * 20): 2.99 for k in range(1, 25)}
        raw = ca.createrawtransaction(threes, outs)
        ca.sendrawtransaction(ca.signrawtransaction(raw, [], [], "SINGLE|ANYONECANPAY")["hex"])
        raw = ca.createrawtransaction(fours, {ext: 3.99})
        signed = core.Transaction.deserialize(bytes.fromhex(ca.signrawtransaction(raw)["hex"]))
        assert signed.vin[0].witness  # a witness-v0 signature
        ca.sendrawtransaction(signed.serialize(True).hex())
        assert len(ca.getrawmempool()) == 3
        before = dict(st.sig_stats)
        ca.generatetoaddress(1, w)
        assert ca.getrawmempool() == []
        assert st.sig_stats["gpu_sighashes_partial"] - before["gpu_sighashes_partial"] == 48
        assert st.sig_stats["gpu_sighashes_v0"] - before["gpu_sighashes_v0"] >= 1
        assert st.sig_stats["gpu_sighashes"] - before["gpu_sighashes"] == 49
        assert st.sig_stats["gpu_sigs"] - before["gpu_sigs"] == 49
        assert st.sig_stats["host_sighashes"] == before["host_sighashes"]
        assert st.sig_stats["host_rechecks"] == before["host_rechecks"]
        assert ca.getgpuinfo()[0]["block_sigs"] == st.sig_stats
        # the twin validates the same chain with the hashes on the host: the same UTXO set
        _sync(ca, cb)
        assert b.state.sig_stats["gpu_sighashes"] == 0 and b.state.sig_stats["gpu_sigs"] >= 49
        assert cb.gettxoutsetinfo()["hash_serialized_2"] == ca.gettxoutsetinfo()["hash_serialized_2"]
        assert cb.getbestblockhash() == ca.getbestblockhash()
        # a block with one bad NONE signature: the batch flags it, the host confirms, the block is refused
        u = max((x for x in ca.listunspent() if x["txid"] == split), key=lambda x: x["amount"])  # the split's change
        raw = ca.createrawtransaction([{"txid": u["txid"], "vout": u["vout"]}], {ext: 1.0})
        tx = core.Transaction.deserialize(bytes.fromhex(ca.signrawtransaction(raw, [], [], "NONE")["hex"]))
        vin = list(tx.vin)
        sig = bytearray(vin[0].script_sig)
        assert sig[sig[0]] == 0x02  # the signature push ends with the hash type NONE
        sig[10] ^= 1
        vin[0].script_sig = bytes(sig)
        tx.vin = vin
        st.add_to_mempool(tx, 1_000_000)
        height = ca.getblockcount()
        rechecks = st.sig_stats["host_rechecks"]
        with pytest.raises(RuntimeError, match="mandatory-script-verify-flag-failed"):
            a.miner.generate(a.mining_script, 1)
        assert ca.getblockcount() == height
        assert st.sig_stats["host_rechecks"] == rechecks + 1
    finally:
        a.stop()
        b.stop()
