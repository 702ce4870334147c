"""Legacy signature hashes on a real MI355X (hip/kernels/sighash.hip, ops/sighash.py): the kernel
against its host model at the padding, compact-size and splice edges, the z limbs and kind it
writes into the packed secp jobs, a mixed block through gather + batch ECDSA, and a node that
connects its blocks with -gpusighash=1."""
import struct

import pytest

import sighash_util as U
from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block
from test_node_rpc import client
from test_p2p import _node

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(core):
    return U.edge_cases(core)


def test_digests_match_the_model(gpu, core, cases):
    from nodexa_chain_core_amd.ops import sighash

    arena, jobs = U.pack_cases(core, cases)
    want = core.sighash_gather_model(arena, jobs)
    got = sighash.digests(arena, jobs).tobytes()
    n = len(cases)
    assert n >= 590 and len(got) == 32 * n  # more than two workgroups, the last one partly filled
    bad = [k for k in range(n) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
    assert not bad, f"{len(bad)} of {n} differ, first: case {bad[0]} {cases[bad[0]][1:]}"
    assert want == U.host_hashes(core, cases)
    # an arena that starts and ends off a dword boundary on the device: shift every offset by one
    shifted = b"".join(U.JOB.pack(*(o + 1 for o in r[:4]), *r[4:]) for r in U.JOB.iter_unpack(jobs))
    assert sighash.digests(b"\xa5" + arena, shifted).tobytes() == want
    # a malformed table never reaches the device
    rec = list(U.JOB.unpack_from(jobs, 0))
    rec[2] = len(arena)
    with pytest.raises(ValueError):
        sighash.digests(arena, U.JOB.pack(*rec))


FIXTURE = dict(n_txs=12, inputs_per_tx=(1, 40), seed=11, hash_types=(1, 0x81, 2, 3, 0), witness_every=4,
               multisig_every=5)


def _connect(core, **kw):
    blk, view, height, info = make_consolidation_block(**FIXTURE, **kw)
    res, _ = core.connect_block(blk, height, view, True, True, None, 0, core.BLOCK_SCRIPT_VERIFY_FLAGS, 8,
                                defer_sighash=True)
    assert res.ok and res.num_sigs == info["sigs"]
    return res, info


def test_gather_fills_the_secp_jobs(gpu, core):
    from nodexa_chain_core_amd.ops import sighash

    res, info = _connect(core)
    arena, jobs, secp_jobs, n_dev, n_host = res.sighash_pack()
    assert (n_dev, n_host) == (info["device_sigs"], info["host_sigs"]) and n_dev > 64 and n_host > 0
    # a job array larger than the job count: the tail is uploaded INVALID and must stay so
    sz = core.SECP_JOB_BYTES
    invalid = bytearray(sz)
    struct.pack_into("<I", invalid, 5 * 32, core.SECP_KIND_INVALID)
    tail = bytes(invalid) * 37
    got = sighash.gather_into_secp(arena, jobs, secp_jobs + tail)
    assert got[:res.num_sigs * sz] == core.secp_pack_jobs(res.sig_items())
    assert got[res.num_sigs * sz:] == tail


def test_block_verdicts_match_the_host(gpu, core):
    from nodexa_chain_core_amd.ops import sighash

    # input 2 signs with hash type 2 (host-hashed), input 4 is the first multisig: corrupt input 5,
    # a P2PKH input with hash type 1, hashed on the device
    res, info = _connect(core, bad_at=5)
    assert res.num_device_hashes == info["device_sigs"]
    items = res.sig_items()
    got = sighash.verify_block_sigs(res)
    want = [core.secp_verify(*it) for it in items]
    assert got == want
    assert [k for k, v in enumerate(got) if not v] == [info["bad_sig"]]
    device_rows = {r[8] for r in U.JOB.iter_unpack(res.sighash_pack()[1])}
    assert info["bad_sig"] in device_rows and len(device_rows) == info["device_sigs"]


def _sync(ca, cb):
    for h in range(cb.getblockcount() + 1, ca.getblockcount() + 1):
        assert cb.submitblock(ca.getblock(ca.getblockhash(h), 0)) is None


def test_node_connects_blocks_with_gpu_sighash(gpu, core, tmp_path):
    a = _node(core, tmp_path, "a", ["-gpusigs=on", "-gpusighash=1", "-maxsigcachesize=0"])
    b = _node(core, tmp_path, "b", ["-gpusigs=on", "-gpusighash=0", "-maxsigcachesize=0"])
    try:
        ca, cb = client(a), client(b)
        st = a.state
        assert st.gpu_sighash is True and b.state.gpu_sighash is False
        w = ca.getnewaddress()
        ca.generatetoaddress(101, w)
        # split the mature coinbase into 24 outputs, then spend all 24 in one transaction
        split = ca.sendmany("", {ca.getnewaddress(): 5.0 for _ in range(24)})
        ca.generatetoaddress(1, w)
        ext = core.base58check_encode(bytes([42]) + bytes(range(1, 21)))
        ins = [{"txid": split, "vout": v["n"]} for v in ca.getrawtransaction(split, True)["vout"] if v["value"] == 5.0]
        assert len(ins) == 24
        raw = ca.createrawtransaction(ins, {ext: 119.9})
        ca.sendrawtransaction(ca.signrawtransaction(raw)["hex"])
        before = dict(st.sig_stats)
        ca.generatetoaddress(1, w)
        assert ca.getrawmempool() == []
        assert st.sig_stats["gpu_sighashes"] - before["gpu_sighashes"] == 24
        assert st.sig_stats["gpu_sigs"] - before["gpu_sigs"] == 24
        assert st.sig_stats["host_rechecks"] == before["host_rechecks"]
        assert ca.getgpuinfo()[0]["block_sigs"] == st.sig_stats
        # the twin validates the same chain with the hashes on the host: the same UTXO set
        _sync(ca, cb)
        assert b.state.sig_stats["gpu_sighashes"] == 0 and b.state.sig_stats["gpu_sigs"] >= 24
        assert cb.gettxoutsetinfo()["hash_serialized_2"] == ca.gettxoutsetinfo()["hash_serialized_2"]
        assert cb.getbestblockhash() == ca.getbestblockhash()
        # a block with one bad signature: the batch flags it, the host confirms, the block is refused
        u = max((x for x in ca.listunspent() if x["txid"] == split), key=lambda x: x["amount"])  # the split's change
        raw = ca.createrawtransaction([{"txid": u["txid"], "vout": u["vout"]}], {ext: 1.0})
        tx = core.Transaction.deserialize(bytes.fromhex(ca.signrawtransaction(raw)["hex"]))
        vin = list(tx.vin)
        sig = bytearray(vin[0].script_sig)
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
