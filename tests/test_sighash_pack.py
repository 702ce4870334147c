"""The gathered legacy signature hash on the host (csrc/chain/sighash.cpp, interpreter.cpp): the
kernel's model against signature_hash at the edges and on the reference's sighash.json, the block
packer behind connect_block(defer_sighash=True), the job-table check and the node flag."""
import json
import os
import struct

import pytest

import sighash_util as U
from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block
from test_node_rpc import client, node_factory  # noqa: F401 — shared fixture

REF_VECTORS = "/root/reference/src/test/data/sighash.json"


@pytest.fixture(scope="module")
def cases(core):
    return U.edge_cases(core)


def test_edge_cases_cover_the_edges(core, cases):
    """The generator reaches what it claims to: the test below is only as good as this."""
    lens = [U.preimage_len(core, raw, code) for raw, _, code, _ in cases]
    assert {n % 64 for n in lens} >= set(U.RESIDUES)
    assert {len(code) for _, _, code, _ in cases} >= set(U.CODE_LENS)
    vins = {len(core.sighash_template(raw)[1]) for raw, _, _, _ in cases}
    assert vins >= {1, 2, 252, 253}
    for raw, i, _, _ in cases:
        n = len(core.sighash_template(raw)[1])
        if n in (252, 253):
            assert 0 <= i < n
    assert {(len(core.sighash_template(raw)[1]), i) for raw, i, _, _ in cases} >= {(252, 0), (252, 251), (253, 0), (253, 252)}
    assert {ht for _, _, _, ht in cases} >= {0x01, 0x00, 0x04, 0x21, 0x7c}
    assert all(core.sighash_all_form(0, ht) for _, _, _, ht in cases)
    assert 590 <= len(cases) <= 640


def test_model_matches_signature_hash(core, cases):
    arena, jobs = U.pack_cases(core, cases)
    got = core.sighash_gather_model(arena, jobs)
    want = U.host_hashes(core, cases)
    assert len(got) == 32 * len(cases)
    bad = [k for k in range(len(cases)) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
    assert not bad, f"{len(bad)} of {len(cases)} differ, first: {cases[bad[0]][1:]}"


def test_template_is_the_blanked_serialisation(core, cases):
    raw = cases[-1][0]  # 253 inputs: the vin count takes three bytes
    t, offs = core.sighash_template(raw)
    assert t[4:7] == b"\xfd\xfd\x00" and len(offs) == 253
    assert offs == [7 + 41 * i + 36 for i in range(253)]
    assert all(t[o] == 0 for o in offs)
    # codeseparators removed with the reference's length rule; a truncated push stops the copy
    assert core.sighash_script_code(b"\x51\xab\x52") == b"\x02\x51\x52"
    # (GetOp has read the opcode and the length byte when it finds the data short: the copy ends there)
    assert core.sighash_script_code(b"\x76\xab\x4c\x05\x01\x02") == b"\x05\x76\x4c\x05"
    assert core.sighash_script_code(bytes(253)) == b"\xfd\xfd\x00" + bytes(253)


def test_eligibility_rule(core):
    for ht, want in [(0x01, True), (0x00, True), (0x04, True), (0x21, True), (0x7c, True), (0x02, False),
                     (0x03, False), (0x81, False), (0x80, False), (0x22, False), (0x63, False), (0x1ff01, True),
                     (-1, False), (-0x7fffffff, True)]:
        assert core.sighash_all_form(0, ht) is want, hex(ht)
        assert core.sighash_all_form(1, ht) is False  # BIP143 stays on the host


def test_reference_sighash_vectors(core):
    if not os.path.exists(REF_VECTORS):
        pytest.skip("reference vector file sighash.json not present")
    with open(REF_VECTORS) as f:
        vectors = [t for t in json.load(f) if not (len(t) == 1 and isinstance(t[0], str))]
    assert len(vectors) == 500
    eligible = []
    for raw_tx, script, n_in, hash_type, expect in vectors:
        if core.sighash_all_form(0, hash_type):
            eligible.append(((bytes.fromhex(raw_tx), n_in, bytes.fromhex(script), hash_type), expect))
    assert len(eligible) == 253
    # the vectors carry their scripts: hash the legacy form of each transaction, as signature_hash does
    cases = [c for c, _ in eligible]
    arena, jobs = U.pack_cases(core, cases)
    got = core.sighash_gather_model(arena, jobs)
    bad = [k for k, (_, expect) in enumerate(eligible) if got[32 * k:32 * k + 32][::-1].hex() != expect]
    assert not bad, f"{len(bad)} of 253 differ, first: {eligible[bad[0]]}"


FIXTURE = dict(n_txs=6, inputs_per_tx=(1, 9), seed=5, hash_types=(1, 0x81, 2, 3, 0), witness_every=4, multisig_every=5)


def test_connect_block_defers_the_hashes(core):
    blk, view, height, info = make_consolidation_block(**FIXTURE)
    ref, _ = core.connect_block(blk, height, view, True, True)
    blk, view, height, info = make_consolidation_block(**FIXTURE)
    res, _ = core.connect_block(blk, height, view, True, True, defer_sighash=True)
    assert ref.ok and res.ok
    assert res.num_sigs == info["sigs"] and info["device_sigs"] > 0 and info["host_sigs"] > 0
    items = res.sig_items()
    assert items == ref.sig_items() and res.sig_at == ref.sig_at
    assert all(core.secp_verify(*it) for it in items)
    arena, jobs, secp_jobs, n_dev, n_host = res.sighash_pack()
    assert (n_dev, n_host) == (info["device_sigs"], info["host_sigs"])
    assert res.num_device_hashes == n_dev and ref.num_device_hashes == 0
    assert len(jobs) == n_dev * core.SIGHASH_JOB_BYTES and len(secp_jobs) == res.num_sigs * core.SECP_JOB_BYTES
    core.sighash_check_jobs(len(arena), jobs, res.num_sigs)
    full = core.secp_pack_jobs(items)
    sz = core.SECP_JOB_BYTES
    z_at, kind_at = 4 * 32, 5 * 32  # x, y, r, s, z (8 limbs each), kind
    digests = core.sighash_gather_model(arena, jobs)
    device = {}
    for k in range(n_dev):
        rec = U.JOB.unpack_from(jobs, k * core.SIGHASH_JOB_BYTES)
        device[rec[8]] = (k, rec[9])
    assert list(device) == sorted(device)  # block order
    for k in range(res.num_sigs):
        mine, want = secp_jobs[k * sz:(k + 1) * sz], full[k * sz:(k + 1) * sz]
        if k not in device:
            assert mine == want  # host-hashed: complete
            continue
        j, kind = device[k]
        assert struct.unpack_from("<I", mine, kind_at)[0] == core.SECP_KIND_INVALID
        assert mine[z_at:z_at + 32] == bytes(32)
        assert mine[:z_at] == want[:z_at]  # key and signature already in place
        assert kind == struct.unpack_from("<I", want, kind_at)[0]
        assert digests[32 * j:32 * j + 32] == items[k][2]
    # without defer_sigs the flag has nothing to act on
    blk, view, height, _ = make_consolidation_block(**FIXTURE)
    res, _ = core.connect_block(blk, height, view, True, False, defer_sighash=True)
    assert res.ok and res.num_sigs == 0


def test_deferred_block_with_a_bad_signature(core):
    blk, view, height, info = make_consolidation_block(**FIXTURE, bad_at=0)
    res, _ = core.connect_block(blk, height, view, True, True, defer_sighash=True)
    assert res.ok
    verdicts = [core.secp_verify(*it) for it in res.sig_items()]
    assert [k for k, v in enumerate(verdicts) if not v] == [info["bad_sig"]] == [0]


def test_check_jobs_rejects_what_the_kernel_must_not_see(core):
    arena = bytes(100)
    ok = U.JOB.pack(0, 10, 20, 96, 10, 0, 70, 4, 0, 2)
    core.sighash_check_jobs(len(arena), ok)
    assert len(core.sighash_gather_model(arena, ok)) == 32
    for bad in (U.JOB.pack(0, 10, 20, 97, 10, 0, 70, 4, 0, 2),          # last segment one byte out
                U.JOB.pack(0, 10, 20, 96, 101, 0, 70, 4, 0, 2),         # first segment too long
                U.JOB.pack(0xfffffff0, 0, 0, 0, 0x20, 0, 0, 0, 0, 2),   # offset + length wraps 32 bits
                U.JOB.pack(0, 0, 101, 0, 0, 0, 0, 0, 0, 2)):            # empty segment past the end
        with pytest.raises(ValueError):
            core.sighash_check_jobs(len(arena), bad)
        with pytest.raises(ValueError):
            core.sighash_gather_model(arena, bad)
    with pytest.raises(ValueError):
        core.sighash_check_jobs(len(arena), U.JOB.pack(0, 10, 20, 96, 10, 0, 70, 4, 1, 2))  # output 1 of 1
    core.sighash_check_jobs(len(arena), U.JOB.pack(0, 10, 20, 96, 10, 0, 70, 4, 1, 2), 2)
    with pytest.raises(ValueError):
        core.sighash_check_jobs(len(arena), ok + ok[:8])  # not whole records


def test_kernel_keeps_its_state_in_registers(tmp_path):
    """The message schedule and the SHA state are indexed by constants only: the compiler's resource
    report for the gfx950 code object shows no scratch, no spills and no LDS."""
    import re
    import subprocess

    from nodexa_chain_core_amd import _build

    hipcc = os.path.join(_build.ROCM, "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    kdir = os.path.join(_build.HIPDIR, "kernels")
    r = subprocess.run([hipcc, "--genco", "--offload-arch=" + _build.ARCH, "-O3", "-std=c++17",
                        "-mcode-object-version=5", "-I" + kdir, "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(kdir, "sighash.hip"), "-o", str(tmp_path / "sighash.hsaco")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rep = r.stderr[r.stderr.index("Function Name: sighash_gather_batch"):]
    usage = {k.strip(): v for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\w+) \[-Rpass", rep)}
    assert usage["ScratchSize [bytes/lane]"] == "0" and usage["Dynamic Stack"] == "False"
    assert usage["VGPRs Spill"] == "0" and usage["SGPRs Spill"] == "0" and usage["LDS Size [bytes/block]"] == "0"
    assert int(usage["VGPRs"]) <= 128  # at least 4 waves per SIMD


def test_gpusighash_flag(core, node_factory):
    import torch

    # the flag only acts with the GPU batch: a node that does not take it (no GPU here, or the batch
    # switched off where there is one) ignores the flag and connects its blocks on the host
    sigs = "-gpusigs=off" if torch.cuda.is_available() else "-gpusigs=on"
    node, addr = node_factory((sigs, "-gpusighash=1", "-maxsigcachesize=0"))
    assert node.state.gpu_sighash is True
    c = client(node)
    w = c.getnewaddress()
    c.generatetoaddress(101, w)
    c.sendtoaddress(c.getnewaddress(), 1.0)
    c.generatetoaddress(1, w)
    assert c.getblockcount() == 102 and c.getrawmempool() == []
    assert node.state.sig_stats["gpu_sighashes"] == 0 and node.state.sig_stats["gpu_batches"] == 0
    assert c.getgpuinfo()[0]["block_sigs"] == node.state.sig_stats


def test_gpusighash_defaults_off(core, node_factory):
    node, _ = node_factory()
    assert node.state.gpu_sighash is False
    assert {"gpu_sighashes", "host_sighashes"} <= set(node.state.sig_stats)
