"""Every form of signature hash on the host (csrc/chain/sighash.cpp pack_sighash_var,
sighash_var_model, sighash_var_check; connect_block(defer_all_forms=True); -gpusighash=2):
the plain-Python yardstick against the reference's sighash.json, the kernel's model over tables
packed in Python and by the native packer, the block path and the node flag."""
import collections
import json
import os
import struct

import pytest

import sighash_forms_util as F
import sighash_ref as R
from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block
from test_node_rpc import client, node_factory  # noqa: F401 — shared fixture
from test_sighash_pack import REF_VECTORS  # the reference's sighash.json, where present

Z_AT, KIND_AT = 4 * 32, 5 * 32  # SecpVerifyJob: x, y, r, s, z (8 limbs each), kind


@pytest.fixture(scope="module")
def vectors():
    if not os.path.exists(REF_VECTORS):
        pytest.skip("reference vector file sighash.json not present")
    with open(REF_VECTORS) as f:
        v = [t for t in json.load(f) if not (len(t) == 1 and isinstance(t[0], str))]
    assert len(v) == 500
    return [((bytes.fromhex(raw), n_in, bytes.fromhex(script), ht, 0, 0), expect) for raw, script, n_in, ht, expect in v]


@pytest.fixture(scope="module")
def cases(core):
    return F.edge_cases(core)


@pytest.fixture(scope="module")
def packed(cases):
    return F.pack_cases(cases)


@pytest.fixture(scope="module")
def key(core):
    sec = bytes(31) + b"\x05"
    return core.secp_pubkey_create(sec, True), core.secp_sign(bytes(32), sec)


# ---------------------------------------------------------------- 1, 2: the reference's vectors
def test_ref_reproduces_the_reference_vectors(core, vectors):
    bad = [k for k, (c, expect) in enumerate(vectors) if F.ref_hashes([c])[0][::-1].hex() != expect]
    assert not bad, f"{len(bad)} of 500 differ, first: {vectors[bad[0]]}"
    forms = collections.Counter(F.form_name(c[3]) for c, _ in vectors)
    assert forms == {"all": 253, "all|acp": 214, "none": 9, "single": 9, "single|acp": 8, "none|acp": 7}
    assert all(core.sighash_form(0, c[3]) == F.form_name(c[3]) for c, _ in vectors)
    assert not any(F.is_constant_one(c) for c, _ in vectors)  # the constructed cases must reach it


def test_model_on_the_reference_vectors(core, vectors):
    cs = [c for c, _ in vectors]
    arena, segs, jobs, job_case = F.pack_cases(cs, with_empty=False)
    assert job_case == list(range(500))  # 500 of 500 are expressible as segments
    core.sighash_var_check(len(arena), segs, jobs)
    got = core.sighash_var_model(arena, segs, jobs)
    bad = [k for k, (_, expect) in enumerate(vectors) if got[32 * k:32 * k + 32][::-1].hex() != expect]
    assert not bad, f"{len(bad)} of 500 differ, first: {vectors[bad[0]]}"


# ---------------------------------------------------------------- 3: the seeded edge set
def test_edge_cases_cover_the_edges(core, cases, packed):
    """The generator reaches what it claims to: the tests below are only as good as this."""
    assert 880 <= len(cases) <= 940
    parsed = {}
    seen = collections.defaultdict(set)
    for raw, i, code, ht, amount, sv in cases:
        tx = parsed.setdefault(raw, R.parse_tx(raw))
        form = (sv, F.form_name(ht))
        assert core.sighash_form(sv, ht) == form[1]
        pre = R.preimage(code, tx, i, ht, amount, sv)
        if pre is not None:
            seen["residue"].add((form, len(pre) % 64))
        seen["code"].add((form, len(code)))
        seen["codesep"].add((form, code))
        if sv == 0:
            seen["vin"].add((form[1], len(tx["vin"]), i))
            if form[1].startswith("single"):
                seen["single"].add((form[1], i, len(tx["vout"])))
        seen["type"].add((sv, ht))
        seen["amount"].add((sv, amount))
    forms = [(sv, F.FORM_NAMES[ht]) for sv, ht in F.FORMS]
    assert len(set(forms)) == 12
    assert seen["residue"] >= {(f, r) for f in forms for r in (0, 1, 55, 56, 63)}
    assert seen["code"] >= {(f, n) for f in forms for n in (0, 1, 25, 252, 253, 520)}
    assert seen["codesep"] >= {(f, c) for f in forms for c in F.CODESEP_CODES}
    for name in ("none", "single", "all|acp", "none|acp", "single|acp"):
        assert seen["vin"] >= {(name, n, i) for n in (1, 2, 252, 253) for i in (0, n - 1)}, name
    for name in ("single", "single|acp"):
        # along the blank run; the last output; vout.size() itself and beyond (the constant one)
        assert seen["single"] >= {(name, i, 253) for i in (0, 1, 251, 252)}
        assert seen["single"] >= {(name, 251, 252), (name, 252, 252), (name, 1, 2), (name, 2, 2), (name, 3, 2)}
    ones = [c for c in cases if F.is_constant_one(c)]
    assert len(ones) >= 6 and {F.form_name(c[3]) for c in ones} == {"single", "single|acp"}
    assert all(h == R.ONE for h in F.ref_hashes(ones))
    for sv in (0, 1):
        assert seen["type"] >= {(sv, ht) for ht in F.WIDE_TYPES}
        for base in (1, 2, 3):  # a full 32-bit and a negative type in each base class
            assert any(s == sv and ht & 0x1f == base and ht > 0xffff for s, ht in seen["type"])
            assert any(s == sv and ht & 0x1f == base and ht < 0 for s, ht in seen["type"])
    assert (1, F.BIG_AMOUNT) in seen["amount"] and F.BIG_AMOUNT >> 56
    # the Python tables: exactly 8 segments, one segment, interior empty segments, no segment at all
    arena, segs, jobs, job_case = packed
    counts = F.seg_counts(segs, jobs)
    assert {n for n, _ in counts} >= {0, 1, 4, 7, 8} and max(n for n, _ in counts) == core.SIGHASH_VAR_MAX_SEGMENTS == 8
    assert any(n >= 3 and 0 in lens[1:-1] and lens[0] and lens[-1] for n, lens in counts)
    assert counts[-1][0] == 0 and job_case[-1] is None
    # more than three workgroups of 256 lanes, the last one partly filled
    assert len(job_case) > 3 * 256 and len(job_case) % 256
    assert len(job_case) == len(cases) - len(ones) + 1
    assert core.SIGHASH_SEG_BYTES == F.SEG.size and core.SIGHASH_VAR_JOB_BYTES == F.JOB.size


def test_ref_matches_signature_hash(core, cases):
    ref, host = F.ref_hashes(cases), F.host_hashes(core, cases)
    bad = [k for k in range(len(cases)) if ref[k] != host[k]]
    assert not bad, f"{len(bad)} of {len(cases)} differ, first: {cases[bad[0]][1:]}"


def test_model_matches_on_the_edge_set(core, cases, packed):
    arena, segs, jobs, job_case = packed
    core.sighash_var_check(len(arena), segs, jobs)
    got, want = core.sighash_var_model(arena, segs, jobs), F.expected_digests(cases, job_case)
    assert len(got) == 32 * len(job_case)
    bad = [k for k in range(len(job_case)) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
    assert not bad, f"{len(bad)} of {len(job_case)} differ, first: {cases[job_case[bad[0]]][1:]}"
    assert got[-32:] == R.sha256d(b"")  # the job without segments hashes the empty string


def test_native_packer_on_the_edge_set(core, cases, key):
    """pack_sighash_var over the same signatures: its digests are the yardstick's, and exactly the
    constant-one cases come out host-filled, z = 1 with the real kind."""
    res = core.sighash_pack_var_cases(cases, *key)
    ref = F.ref_hashes(cases)
    assert res.all_forms and [it[2] for it in res.sig_items()] == ref
    arena, segs, jobs, secp_jobs, n_dev, n_host = res.sighash_pack_var()
    ones = [k for k, c in enumerate(cases) if F.is_constant_one(c)]
    assert (n_dev, n_host) == (len(cases) - len(ones), len(ones)) and res.num_device_hashes == n_dev
    core.sighash_var_check(len(arena), segs, jobs, len(cases))
    digests = core.sighash_var_model(arena, segs, jobs)
    device = {}
    for j in range(n_dev):
        first, n_seg, out, kind = F.JOB.unpack_from(jobs, j * F.JOB.size)
        assert 1 <= n_seg <= 8
        device[out] = (j, kind)
    assert list(device) == sorted(device) and not set(device) & set(ones)
    sz = core.SECP_JOB_BYTES
    full = core.secp_pack_jobs([(key[0], key[1], m) for m in ref])
    real_kind = struct.unpack_from("<I", full, KIND_AT)[0]
    assert real_kind in (2, 3)
    for k in range(len(cases)):
        mine = secp_jobs[k * sz:(k + 1) * sz]
        if k in device:
            j, kind = device[k]
            assert digests[32 * j:32 * j + 32] == ref[k], cases[k][1:]
            assert struct.unpack_from("<I", mine, KIND_AT)[0] == core.SECP_KIND_INVALID and kind == real_kind
            assert mine[Z_AT:Z_AT + 32] == bytes(32)
        else:
            assert k in ones and mine == full[k * sz:(k + 1) * sz]
            # the message is uint256 one (first byte 1); z is its bytes as a big-endian integer, in little-endian limbs
            assert mine[Z_AT:Z_AT + 32] == R.ONE[::-1]
            assert struct.unpack_from("<I", mine, KIND_AT)[0] == real_kind


# ---------------------------------------------------------------- 4: connect_block
# the seed is one at which no legacy SINGLE signs input 2 or above of these two-output transactions
FIXTURE = dict(n_txs=6, inputs_per_tx=(1, 9), seed=143, hash_types=(1, 0x81, 2, 3, 0x82, 0x83, 0), witness_every=4,
               multisig_every=5)


def _connect(core, defer_sighash=False, **kw):
    blk, view, height, info = make_consolidation_block(**FIXTURE, **{k: v for k, v in kw.items() if k == "bad_at"})
    opts = {k: v for k, v in kw.items() if k != "bad_at"}
    res, _ = core.connect_block(blk, height, view, True, True, defer_sighash=defer_sighash, **opts)
    assert res.ok
    return res, info


def test_connect_block_defers_every_form(core):
    ref, info = _connect(core)
    res, _ = _connect(core, True, defer_all_forms=True)
    assert res.all_forms and not ref.all_forms
    assert res.num_sigs == info["sigs"] and info["host_sigs"] > 0
    items = res.sig_items()
    assert items == ref.sig_items() and res.sig_at == ref.sig_at
    assert all(core.secp_verify(*it) for it in items)
    arena, segs, jobs, secp_jobs, n_dev, n_host = res.sighash_pack_var()
    # two outputs per transaction and no legacy SINGLE at input 2 or above: nothing is left to the host
    assert (n_dev, n_host) == (info["sigs"], 0) and res.num_device_hashes == n_dev
    assert res.num_device_v0 > 0 and res.num_device_partial > 0
    assert res.num_device_v0 + res.num_device_partial + info["device_sigs"] == n_dev
    assert len(jobs) == n_dev * core.SIGHASH_VAR_JOB_BYTES and len(secp_jobs) == n_dev * core.SECP_JOB_BYTES
    core.sighash_var_check(len(arena), segs, jobs, res.num_sigs)
    digests = core.sighash_var_model(arena, segs, jobs)
    full = core.secp_pack_jobs(items)
    sz = core.SECP_JOB_BYTES
    for k in range(n_dev):
        first, n_seg, out, kind = F.JOB.unpack_from(jobs, k * F.JOB.size)
        assert out == k  # block order, every signature a job
        mine, want = secp_jobs[k * sz:(k + 1) * sz], full[k * sz:(k + 1) * sz]
        assert struct.unpack_from("<I", mine, KIND_AT)[0] == core.SECP_KIND_INVALID
        assert mine[Z_AT:Z_AT + 32] == bytes(32) and mine[:Z_AT] == want[:Z_AT]
        assert kind == struct.unpack_from("<I", want, KIND_AT)[0]
        assert digests[32 * k:32 * k + 32] == items[k][2]
    with pytest.raises(ValueError):
        res.sighash_pack()  # four fixed segments cannot express these forms


def test_all_forms_block_with_a_bad_signature(core):
    for bad_at in (1, 2, 3):
        res, info = _connect(core, True, defer_all_forms=True, bad_at=bad_at)
        verdicts = [core.secp_verify(*it) for it in res.sig_items()]
        assert [k for k, v in enumerate(verdicts) if not v] == [info["bad_sig"]]


def test_keyword_false_changes_nothing(core):
    old, info = _connect(core, True)
    new, _ = _connect(core, True, defer_all_forms=False)
    assert not new.all_forms and new.sighash_pack() == old.sighash_pack() and new.sig_items() == old.sig_items()
    assert new.num_device_hashes == info["device_sigs"] and new.num_device_v0 == new.num_device_partial == 0
    # without defer_sighash the keyword has nothing to act on
    plain, _ = _connect(core, False, defer_all_forms=True)
    assert not plain.all_forms and plain.num_device_hashes == 0 and plain.sig_items() == old.sig_items()
    with pytest.raises(ValueError):
        old.sighash_pack_var()  # templates only: not connected for this packer


# ---------------------------------------------------------------- 5: the arena stays linear
def test_arena_bound(core, key):
    import random

    import sighash_util as U

    rng = random.Random(3)
    raw = U.make_tx(core, rng, 253, tuple(rng.randrange(20, 30) for _ in range(253)))
    code = U.plain_code(rng, 25)
    cs = [(raw, i, code, ht, 0, 0) for i in range(253) for ht in (0x03, 0x02)]
    res = core.sighash_pack_var_cases(cs, *key)
    arena, segs, jobs, _, n_dev, n_host = res.sighash_pack_var()
    assert (n_dev, n_host) == (506, 0)
    bound = 3 * len(raw) + sum(len(R.legacy_script_code(c[2])) + 64 for c in cs) + 9 * 253
    assert len(arena) < bound, (len(arena), bound)
    got = core.sighash_var_model(arena, segs, jobs)
    assert got == b"".join(F.ref_hashes(cs))
    # witness v0: at most the emitted code + 160 bytes each, nothing shared needed
    ws = [(raw, i, code, ht, 5, 1) for i in range(0, 253, 50) for ht in F.LEGACY_TYPES]
    arena, segs, jobs, _, n_dev, _ = core.sighash_pack_var_cases(ws, *key).sighash_pack_var()
    assert n_dev == len(ws) and len(arena) <= sum(len(R.compact_size(len(c[2])) + c[2]) + 160 for c in ws)
    assert core.sighash_var_model(arena, segs, jobs) == b"".join(F.ref_hashes(ws))


# ---------------------------------------------------------------- 6: nothing malformed reaches the device
def test_var_check_rejects_what_the_kernel_must_not_see(core):
    arena = bytes(100)
    seg, job = F.SEG.pack, F.JOB.pack
    nine = b"".join(seg(k, 1) for k in range(9))
    twins = [  # (malformed, well-formed twin) as (segs, jobs, n_out)
        ((seg(0, 10) + seg(97, 4), job(0, 2, 0, 2), None), (seg(0, 10) + seg(96, 4), job(0, 2, 0, 2), None)),
        ((seg(0xfffffff0, 0x20), job(0, 1, 0, 2), None), (seg(0x50, 0x14), job(0, 1, 0, 2), None)),  # 32-bit wrap
        ((seg(0, 10) + seg(10, 4), job(1, 2, 0, 2), None), (seg(0, 10) + seg(10, 4), job(0, 2, 0, 2), None)),
        ((nine, job(0, 9, 0, 2), None), (nine, job(1, 8, 0, 2), None)),
    ]
    out_twin = ((seg(0, 10), job(0, 1, 1, 2), None), (seg(0, 10), job(0, 1, 1, 2), 2))  # output 1 of 1 / of 2
    for (bs, bj, bn), (gs, gj, gn) in twins + [out_twin]:
        with pytest.raises(ValueError):
            core.sighash_var_check(len(arena), bs, bj, bn)
        if (bs, bj, bn) != out_twin[0]:  # the model writes its rows in job order: no output index to refuse
            with pytest.raises(ValueError):
                core.sighash_var_model(arena, bs, bj)
        core.sighash_var_check(len(arena), gs, gj, gn)
        assert len(core.sighash_var_model(arena, gs, gj)) == 32
    # a segment past the end is refused even when no job names it, and an empty one at the very end is fine
    with pytest.raises(ValueError):
        core.sighash_var_check(len(arena), seg(101, 0), b"")
    core.sighash_var_check(len(arena), seg(100, 0), job(0, 1, 0, 2))
    # a message of 2^29 bytes: eight ranges of 2^26 (the check alone decides; the twin is one byte short)
    big = 1 << 26
    long_segs = seg(0, big) * 8
    with pytest.raises(ValueError):
        core.sighash_var_check(big, long_segs, job(0, 8, 0, 2))
    with pytest.raises(ValueError):
        core.sighash_var_model(bytes(big), long_segs, job(0, 8, 0, 2))
    core.sighash_var_check(big, seg(0, big) * 7 + seg(0, big - 1), job(0, 8, 0, 2))
    for bad in ((seg(0, 4)[:5], job(0, 0, 0, 2)), (seg(0, 4), job(0, 1, 0, 2)[:12])):  # not whole records
        with pytest.raises(ValueError):
            core.sighash_var_check(len(arena), *bad)


# ---------------------------------------------------------------- 7: the compiler's report
def test_var_kernel_keeps_its_state_in_registers(tmp_path):
    """The read position and the segment descriptors are named registers, the message schedule and
    the SHA state indexed by constants only: no scratch, no spills, no LDS, at most 128 VGPRs."""
    import re
    import subprocess

    from nodexa_chain_core_amd import _build

    hipcc = os.path.join(_build.ROCM, "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    kdir = os.path.join(_build.HIPDIR, "kernels")
    r = subprocess.run([hipcc, "--genco", "--offload-arch=" + _build.ARCH, "-O3", "-std=c++17",
                        "-mcode-object-version=5", "-I" + kdir, "-Rpass-analysis=kernel-resource-usage",
                        os.path.join(kdir, "sighash_var.hip"), "-o", str(tmp_path / "sighash_var.hsaco")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rep = r.stderr[r.stderr.index("Function Name: sighash_gather_var"):]
    usage = {k.strip(): v for k, v in re.findall(r"remark:\s+([A-Za-z /\[\]]+?): (\w+) \[-Rpass", rep)}
    assert usage["ScratchSize [bytes/lane]"] == "0" and usage["Dynamic Stack"] == "False"
    assert usage["VGPRs Spill"] == "0" and usage["SGPRs Spill"] == "0" and usage["LDS Size [bytes/block]"] == "0"
    assert int(usage["VGPRs"]) <= 128  # at least 4 waves per SIMD


# ---------------------------------------------------------------- 8: the node flag
def test_gpusighash_2_flag(core, node_factory):
    import torch

    # as test_gpusighash_flag: a node without the GPU batch ignores the flag and connects on the host
    sigs = "-gpusigs=off" if torch.cuda.is_available() else "-gpusigs=on"
    node, addr = node_factory((sigs, "-gpusighash=2", "-maxsigcachesize=0"))
    assert node.state.gpu_sighash is True and node.state.gpu_sighash_forms == "all"
    c = client(node)
    w = c.getnewaddress()
    c.generatetoaddress(101, w)
    c.sendtoaddress(c.getnewaddress(), 1.0)
    c.generatetoaddress(1, w)
    assert c.getblockcount() == 102 and c.getrawmempool() == []
    st = node.state.sig_stats
    assert st["gpu_sighashes"] == st["gpu_sighashes_v0"] == st["gpu_sighashes_partial"] == st["gpu_batches"] == 0
    assert c.getgpuinfo()[0]["block_sigs"] == st


@pytest.mark.parametrize("flag,on,forms", [(None, False, "legacy-all"), ("-gpusighash=0", False, "legacy-all"),
                                           ("-gpusighash=1", True, "legacy-all")])
def test_gpusighash_0_and_1_as_before(core, node_factory, flag, on, forms):
    node, _ = node_factory((flag,) if flag else ())
    assert node.state.gpu_sighash is on and node.state.gpu_sighash_forms == forms
    assert {"gpu_sighashes_v0", "gpu_sighashes_partial"} <= set(node.state.sig_stats)
    assert all(isinstance(v, int) for v in node.state.sig_stats.values())
