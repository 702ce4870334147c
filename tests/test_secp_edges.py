"""The batch ECDSA verifier at its edges, against Python integers (tests/secp_ref.py).

Primitive tier: every function of hip/kernels/secp256k1_device.hpp that the verifier is made of,
run through one op switch (secp256k1_probe.hpp) on the host (`_core.secp32_probe`) and on the
device (secp256k1_probe.hip), over an edge set of 256-bit values whose pairs take the rare carry
and reduction branches that random operands never reach. Signature tier: constructed signatures
that meet a doubling or an inverse inside an addition, R at infinity, x(R) >= n, keys at and past
p, every key encoding, s and z at their ends, each with the exact raw verdict (1, 0, or 2 = "ask
the host") the kernel has to give; and the launch grid's tail."""
import functools
import itertools
import random
import struct
from collections import Counter

import pytest

import secp_ref as ref
from secp_ref import M256, N, NC, P
from test_secp_batch import cases

# op selectors of secp256k1_probe.hpp
F_MUL, F_SQR, F_ADD, F_SUB, F_INV, F_SQRT, S_MUL, S_INV, F_GEQ_P, S_GEQ_N, S_SUB_N, J_DOUBLE, J_ADD_AFFINE = range(13)
IN_WORDS, OUT_WORDS = 40, 25
SENTINEL = 0x5EC9DEAD


def pack(records) -> bytes:
    """Records of up to five 256-bit values as 8 little-endian 32-bit limbs each."""
    return b"".join(b"".join(v.to_bytes(32, "little") for v in rec).ljust(IN_WORDS * 4, b"\0") for rec in records)


def unpack(out: bytes) -> list[tuple[int, int, int, int]]:
    """(out0, out1, out2, flag) per record."""
    assert len(out) % (OUT_WORDS * 4) == 0
    res = []
    for o in range(0, len(out), OUT_WORDS * 4):
        res.append(tuple(int.from_bytes(out[o + 32 * k:o + 32 * k + 32], "little") for k in range(3))
                   + (int.from_bytes(out[o + 96:o + 100], "little"),))
    return res


@functools.lru_cache(maxsize=None)
def all_values() -> tuple[int, ...]:
    edge, rnd = ref.edge_values()
    return edge + rnd


@functools.lru_cache(maxsize=None)
def point_records():
    """(j_double records, j_add_affine records); a record is (limb values, the affine points it
    stands for). Every point goes in as (x, y, 1) and as four other Jacobian representatives; the
    additions pair each with every point of the list and its negative, so P + P and P + (-P) are
    among them under every representative."""
    rng = random.Random(78)
    pts = ref.probe_points()
    dbl, addr = [], []
    for p in pts:
        for jf in ref.jacobian_forms(p, rng):
            dbl.append((jf, (p,)))
            for q in pts:
                for qq in (q, ref.neg(q)):
                    addr.append((jf + qq, (p, qq)))
    return tuple(dbl), tuple(addr)


@functools.lru_cache(maxsize=None)
def op_records(op: int) -> tuple:
    """The input records of an op, on the domain the header states for it."""
    vals = all_values()
    if op in (F_MUL, S_MUL):  # unreduced inputs are legal: the folds take any 512-bit product
        return tuple(itertools.product(vals, vals))
    if op in (F_ADD, F_SUB):
        lo = [v for v in vals if v < P]
        return tuple(itertools.product(lo, lo))
    if op in (F_INV, F_SQRT):
        return tuple((v,) for v in vals if 1 <= v < P)
    if op == S_INV:
        return tuple((v,) for v in vals if 1 <= v < N)
    if op == J_DOUBLE:
        return tuple(r for r, _ in point_records()[0])
    if op == J_ADD_AFFINE:
        return tuple(r for r, _ in point_records()[1])
    return tuple((v,) for v in vals)  # F_SQR and the single-operand predicates and helpers


def check_against_python(op: int, out: bytes) -> None:
    recs, got = op_records(op), unpack(out)
    assert len(got) == len(recs) and len(recs) > 0
    if op in (J_DOUBLE, J_ADD_AFFINE):
        meta = [m for _, m in point_records()[op - J_DOUBLE]]
        n_deg = 0
        for rec, pts, (X, Y, Z, flag) in zip(recs, meta, got):
            if op == J_DOUBLE:
                want, deg = ref.double(pts[0]), False
            else:
                want, deg = ref.add(*pts), pts[0][0] == pts[1][0]  # P + P or P + (-P)
            assert flag == int(deg), ("degenerate flag", [hex(v) for v in rec])
            n_deg += deg
            if not deg:
                assert Z % P != 0 and ref.affine_of(X, Y, Z) == want, [hex(v) for v in rec]
        if op == J_ADD_AFFINE:  # both kinds under each of the five representatives of each point
            assert n_deg == 2 * 5 * len(ref.probe_points())
        return
    for rec, (o0, o1, o2, flag) in zip(recs, got):
        a, b = rec[0], rec[-1]
        want = {
            F_MUL: lambda: (a * b % P, 0),
            F_SQR: lambda: (a * a % P, 0),
            F_ADD: lambda: ((a + b) % P, 0),
            F_SUB: lambda: ((a - b) % P, 0),
            F_INV: lambda: (pow(a, -1, P), 0),
            # the root a^((p+1)/4) when a is a square, false when it is not; the power either way
            F_SQRT: lambda: (pow(a, (P + 1) // 4, P), int(ref.sqrt_p(a) is not None)),
            S_MUL: lambda: (a * b % N, 0),
            S_INV: lambda: (pow(a, -1, N), 0),
            F_GEQ_P: lambda: (0, int(a >= P)),
            S_GEQ_N: lambda: (0, int(a >= N)),
            S_SUB_N: lambda: ((a + NC) & M256, 0),
        }[op]()
        assert (o0, flag) == want and o1 == 0 and o2 == 0, (op, [hex(v) for v in rec], hex(o0), flag)
        if op == F_SQRT and flag:
            assert o0 == ref.sqrt_p(a)


ALL_OPS = list(range(13))
OP_NAMES = ["f_mul", "f_sqr", "f_add", "f_sub", "f_inv", "f_sqrt", "s_mul", "s_inv", "f_geq_p", "s_geq_n", "s_sub_n",
            "j_double", "j_add_affine"]


# ---------------------------------------------------------------- the vectors themselves
def test_edge_set_reaches_the_rare_branches():
    """Agreement on E x E means little unless the pairs take the branches: count, with the folds
    mirrored on whole integers, the pairs that take each rare branch of f_mul and s_mul."""
    edge, rnd = ref.edge_values()
    assert len(edge) == 134 and len(rnd) == 32
    f, s = Counter(), Counter()
    for a, b in op_records(F_MUL):
        r, taken = ref.classify_f_mul(a, b)
        assert r == a * b % P
        f.update(taken)
        r, taken = ref.classify_s_mul(a, b)
        assert r == a * b % N
        s.update(taken)
    print("f_mul branches", dict(f), "s_mul branches", dict(s))
    assert f["k2"] >= 1     # the carry out of the second fold: if (k2) f_add_pc(r, k2)
    assert f["geq"] >= 1    # the final f_geq_p subtraction
    assert s["carry"] >= 1  # the carry out of the third fold: if (c) s_sub_n(r)
    assert s["sub1"] >= 1   # the first conditional s_sub_n
    # The second conditional s_sub_n is not required: no pair of the set takes it and none was
    # found that does. After the first one r < 2^256 - n < n, so it looks unreachable.
    assert s["sub2"] == 0
    # The same classifiers on random pairs take none of the branches, which is why tests on
    # random signatures never get there.
    rng = random.Random(1)
    rare = Counter()
    for _ in range(2000):
        a, b = rng.getrandbits(256), rng.getrandbits(256)
        rare.update(ref.classify_f_mul(a, b)[1] | ref.classify_s_mul(a, b)[1])
    assert not rare


def test_python_reference_is_sound():
    """The reference against facts it was not built from: group order, known multiples of G."""
    assert ref.on_curve(ref.G) and ref.mul(N, ref.G) is None and ref.mul(N - 1, ref.G) == ref.neg(ref.G)
    assert ref.double(ref.G) == (0xC6047F9441ED7D6D3045406E95C07CD85C778E4B8CEF3CA7ABAC09B95C709EE5,
                                 0x1AE168FEA63DC339A3C58419466CEAEEF7F632653266D0E1236431A950CFE52A)
    assert ref.mul(3, ref.G)[0] == 0xF9308A019258C31049344F85F89D5229B531C845836F99B08601F113BCE036F9
    assert ref.add(ref.G, ref.neg(ref.G)) is None and ref.add(ref.G, ref.G) == ref.double(ref.G)
    assert all(ref.on_curve(p) for p in ref.probe_points())
    assert ref.sqrt_p(8) is not None and ref.lift_x(N + 1) is None and ref.lift_x(N + 2) is not None
    d, z, k = 0x1234567, 0xABCDEF, 0x7654321
    r = ref.mul(k, ref.G)[0] % N
    s = pow(k, -1, N) * (z + r * d) % N
    assert ref.ecdsa_verify(ref.mul(d, ref.G), r, s, z) and not ref.ecdsa_verify(ref.mul(d, ref.G), r, s, z + 1)


# ---------------------------------------------------------------- primitives, host build
@pytest.mark.parametrize("op", ALL_OPS, ids=OP_NAMES)
def test_host_primitive_matches_python(core, op):
    out = core.secp32_probe(op, pack(op_records(op)))
    assert len(out) == len(op_records(op)) * core.SECP_PROBE_OUT_BYTES
    check_against_python(op, out)


def test_probe_record_layout(core):
    assert (core.SECP_PROBE_IN_BYTES, core.SECP_PROBE_OUT_BYTES) == (IN_WORDS * 4, OUT_WORDS * 4)
    with pytest.raises(ValueError):
        core.secp32_probe(13, pack([(1, 2)]))
    with pytest.raises(ValueError):
        core.secp32_probe(F_MUL, pack([(1, 2)])[:-1])


# ---------------------------------------------------------------- whole signatures, host model
def _random_fill(core, n, seed):
    """(item, host-model verdict) of the random mix of test_secp_batch, to pad a launch with."""
    return [((p, s, m), core.secp_verify_model32(p, s, m)) for p, s, m, _ in cases(core, n, seed=seed)]


def test_vectors_cover_the_table():
    vs = ref.signature_vectors()
    assert len({v.name for v in vs}) == len(vs) >= 40
    assert Counter(v.raw for v in vs)[2] == 5 and {v.raw for v in vs} == {0, 1, 2}
    # a raw 1 is final, a raw 0 is final; only a 2 leaves the answer to the host
    assert all(v.final == (v.raw == 1) for v in vs if v.raw != 2)
    assert all(v.s <= N // 2 for v in vs if v.raw == 2)


@pytest.mark.parametrize("v", ref.signature_vectors(), ids=lambda v: v.name)
def test_model32_vector_verdict(core, v):
    assert ref.verify_bytes(v.pub, v.r, v.s, v.msg) == v.final  # the table against the definition
    assert bool(core.secp_verify(v.pub, v.sig, v.msg)) == v.final
    assert core.secp_verify_model32(v.pub, v.sig, v.msg) == v.raw


def test_model32_random_sets_never_ask_the_host(core):
    """Verdict 2 is for the constructed rows alone: on random signatures it must not appear, or a
    verifier that answered 2 to everything would pass every test that settles a 2 on the host."""
    for seed, n in ((11, 48), (5, 1000)):
        cs = cases(core, n, seed=seed)
        got = [core.secp_verify_model32(p, s, m) for p, s, m, _ in cs]
        assert set(got) <= {0, 1}
        assert [g == 1 for g in got] == [e for *_, e in cs]


# ---------------------------------------------------------------- device
def _gpu_probe(op: int, records: bytes, n: int) -> bytes:
    import numpy as np
    import torch

    from nodexa_chain_core_amd.ops import runtime

    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        kern = runtime.static_kernel("secp256k1_probe", "secp_probe")
        d_in = torch.frombuffer(bytearray(records), dtype=torch.int32).to(dev)
        assert d_in.numel() == n * IN_WORDS
        d_out = torch.full((n * OUT_WORDS + 8,), SENTINEL, dtype=torch.int32, device=dev)
        kern.launch(((n + 63) // 64, 1, 1), (64, 1, 1), 0, runtime.current_stream_handle(),
                    struct.pack("<QQII", d_in.data_ptr(), d_out.data_ptr(), op, n))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().astype(np.uint32)
    assert (out[n * OUT_WORDS:] == SENTINEL).all(), "the probe wrote past its last record"
    return out[:n * OUT_WORDS].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("op", ALL_OPS, ids=OP_NAMES)
def test_gpu_primitive_matches_host_and_python(core, gpu, op):
    records = pack(op_records(op))
    out = _gpu_probe(op, records, len(op_records(op)))
    assert out == core.secp32_probe(op, records)  # the device build of the header, byte for byte
    check_against_python(op, out)


def _gpu_raw_with_guard(items, extra=8):
    """One launch of secp_verify_batch into a buffer `extra` words longer than the batch."""
    import numpy as np
    import torch

    from nodexa_chain_core_amd import _core
    from nodexa_chain_core_amd.ops import runtime, secp

    dev = torch.device("cuda", 0)
    n = len(items)
    with torch.cuda.device(dev):
        kern = runtime.static_kernel("secp256k1_verify", "secp_verify_batch")
        jobs = torch.frombuffer(bytearray(_core.secp_pack_jobs(list(items))), dtype=torch.int32).to(dev)
        out = torch.full((n + extra,), SENTINEL, dtype=torch.int32, device=dev)
        runtime.hip().launch_secp_verify(kern, jobs.data_ptr(), n, secp._gen_table(dev).data_ptr(), out.data_ptr(),
                                         runtime.current_stream_handle())
        torch.cuda.synchronize()
        got = out.cpu().numpy().astype(np.uint32)
    return got[:n].tolist(), got[n:].tolist()


@pytest.mark.gpu
def test_gpu_vector_verdicts(core, gpu):
    from nodexa_chain_core_amd.ops import secp

    vs = ref.signature_vectors()
    raw = secp.verify_batch_raw([v.item for v in vs], device=0)
    final = secp.verify_batch([v.item for v in vs], device=0)
    for v, got_raw, got_final in zip(vs, raw, final):
        assert got_raw == core.secp_verify_model32(*v.item) == v.raw, v.name
        assert got_final == ref.verify_bytes(v.pub, v.r, v.s, v.msg) == bool(core.secp_verify(*v.item)) == v.final, v.name


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 256, 257])
def test_gpu_grid_tail(core, gpu, n):
    """Blocks are 256 wide: one job, one full block, one job past it. The verdict words beyond the
    batch stay as they were, and the first n are right."""
    vs = ref.signature_vectors()
    batch = ([(v.item, v.raw) for v in vs] + _random_fill(core, 257 - len(vs), seed=23))[:n]
    assert batch[0][1] == 2  # alone at n = 1: a doubling vector, so a zeroed or skipped word shows
    got, guard = _gpu_raw_with_guard([it for it, _ in batch])
    assert guard == [SENTINEL] * 8
    assert got == [w for _, w in batch]


@pytest.mark.gpu
def test_gpu_verdict_independent_of_position(core, gpu):
    vs = ref.signature_vectors()
    batch = [(v.item, v.raw) for v in vs] + _random_fill(core, 300 - len(vs), seed=29)
    order = list(range(len(batch)))
    random.Random(31).shuffle(order)
    a, _ = _gpu_raw_with_guard([it for it, _ in batch])
    b, _ = _gpu_raw_with_guard([batch[i][0] for i in order])
    assert a == [w for _, w in batch]
    assert b == [batch[i][1] for i in order]
    assert set(a) <= {0, 1, 2} and Counter(a)[2] == Counter(v.raw for v in vs)[2]
