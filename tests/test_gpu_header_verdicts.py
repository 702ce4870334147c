"""hip/kernels/header_batch.hip on the MI355X, its two deciding kernels alone on hand-built
buffers: `hb_verdict` (KawPow rows: high-hash / invalid-mix-hash / valid, the checkpoint rule) and
`hb_eq_scatter` (Equihash rows: nBits decoded on the device, SHA256d hash against it).

Real hashing never lands on final == boundary, boundary == pow limit, a mix that differs in one
word or a hash one unit from an exotic target, so the fixture tests cannot see a `<` for a `<=` or
a byte-order slip there. The oracle is CheckProofOfWork on Python integers (negative, zero,
overflowing, above the pow limit, hash <= target), cross-checked with core.check_proof_of_work and
core.set_compact wherever a case has an nBits form."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW = 128
MARK = 0xA5  # prefilled into every output byte: neither a code nor likely in 32 zero-ish hash bytes
M256 = (1 << 256) - 1
EPOCH = 7500


# ------------------------------------------------------------------------------- the oracle
def decode_compact(bits: int):
    """arith_uint256::SetCompact: (target, negative, overflow)."""
    size, word = bits >> 24, bits & 0x007FFFFF
    if size <= 3:
        word >>= 8 * (3 - size)
        target = word
    else:
        target = (word << 8 * (size - 3)) & M256
    negative = word != 0 and (bits & 0x00800000) != 0
    overflow = word != 0 and (size > 34 or (word > 0xFF and size > 33) or (word > 0xFFFF and size > 32))
    return target, negative, overflow


def target_ok(target: int, pow_limit: int, negative=False, overflow=False) -> bool:
    return not (negative or overflow or target == 0 or target > pow_limit)


def check_pow(hash_int: int, bits: int, pow_limit: int) -> bool:
    target, negative, overflow = decode_compact(bits)
    return target_ok(target, pow_limit, negative, overflow) and hash_int <= target


def verdict(c: dict, last_checkpoint: int, pow_limit: int):
    """hb_verdict's code for one row, None = the row's code is left as it was."""
    if c["kind"] == 2:
        return None
    if c["kind"] != 0:
        return 255
    below = last_checkpoint >= 0 and c["height"] <= last_checkpoint
    final = c["mo_final"] if below else c["full_final"]
    if not (target_ok(c["boundary"], pow_limit) and final <= c["boundary"]):
        return 2
    if not below and c["full_mix"] != c["claimed_mix"]:
        return 1
    return 0


# ------------------------------------------------------------------------------- hb_verdict
def _flip(mix: bytes, byte: int) -> bytes:
    m = bytearray(mix)
    m[byte] ^= 0x01
    return bytes(m)


def _verdict_cases(core, params, cp: int, rng: random.Random) -> list:
    pow_limit = int.from_bytes(params.pow_limit, "little")
    top = pow_limit >> 240  # 0x00ff (mainnet style) or 0x7fff (regtest)
    # a boundary inside the limit whose first two and last bytes all have room for +-1
    B = (((top // 2) & 0x7F7F) << 240) | (rng.getrandbits(232) << 8) | 0x80
    above_cp = cp + 7  # full final and mix decide
    cases = []

    def add(note, kind=0, height=above_cp, boundary=B, mo_final=None, full_final=None, mix_byte=None, bits=None):
        claimed = rng.randbytes(32)
        c = {"note": note, "kind": kind, "height": height, "boundary": boundary, "claimed_mix": claimed,
             "full_mix": claimed if mix_byte is None else _flip(claimed, mix_byte),
             "mo_final": rng.getrandbits(256) if mo_final is None else mo_final,
             "full_final": rng.getrandbits(256) if full_final is None else full_final,
             "bits": rng.getrandbits(32) if bits is None else bits}
        cases.append(c)

    hi_low = (((B >> 240) - 1) << 240) | ((1 << 240) - 1)  # one less in the top bytes, all ones below
    lo_high = ((B >> 240) + 1) << 240                      # one more in the top bytes, zeros below
    finals = [("equal", B), ("lsb+1", B + 1), ("lsb-1", B - 1), ("msb+1", B + (1 << 248)), ("byte1+1", B + (1 << 240)),
              ("byte1-1", B - (1 << 240)), ("top-1,rest-ones", hi_low), ("top+1,rest-zero", lo_high), ("zero", 0)]
    if B >> 248:
        finals.append(("msb-1", B - (1 << 248)))
    for name, f in finals:
        add("full final " + name, full_final=f)  # the mix-only final is random: almost surely above B
        if cp >= 0:
            add("mix-only final " + name, height=cp, mo_final=f, mix_byte=5)
    # the boundary against the pow limit
    add("boundary == limit", boundary=pow_limit, full_final=rng.getrandbits(200))
    add("boundary == limit == final", boundary=pow_limit, full_final=pow_limit)
    add("boundary == limit + 1", boundary=pow_limit + 1, full_final=rng.getrandbits(200))
    add("boundary top byte + 1", boundary=pow_limit + (1 << 248), full_final=0)
    add("boundary all ones", boundary=M256, full_final=0)
    add("zero boundary, final 0", boundary=0, full_final=0, mo_final=0)
    add("zero boundary, final 1", boundary=0, full_final=1, mo_final=1)
    if cp >= 0:
        add("zero boundary below the checkpoint", boundary=0, full_final=0, mo_final=0, height=cp)
    # the mix
    for byte in (0, 3, 28, 31):  # word 0 only (both ends of it), word 7 only
        add("mix differs in byte %d" % byte, full_final=B - 1, mix_byte=byte)
    add("mix differs and high-hash", full_final=B + 1, mix_byte=0)
    add("mix differs, boundary above limit", boundary=pow_limit + 1, full_final=0, mix_byte=31)
    # the checkpoint: which final decides, and whether the mix is looked at
    for h in sorted({max(cp - 1, 0), max(cp, 0), cp + 1, 0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF}):
        add("h %d: mix-only passes, full fails" % h, height=h, mo_final=B - 1, full_final=B + 1)
        add("h %d: mix-only fails, full passes" % h, height=h, mo_final=B + 1, full_final=B - 1)
        add("h %d: both pass, mix differs" % h, height=h, mo_final=B, full_final=B, mix_byte=17)
        add("h %d: mix-only passes, full fails, mix differs" % h, height=h, mo_final=B, full_final=B + 1, mix_byte=17)
    # other kinds: 1 and 3 are the host's (255), an Equihash row's code is hb_eq_scatter's
    for kind in (1, 2, 3):
        add("kind %d" % kind, kind=kind, full_final=0, mo_final=0)
    # cases with an nBits form, cross-checked with the host's CheckProofOfWork below
    for bits in (0x1D00FFFF, 0x1B123456, 0x2000FFFF, 0x20010000, 0x207FFFFF, 0x21008000, 0x03123456, 0x02008000):
        t, neg, ovf = decode_compact(bits)
        assert (t, neg, ovf) == tuple(core.set_compact(bits)) and not neg and not ovf
        for f in (t, t + 1, t - 1):
            add("nBits %08x" % bits, boundary=t, full_final=f, bits=bits)
            want = core.check_proof_of_work(f.to_bytes(32, "little"), bits, params)
            assert (verdict(cases[-1], cp, pow_limit) == 0) == want == check_pow(f, bits, pow_limit)
    return cases


def _launch_verdict(gpu, params, cp, rows_cases, before, after, rng):
    """hb_verdict over rows [before, before + len(rows_cases)) of a batch with unrelated rows on
    both sides: (codes of the whole batch, the rest of the output buffer)."""
    import torch

    from nodexa_chain_core_amd.ops import runtime

    count = len(rows_cases)
    n = before + count + after
    rows = np.frombuffer(rng.randbytes(n * ROW), np.uint8).reshape(n, ROW).copy()
    mo = np.frombuffer(rng.randbytes(n * 128), np.uint8).reshape(n, 128).copy()
    full = np.frombuffer(rng.randbytes(n * 64), np.uint8).reshape(n, 64).copy()
    kinds = np.zeros(n, np.uint8)  # the rows outside the range are KawPow rows too: they must stay untouched
    for k, c in enumerate(rows_cases):
        i = before + k
        kinds[i] = c["kind"]
        rows[i, 72:76] = np.frombuffer(c["bits"].to_bytes(4, "little"), np.uint8)
        rows[i, 76:80] = np.frombuffer(c["height"].to_bytes(4, "little"), np.uint8)
        mo[i, 32:64] = np.frombuffer(c["mo_final"].to_bytes(32, "big"), np.uint8)
        mo[i, 64:96] = np.frombuffer(c["boundary"].to_bytes(32, "big"), np.uint8)
        mo[i, 96:128] = np.frombuffer(c["claimed_mix"], np.uint8)
        full[i, 0:32] = np.frombuffer(c["full_mix"], np.uint8)
        full[i, 32:64] = np.frombuffer(c["full_final"].to_bytes(32, "big"), np.uint8)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)  # noqa: E731
    d_rows, d_kinds, d_mo = dev(rows.reshape(-1)), dev(kinds), dev(mo.reshape(-1))
    d_full = dev(full.reshape(-1).view(np.int32))
    d_jobs = torch.zeros(n * 48, dtype=torch.uint8, device=gpu)
    d_jprog = torch.zeros(n, dtype=torch.int32, device=gpu)
    d_eq = torch.zeros(8, dtype=torch.int32, device=gpu)
    d_out = torch.full((n * 33 + 64,), MARK, dtype=torch.uint8, device=gpu)
    runtime.hip().launch_header_batch(
        runtime.static_kernel("header_batch", "hb_verdict"), 1, d_rows.data_ptr(), d_kinds.data_ptr(), d_mo.data_ptr(),
        d_jobs.data_ptr(), d_jprog.data_ptr(), d_full.data_ptr(), d_out.data_ptr(), d_eq.data_ptr(), d_eq.data_ptr(),
        d_eq.data_ptr(), n, 0, before, count, EPOCH, cp, bytes(params.pow_limit), runtime.current_stream_handle())
    out = d_out.cpu().numpy()
    assert not d_jobs.any() and not d_jprog.any()
    return out[:n], out[n:]


@pytest.mark.parametrize("net", ["test", "regtest"])
@pytest.mark.parametrize("cp", [-1, 0, 1000])
def test_hb_verdict_cases(core, gpu, net, cp):
    """Every constructed case once, as the middle rows of a larger batch."""
    params = core.make_chain_params(net)
    pow_limit = int.from_bytes(params.pow_limit, "little")
    rng = random.Random("verdict/%s/%d" % (net, cp))
    cases = _verdict_cases(core, params, cp, rng)
    before, after = 19, 300
    codes, rest = _launch_verdict(gpu, params, cp, cases, before, after, rng)
    want = [verdict(c, cp, pow_limit) for c in cases]
    assert {0, 1, 2, 255, None} == set(want)
    got = [int(x) for x in codes[before:before + len(cases)]]
    bad = [(c["note"], g, w) for c, g, w in zip(cases, got, want) if g != (MARK if w is None else w)]
    assert not bad, bad
    assert (codes[:before] == MARK).all() and (codes[before + len(cases):] == MARK).all()
    assert (rest == MARK).all()  # the block hashes are hb_jobs' to write


@pytest.mark.parametrize("count", [1, 255, 257])
def test_hb_verdict_counts(core, gpu, count):
    """Block tails: the cases repeated over `count` rows from a random start, nothing else written."""
    params = core.make_chain_params("test")
    pow_limit = int.from_bytes(params.pow_limit, "little")
    cp = 1000
    rng = random.Random("verdict-count/%d" % count)
    cases = _verdict_cases(core, params, cp, rng)
    start = rng.randrange(len(cases))
    chosen = [cases[(start + k) % len(cases)] for k in range(count)]
    codes, rest = _launch_verdict(gpu, params, cp, chosen, 3, 70, rng)
    want = [verdict(c, cp, pow_limit) for c in chosen]
    assert [int(x) for x in codes[3:3 + count]] == [MARK if w is None else w for w in want]
    assert (codes[:3] == MARK).all() and (codes[3 + count:] == MARK).all() and (rest == MARK).all()


# ------------------------------------------------------------------------------- hb_eq_scatter
EQ_BITS = (0x1D00FFFF, 0x207FFFFF, 0x03123456, 0x01003456, 0x04923456, 0x23000001, 0x2200FFFF, 0x20800000,
           0x01803456, 0x00FFFFFF, 0x02008000, 0x03000000, 0x20800001,
           0x2100FFFF, 0x220000FF, 0x22000100, 0xFF000001)


def _eq_cases(core, params) -> list:
    """(nBits, hash as an integer) pairs: each value's decoded target, one above and one below where
    they exist, hash 0 for a zero target; plus the pow-limit compact and a value just above it."""
    pow_limit = int.from_bytes(params.pow_limit, "little")
    limit_compact = core.dgw_constants(params)["compacts"][0]
    size, word = limit_compact >> 24, limit_compact & 0x007FFFFF
    over = (size << 24 | word + 1) if word + 1 < 0x00800000 else ((size + 1) << 24 | 0x008000)
    assert decode_compact(over)[0] > pow_limit >= decode_compact(limit_compact)[0]
    cases = []
    for bits in EQ_BITS + (limit_compact, over):
        target, negative, overflow = decode_compact(bits)
        assert (target, negative, overflow) == tuple(core.set_compact(bits))
        for h in (target, target + 1, target - 1):
            if 0 <= h <= M256:
                cases.append((bits, h))
                assert check_pow(h, bits, pow_limit) == core.check_proof_of_work(h.to_bytes(32, "little"), bits, params)
    assert {check_pow(h, b, pow_limit) for b, h in cases} == {True, False}
    return cases


@pytest.mark.parametrize("net", ["test", "regtest"])
@pytest.mark.parametrize("eq_n", [1, 256, 300])
def test_hb_eq_scatter(core, gpu, net, eq_n):
    import torch

    from nodexa_chain_core_amd.ops import runtime

    params = core.make_chain_params(net)
    pow_limit = int.from_bytes(params.pow_limit, "little")
    rng = random.Random("eq/%s/%d" % (net, eq_n))
    cases = _eq_cases(core, params)
    assert eq_n == 1 or len(cases) <= eq_n // 2
    start = rng.randrange(len(cases)) if eq_n == 1 else 0
    n = eq_n + 45
    index = rng.sample(range(n), eq_n)  # an injection into the batch, in no order
    rows = np.frombuffer(rng.randbytes(n * ROW), np.uint8).reshape(n, ROW).copy()
    hashes = np.zeros((eq_n, 32), np.uint8)
    verdicts = np.zeros(eq_n, np.uint32)
    want = np.full(n, MARK, np.uint8)
    for k in range(eq_n):
        bits, h = cases[(start + k) % len(cases)]
        if k >= len(cases):  # the second and later passes over the cases: some with a bad solution
            verdicts[k] = rng.choice((0, 0, 1, 7, 0x100, 0x80000000))
        rows[index[k], 72:76] = np.frombuffer(bits.to_bytes(4, "little"), np.uint8)
        hashes[k] = np.frombuffer(h.to_bytes(32, "little"), np.uint8)  # uint256 storage order
        want[index[k]] = 3 if verdicts[k] else (0 if check_pow(h, bits, pow_limit) else 2)
    if eq_n > 1:
        assert {0, 2, 3} <= set(want.tolist())
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu)  # noqa: E731
    d_rows = dev(rows.reshape(-1))
    d_index = dev(np.array(index, np.uint32).view(np.int32))
    d_verdict = dev(verdicts.view(np.int32))
    d_hash = dev(hashes.reshape(-1))
    d_kinds = torch.full((n,), 2, dtype=torch.uint8, device=gpu)
    d_mo = torch.zeros(n * 128, dtype=torch.uint8, device=gpu)
    d_jobs = torch.zeros(n * 48, dtype=torch.uint8, device=gpu)
    d_jprog = torch.zeros(n, dtype=torch.int32, device=gpu)
    d_full = torch.zeros(n * 16, dtype=torch.int32, device=gpu)
    d_out = torch.full((n * 33 + 64,), MARK, dtype=torch.uint8, device=gpu)
    # first / count are not hb_eq_scatter's: the pipeline passes 0, 0
    runtime.hip().launch_header_batch(
        runtime.static_kernel("header_batch", "hb_eq_scatter"), 2, d_rows.data_ptr(), d_kinds.data_ptr(),
        d_mo.data_ptr(), d_jobs.data_ptr(), d_jprog.data_ptr(), d_full.data_ptr(), d_out.data_ptr(), d_index.data_ptr(),
        d_verdict.data_ptr(), d_hash.data_ptr(), n, eq_n, 0, 0, EPOCH, -1, bytes(params.pow_limit),
        runtime.current_stream_handle())
    out = d_out.cpu().numpy()
    bad = [(hex(cases[(start + k) % len(cases)][0]), hex(cases[(start + k) % len(cases)][1]), int(verdicts[k]),
            int(out[index[k]]), int(want[index[k]])) for k in range(eq_n) if out[index[k]] != want[index[k]]]
    assert not bad, bad[:8]
    assert np.array_equal(out[:n], want)  # rows that are not mapped keep their marker
    want_hashes = np.full((n, 32), MARK, np.uint8)
    want_hashes[index] = hashes
    assert np.array_equal(out[n:n * 33].reshape(n, 32), want_hashes)
    assert (out[n * 33:] == MARK).all()
