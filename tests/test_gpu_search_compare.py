"""The 256-bit target compares of x16r_hits (hip/kernels/x16r.hip: little-endian words, walked from
the most significant) and ethash_final_batch (hip/kernels/ethash_hashimoto.hip: byte-swapped words)
hit at their edges: the target on the smallest hash of the range, one under it, and one unit over
and under it in each of the eight 32-bit words, so that the walk is decided at every position it
can be. Then the limits around them: X16rSearcher's clamp at 2^32, ethash_search's hit list past
its capacity and its nonces across 2^64.

Expected values come from the host's hashes (`core.x16r` / `core.x16rv2` / `core.ethash_hash`) and
Python integers (tests/search_oracle.py)."""
import inspect
import random

import pytest

from search_oracle import M64, le256_be, le256_le, words_plain

pytestmark = pytest.mark.gpu

WORDS = range(8)


# ------------------------------------------------------------------ X16R
X_START, X_COUNT, X_WINDOW = 1000, 600, 256  # two full windows and a partial one


def x16r_header(hdr: bytes, nonce: int) -> bytes:
    return hdr[:76] + (nonce & 0xFFFFFFFF).to_bytes(4, "little")


@pytest.fixture(scope="module")
def xsearcher(gpu):
    from nodexa_chain_core_amd.ops.x16r import X16rSearcher

    return X16rSearcher(0, window=X_WINDOW)


_x16r_host: dict = {}


@pytest.fixture(params=[False, True], ids=["x16r", "x16rv2"])
def xcase(request, core):
    """(v2, header, host hashes of the 600 nonces, index of the smallest as a little-endian number)."""
    v2 = request.param
    if v2 not in _x16r_host:
        hdr = random.Random(4).randbytes(80)
        fn = core.x16rv2 if v2 else core.x16r
        hs = [fn(h, h[4:36]) for h in (x16r_header(hdr, X_START + i) for i in range(X_COUNT))]
        j = min(range(X_COUNT), key=lambda i: int.from_bytes(hs[i], "little"))
        assert j >= X_WINDOW          # the hit is not in the first window
        assert words_plain(hs[j], "little")
        _x16r_host[v2] = (v2, hdr, hs, j)
    return _x16r_host[v2]


def le_target(value: int) -> bytes:
    return value.to_bytes(32, "little")


def test_x16r_target_on_the_smallest_hash(xsearcher, xcase):
    v2, hdr, hs, j = xcase
    H = int.from_bytes(hs[j], "little")
    assert [i for i in range(X_COUNT) if le256_le(hs[i], le_target(H))] == [j]
    assert xsearcher.search(hdr, v2, le_target(H), X_START, X_COUNT) == ((X_START + j, hs[j]), j + 1)
    assert not any(le256_le(h, le_target(H - 1)) for h in hs)
    assert xsearcher.search(hdr, v2, le_target(H - 1), X_START, X_COUNT) == (None, X_COUNT)


@pytest.mark.parametrize("k", WORDS)
def test_x16r_word_walk_decided_at_word(xsearcher, xcase, k):
    """Target and hash differ in word k alone: by +1 the hash qualifies, by -1 it does not."""
    v2, hdr, hs, j = xcase
    H = int.from_bytes(hs[j], "little")
    over, under = le_target(H + (1 << 32 * k)), le_target(H - (1 << 32 * k))
    assert [i for i in range(X_COUNT) if le256_le(hs[i], over)] == [j]
    assert xsearcher.search(hdr, v2, over, X_START, X_COUNT) == ((X_START + j, hs[j]), j + 1)
    assert not any(le256_le(h, under) for h in hs)
    assert xsearcher.search(hdr, v2, under, X_START, X_COUNT) == (None, X_COUNT)


def test_x16r_clamp_at_2_32(core, xsearcher, xcase):
    v2, hdr, _hs, _j = xcase
    start = 0xFFFFFF00
    assert xsearcher.search(hdr, v2, bytes(32), start, 1000) == (None, (1 << 32) - start)
    h = x16r_header(hdr, start)
    first = (core.x16rv2 if v2 else core.x16r)(h, h[4:36])
    assert xsearcher.search(hdr, v2, b"\xff" * 32, start, 1000) == ((start, first), 1)


# ------------------------------------------------------------------ classic Ethash
E_START, E_COUNT, E_WINDOW = 5000, 200, 64
E_HEADER = random.Random(1).randbytes(32)


@pytest.fixture(scope="module")
def epoch0(gpu, core):
    import torch

    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

    e = DeviceEpoch(0, device=0, ctx=core.get_epoch_context(0))
    e.build()
    torch.cuda.synchronize()
    assert e.l1_matches()
    return e


@pytest.fixture(scope="module")
def ecase(core, epoch0):
    """(host (final, mix) of the 200 nonces, index of the smallest final as a big-endian number)."""
    fm = [core.ethash_hash(epoch0.ctx, E_HEADER, E_START + i) for i in range(E_COUNT)]
    j = min(range(E_COUNT), key=lambda i: fm[i][0])
    assert j >= E_WINDOW and words_plain(fm[j][0], "big")
    return fm, j


def be_target(value: int) -> bytes:
    return value.to_bytes(32, "big")


def esearch(epoch0, boundary):
    return epoch0.ethash_search(E_HEADER, boundary, E_START, E_COUNT, window=E_WINDOW)


def test_ethash_boundary_on_the_smallest_hash(epoch0, ecase):
    fm, j = ecase
    F = int.from_bytes(fm[j][0], "big")
    assert [i for i in range(E_COUNT) if le256_be(fm[i][0], be_target(F))] == [j]
    assert esearch(epoch0, be_target(F)) == (E_START + j, *fm[j])
    assert not any(le256_be(f, be_target(F - 1)) for f, _ in fm)
    assert esearch(epoch0, be_target(F - 1)) is None


@pytest.mark.parametrize("k", WORDS)
def test_ethash_word_walk_decided_at_word(epoch0, ecase, k):
    """Boundary and final differ in one 32-bit word alone; k = 0 is the least significant, bytes
    28..31 of the final, the word the kernel byte-swaps and looks at last."""
    fm, j = ecase
    F = int.from_bytes(fm[j][0], "big")
    over, under = be_target(F + (1 << 32 * k)), be_target(F - (1 << 32 * k))
    assert [i for i in range(E_COUNT) if le256_be(fm[i][0], over)] == [j]
    assert esearch(epoch0, over) == (E_START + j, *fm[j])
    assert not any(le256_be(f, under) for f, _ in fm)
    assert esearch(epoch0, under) is None


def test_ethash_hit_list_overflow(core, epoch0):
    """More hits in one window than the hit list holds: the lowest index may not be among the listed
    ones, and the answer is still the first nonce that qualifies on the host. First with every job
    a hit, then with three in four and the first nonce not one of them."""
    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

    max_hits = inspect.signature(DeviceEpoch.ethash_search).parameters["max_hits"].default
    n = 2 * max_hits
    got = epoch0.ethash_search(E_HEADER, b"\xff" * 32, E_START, n, window=n)
    assert got == (E_START, *core.ethash_hash(epoch0.ctx, E_HEADER, E_START))
    boundary = b"\xc0" + bytes(31)  # 3 n / 4 = 1.5 max_hits hits expected, sigma 0.02 max_hits: the list overflows
    start = next(x for x in range(E_START, E_START + 64) if not le256_be(core.ethash_hash(epoch0.ctx, E_HEADER, x)[0], boundary))
    first = next(x for x in range(start, start + 64) if le256_be(core.ethash_hash(epoch0.ctx, E_HEADER, x)[0], boundary))
    assert first > start
    got = epoch0.ethash_search(E_HEADER, boundary, start, n, window=n)
    assert got == (first, *core.ethash_hash(epoch0.ctx, E_HEADER, first))


def test_ethash_nonces_across_2_64(core, epoch0):
    start, n = (1 << 64) - 10, 64
    hh = random.Random(101).randbytes(32)
    fm = [core.ethash_hash(epoch0.ctx, hh, (start + i) & M64) for i in range(n)]
    j = min(range(n), key=lambda i: fm[i][0])
    assert j >= 10  # the hit lies past the wrap
    assert [i for i in range(n) if le256_be(fm[i][0], fm[j][0])] == [j]
    assert epoch0.ethash_search(hh, fm[j][0], start, n, window=n) == ((start + j) & M64, *fm[j])
