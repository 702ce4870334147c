"""The integer helpers of tests/search_oracle.py against their big-integer definitions, and the
rule by which KawpowSearcher.search trims a padded launch to its window (no GPU: `launch` and
`collect` are stubs)."""
import random

import pytest

from search_oracle import M64, M256, boundary_for, head64, in_window, le256_be, le256_le, words_plain


def edge_pairs():
    """(a, b) 256-bit integers: random ones, equal ones, one apart, and one apart across a word."""
    rng = random.Random(21)
    vals = [0, 1, M256, M256 - 1, 1 << 255]
    vals += [rng.getrandbits(256) for _ in range(40)]
    vals += [1 << 32 * k for k in range(1, 8)]                  # x - 1 borrows through k words
    vals += [(rng.getrandbits(256) | ((1 << 32 * k) - 1)) & M256 for k in range(1, 8)]  # x + 1 carries into word k
    pairs = [(rng.choice(vals), rng.choice(vals)) for _ in range(200)]
    for v in vals:
        pairs += [(v, v), (v, (v + 1) & M256), (v, (v - 1) & M256), ((v + 1) & M256, v)]
    return pairs


def test_256_bit_compares():
    for a, b in edge_pairs():
        assert le256_be(a.to_bytes(32, "big"), b.to_bytes(32, "big")) == (a <= b), (a, b)
        assert le256_le(a.to_bytes(32, "little"), b.to_bytes(32, "little")) == (a <= b), (a, b)
    # the two byte orders are different numbers
    x, y = bytes([1] + [0] * 31), bytes([0] * 31 + [2])
    assert le256_le(x, y) and not le256_be(x, y)


def test_head64_and_boundary_for():
    rng = random.Random(22)
    for _ in range(50):
        fin = rng.randbytes(32)
        words = [int.from_bytes(fin[4 * k:4 * k + 4], "little") for k in range(8)]  # as the kernel holds them
        bswap = [int.from_bytes(w.to_bytes(4, "little"), "big") for w in words]
        assert head64(fin) == bswap[0] << 32 | bswap[1] == int.from_bytes(fin, "big") >> 192
    for prefix in (0, 1, (1 << 32) - 1, 1 << 32, M64 - 1, M64, rng.getrandbits(64)):
        b = boundary_for(prefix)
        assert len(b) == 32 and head64(b) == prefix
        for a in (prefix - 1, prefix, prefix + 1):  # the full compare is the prefix compare, at and around it
            if 0 <= a <= M64:
                for tail in (bytes(24), b"\xff" * 24, rng.randbytes(24)):
                    assert le256_be(a.to_bytes(8, "big") + tail, b) == (a <= prefix)


def test_words_plain():
    v = int.from_bytes(bytes(range(1, 33)), "big")
    assert words_plain(v.to_bytes(32, "big"), "big") and words_plain(v.to_bytes(32, "little"), "little")
    for k in range(8):
        for bad in (v & ~(0xFFFFFFFF << 32 * k), v | 0xFFFFFFFF << 32 * k):
            assert not words_plain(bad.to_bytes(32, "big"), "big")
        for sign in (1, -1):  # what the property is for: the step changes word k alone
            w = v + sign * (1 << 32 * k)
            assert (w ^ v) >> 32 * (k + 1) == 0 and (w ^ v) & ((1 << 32 * k) - 1) == 0


def test_in_window_across_2_64():
    assert in_window(5, 5, 1) and not in_window(6, 5, 1) and not in_window(4, 5, 1)
    assert not in_window(5, 5, 0)
    start, n = (1 << 64) - 773, 1000
    inside = [start, M64, 0, 1, 226]
    outside = [start - 1, 227, 228, 762, 1 << 63]
    assert all(in_window(x, start, n) for x in inside) and not any(in_window(x, start, n) for x in outside)
    assert [x for x in range(220, 232) if in_window(x, start, n)] == list(range(220, 227))
    rng = random.Random(23)
    for _ in range(200):
        start, n = rng.getrandbits(64), rng.randrange(1, 1 << 20)
        members = {(start + i) & M64 for i in (0, 1, n // 2, n - 1)}
        assert all(in_window(x, start, n) for x in members)
        assert not in_window((start + n) & M64, start, n) and not in_window((start - 1) & M64, start, n)
    assert all(in_window(x, 0, 1 << 64) for x in (0, M64))  # the whole space


# ------------------------------------------------------------------ KawpowSearcher.search
G = 768


def stub_searcher(core, shares):
    """A KawpowSearcher that was never initialised (no device): `launch` records, `collect` answers."""
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher

    s = KawpowSearcher.__new__(KawpowSearcher)
    s.jit_mode, s.granule = "off", G
    s.launched = []
    s.launch = lambda header, start, n, target64: s.launched.append((start, n, target64))
    s.collect = lambda: list(shares)
    return s


def shares_at(nonces, final=bytes(32)):
    from nodexa_chain_core_amd.ops.kawpow import Share

    return [Share(x, bytes(32), final) for x in nonces]


@pytest.mark.parametrize("start, num", [(5000, 1000), ((1 << 32) - 773, 1000), ((1 << 64) - 773, 1000),
                                        ((1 << 64) - 773, 773), ((1 << 64) - 1000, 1000), ((1 << 64) - 1, 2 * G)])
def test_search_trims_to_the_window(core, start, num):
    padded = -(-num // G) * G
    launched_nonces = [start, start + 1, start + num - 1, start + num, start + num + 1, start + padded - 1,
                       M64, 0, 1]  # the last three: around the wrap, wherever the window lies
    launched_nonces = sorted({x & M64 for x in launched_nonces if in_window(x & M64, start, padded)} | {start})
    s = stub_searcher(core, shares_at(launched_nonces))
    got = [x.nonce for x in s.search(bytes(32), start, num, b"\xff" * 32)]
    assert s.launched == [(start, padded, M64)]
    assert got == [x for x in launched_nonces if in_window(x, start, num)]
    assert start in got and (start + num - 1) & M64 in got and (start + num) & M64 not in got


def test_search_applies_the_full_boundary(core):
    boundary = bytes.fromhex("00ff" + "00" * 29 + "80")
    under = (int.from_bytes(boundary, "big") - 1).to_bytes(32, "big")
    over = (int.from_bytes(boundary, "big") + 1).to_bytes(32, "big")
    from nodexa_chain_core_amd.ops.kawpow import Share

    s = stub_searcher(core, [Share(10, bytes(32), under), Share(11, bytes(32), boundary), Share(12, bytes(32), over)])
    assert [x.nonce for x in s.search(bytes(32), 0, G, boundary)] == [10, 11]
    assert s.launched == [(0, G, 0x00FF000000000000)]
