"""An independent DarkGravityWave for the tests: plain Python integers, no limbs, no reciprocals.

`dgw` follows the reference's DarkGravityWave (src/pow.cpp:18-102) over a raw (nTime, nBits)
series; `expected_bits_oracle` adds the per-header contract of hip/kernels/dgw.hip (`dgw_batch`).
The host model (csrc/chain/pow_rules.cpp `dgw_average`) and the kernel are twins that share the
limb loop and the ceil(2^64 / d) reciprocal, so both are compared with this file instead of with
each other: tests/test_dgw_series.py (host) and tests/test_gpu_dgw_edges.py (kernel).

The second half builds the adversarial series both test files use, each from a seeded
`random.Random`: windows that cross 2^31 and 2^32 in nTime, total spans on every edge of the
1/3x..3x clamp (and negative ones), and six families of nBits."""
import functools
import random
import struct

PAST = 180
WINDOW = PAST + 1  # a window's 180 blocks and the header after them
M256 = (1 << 256) - 1


def set_compact(bits: int) -> int:
    """arith_uint256::SetCompact, the magnitude only: the sign bit is dropped, a left shift wraps at 2^256."""
    size, word = bits >> 24, bits & 0x007FFFFF
    if size <= 3:
        return word >> 8 * (3 - size)
    return (word << 8 * (size - 3)) & M256


def get_compact(v: int) -> int:
    """arith_uint256::GetCompact(false)."""
    size = (v.bit_length() + 7) // 8
    c = v << 8 * (3 - size) if size <= 3 else (v >> 8 * (size - 3)) & 0xFFFFFFFF
    if c & 0x00800000:
        c >>= 8
        size += 1
    return c | size << 24


def limit(constants, which: int) -> int:
    """Limit `which` (0 pow, 1 KawPow, 2 Equihash with a null one already replaced by the pow limit)
    of core.dgw_constants as an integer."""
    return sum(w << 32 * k for k, w in enumerate(constants["limits"][8 * which:8 * which + 8]))


def dgw_path(constants, times, bits, j: int, next_time: int):
    """(nBits, path) of the header after series entry j, whose nTime is next_time; path is
    "equihash" / "kawpow" for the two bootstraps and "computed" otherwise."""
    if j < PAST - 1:
        raise ValueError("DGW window shorter than 180 blocks")
    avg = 0
    kawpow_blocks = equihash_blocks = 0
    for n in range(1, PAST + 1):  # newest first
        k = j - (n - 1)
        t = set_compact(bits[k])
        avg = t if n == 1 else ((avg * n + t) & M256) // (n + 1)
        kawpow_blocks += times[k] >= constants["kawpow_time"]
        equihash_blocks += times[k] >= constants["equihash_time"]
    if next_time >= constants["equihash_time"] and equihash_blocks != PAST:
        return get_compact(limit(constants, 2)), "equihash"
    if next_time >= constants["kawpow_time"] and kawpow_blocks != PAST:
        return get_compact(limit(constants, 1)), "kawpow"
    span = constants["target_timespan"]
    actual = times[j] - times[j - (PAST - 1)]  # signed: the series holds u32 values
    actual = max(span // 3, min(span * 3, actual))
    new = ((avg * (actual & 0xFFFFFFFF)) & M256) // span
    return get_compact(min(new, limit(constants, 0))), "computed"


def dgw(constants, times, bits, j: int, next_time: int) -> int:
    return dgw_path(constants, times, bits, j, next_time)[0]


def expected_bits_oracle(constants, times, bits, a: int, n: int, base_height: int) -> list:
    """What dgw_batch must write for the n headers that follow `a` ancestors in the series, the
    parent of the first at height base_height: 0 = not decided here (the host's serial path)."""
    out = []
    for i in range(n):
        last_height = base_height + i
        j = a - 1 + i
        if last_height + 1 < constants["dgw_activation_block"]:
            out.append(0)
        elif last_height < PAST:
            out.append(get_compact(limit(constants, 0)))
        elif j < PAST - 1:
            out.append(0)
        else:
            out.append(dgw(constants, times, bits, j, times[j + 1]))
    return out


def pack(values) -> bytes:
    return struct.pack("<%dI" % len(values), *values)


# ---------------------------------------------------------------------------------- series
T0S = (5000, 0x7FFFFF00, 0xFFFE0000)  # plain, across 2^31, up against 2^32
FAMILIES = ("random32", "exponents", "wrapping", "realistic", "tiny", "renormalise")
_EXPONENTS = (0, 1, 2, 3, 4, 29, 30, 31, 32, 33, 34, 35, 36, 255)
_WRAPPING = (0x207FFFFF, 0x2100FFFF, 0x22000001, 0x1D00FFFF, 0x1E00FFFF)
_TINY = (0x03000001, 0x02008000, 0x01003456, 0x04800000, 0x00FFFFFF, 0x03123456)


def spans(target_timespan: int):
    """Total window spans: on, one inside and one outside each clamp edge, negative, zero, huge."""
    t = target_timespan
    return (-500, 0, 1, t // 3 - 1, t // 3, t // 3 + 1, t, 3 * t - 1, 3 * t, 3 * t + 1, 100000)


def _window_bits(rng: random.Random, family: str) -> list:
    if family == "random32":
        return [rng.getrandbits(32) for _ in range(WINDOW)]
    if family == "exponents":
        return [rng.choice(_EXPONENTS) << 24 | rng.getrandbits(24) for _ in range(WINDOW)]
    if family == "wrapping":
        return [rng.choice(_WRAPPING) for _ in range(WINDOW)]
    if family == "realistic":
        return [0x1B00FFFF + rng.randint(-300, 300) for _ in range(WINDOW)]
    if family == "tiny":
        return [rng.choice(_TINY) for _ in range(WINDOW)]
    if family == "renormalise":
        return [0x1C7FFFFF] * WINDOW
    raise ValueError(family)


def _window_times(rng: random.Random, t0: int, span: int) -> list:
    """181 u32 times: entry 0 at t0, entry 179 at t0 + span exactly, the ones between interpolated
    with +-1 jitter (so some run backwards), the header after the window 60 s later."""
    t = [t0 + span * k // (PAST - 1) + (rng.randint(-1, 1) if 0 < k < PAST - 1 else 0) for k in range(PAST)]
    t.append(t[-1] + 60)
    return [x & 0xFFFFFFFF for x in t]


@functools.lru_cache(maxsize=None)
def family_series(family: str, t0: int, target_timespan: int, seed: int = 2024):
    """(times, bits) tuples: one 181-entry block per span of `spans`, concatenated. Block w is
    entries [181 w, 181 w + 180]; the header at 181 w + 180 sees exactly block w's window."""
    rng = random.Random("%s/%d/%d/%d" % (family, t0, target_timespan, seed))
    times, bits = [], []
    for span in spans(target_timespan):
        times += _window_times(rng, t0, span)
        bits += _window_bits(rng, family)
    return tuple(times), tuple(bits)


def smooth_series(length: int, t0: int = 1_700_000_000, seed: int = 7):
    """A calm chain: ~61 s blocks with a few seconds of jitter, nBits wandering around 0x1b00ffff."""
    rng = random.Random(seed)
    times, bits = [t0], [0x1B00FFFF]
    for _ in range(length - 1):
        times.append(times[-1] + 61 + rng.randint(-5, 5))
        bits.append(0x1B00FFFF + rng.randint(-300, 300))
    return times, bits
