"""secp256k1 and ECDSA verification in plain Python integers, written from the definitions and
sharing nothing with the project's C++ / HIP code, plus the deterministic vector builders of
tests/test_secp_edges.py: the edge set of 256-bit values, the fold classifiers that tell which
rare branch of f_mul / s_mul a pair takes, the point lists, and the whole-signature vectors with
the raw verdict each must get from the batch verifier."""
import functools
import random
from typing import NamedTuple

from test_secp_batch import _der

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
C = 2**32 + 977          # 2^256 mod p
NC = 2**256 - N          # 2^256 mod n
M256 = 2**256 - 1


# ---------------------------------------------------------------- the curve y^2 = x^3 + 7 over p
# A point is (x, y) or None for the point at infinity.
def on_curve(pt) -> bool:
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def double(a):
    if a is None or a[1] == 0:
        return None
    lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    x = (lam * lam - 2 * a[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        return double(a) if a[1] == b[1] else None
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def mul(k: int, a):
    k %= N
    r = None
    while k:
        if k & 1:
            r = add(r, a)
        a = double(a)
        k >>= 1
    return r


def sqrt_p(a: int):
    """The root a^((p+1)/4) of a (p = 3 mod 4), or None when a is not a square."""
    a %= P
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a else None


def lift_x(x: int):
    """The curve point with this x < p and the root sqrt_p gives, or None."""
    y = sqrt_p(x ** 3 + 7)
    return None if y is None else (x, y)


def ecdsa_verify(Q, r: int, s: int, z: int) -> bool:
    """Textbook ECDSA: Q a curve point other than infinity, z the message as an integer."""
    if Q is None or not on_curve(Q):
        return False
    if not (1 <= r <= N - 1 and 1 <= s <= N - 1):
        return False
    w = pow(s, -1, N)
    R = add(mul(z * w, G), mul(r * w, Q))
    return R is not None and R[0] % N == r


# ---------------------------------------------------------------- serialisation
def ser_key(Q, kind: int = 2) -> bytes:
    """kind 2: compressed (02/03 by parity), 4: uncompressed, 6: hybrid (06/07 by parity)."""
    x, y = Q
    if kind == 2:
        return bytes([2 + (y & 1)]) + x.to_bytes(32, "big")
    if kind == 4:
        return b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")
    assert kind == 6
    return bytes([6 + (y & 1)]) + x.to_bytes(32, "big") + y.to_bytes(32, "big")


def parse_key(pub: bytes):
    """A serialised key as a curve point, or None when it is not one: 33 bytes 02/03, 65 bytes
    04/06/07, coordinates below p, on the curve, hybrid prefix parity equal to y's."""
    if len(pub) == 33 and pub[0] in (2, 3):
        x = int.from_bytes(pub[1:], "big")
        if x >= P:
            return None
        pt = lift_x(x)
        if pt is None:
            return None
        return pt if (pt[1] & 1) == (pub[0] & 1) else neg(pt)
    if len(pub) == 65 and pub[0] in (4, 6, 7):
        x, y = int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big")
        if x >= P or y >= P or not on_curve((x, y)):
            return None
        if pub[0] != 4 and (y & 1) != (pub[0] & 1):
            return None
        return x, y
    return None


def verify_bytes(pub: bytes, r: int, s: int, msg: bytes) -> bool:
    return ecdsa_verify(parse_key(pub), r, s, int.from_bytes(msg, "big"))


# ---------------------------------------------------------------- the edge set of 256-bit values
@functools.lru_cache(maxsize=None)
def edge_values() -> tuple[tuple[int, ...], tuple[int, ...]]:
    """(the 134 edge values, 32 seeded random values)."""
    e = set()
    for base in (0, P, N, 2**256, 2**255, 2**128, 2**224, 2**32, C, P // 2, N // 2, (P + 1) // 2, P - N):
        for d in range(-3, 4):
            if 0 <= base + d < 2**256:
                e.add(base + d)
    for k in range(0, 256, 16):
        e.update((1 << k, (1 << k) - 1, P - (1 << k), N - (1 << k)))
    e.add(int("ffffffff00000000" * 4, 16))
    e.add(int("00000000ffffffff" * 4, 16))
    rng = random.Random(20250256)
    rnd = []
    while len(rnd) < 32:
        v = rng.getrandbits(256)
        if v not in e and v not in rnd:
            rnd.append(v)
    return tuple(sorted(e)), tuple(rnd)


def classify_f_mul(a: int, b: int) -> tuple[int, frozenset]:
    """The folds of secp256k1_device.hpp f_mul on whole integers: (result, rare branches taken).
    "k2" is the carry out of the second fold, "geq" the final subtraction of p."""
    t = a * b
    s = (t & M256) + (t >> 256) * C      # fold 1: r = low 256 bits, c = the rest (< 2^34)
    s = (s & M256) + (s >> 256) * C      # fold 2: f_add_pc(r, c)
    r, k2 = s & M256, s >> 256
    taken = set()
    if k2:
        taken.add("k2")
        r += k2 * C
        assert r <= M256
    if r >= P:
        taken.add("geq")
        r -= P
    return r, frozenset(taken)


def classify_s_mul(a: int, b: int) -> tuple[int, frozenset]:
    """The folds of s_mul: "carry" is the carry out of the third fold, "sub1" / "sub2" the two
    conditional subtractions of n that follow."""
    t = a * b
    u = (t & M256) + (t >> 256) * NC     # fold 1
    w = (u & M256) + (u >> 256) * NC     # fold 2
    s = (w & M256) + (w >> 256) * NC     # fold 3
    r, c = s & M256, s >> 256
    taken = set()
    if c:
        taken.add("carry")
        r = (r + NC) & M256
    for name in ("sub1", "sub2"):
        if r >= N:
            taken.add(name)
            r = (r + NC) & M256
    return r, frozenset(taken)


# ---------------------------------------------------------------- points for j_double / j_add_affine
@functools.lru_cache(maxsize=None)
def probe_points() -> tuple:
    """G, 2G, 3G, the points with x = 1 and x = n + 2, three random multiples of G."""
    rng = random.Random(77)
    pts = [G, double(G), mul(3, G), lift_x(1), lift_x(N + 2)]
    pts += [mul(rng.randrange(1, N), G) for _ in range(3)]
    assert all(p is not None and on_curve(p) for p in pts)
    return tuple(pts)


def jacobian_forms(pt, rng) -> list[tuple[int, int, int]]:
    """(x, y, 1) and the representatives (l^2 x, l^3 y, l) for l in 2, p - 1, C and a random one."""
    x, y = pt
    return [(l * l * x % P, l * l * l * y % P, l) for l in (1, 2, P - 1, C, rng.randrange(2, P))]


def affine_of(X: int, Y: int, Z: int):
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


# ---------------------------------------------------------------- whole-signature vectors
class SigVector(NamedTuple):
    name: str
    pub: bytes
    r: int          # as carried by the DER signature (may be out of range on purpose)
    s: int
    msg: bytes
    raw: int        # the verdict the batch verifier itself must give: 1, 0 or 2 (ask the host)
    final: bool     # the answer after the host has settled a 2

    @property
    def sig(self) -> bytes:
        return _der(self.r, self.s)

    @property
    def item(self) -> tuple[bytes, bytes, bytes]:
        return self.pub, self.sig, self.msg


def _msg(z: int) -> bytes:
    return z.to_bytes(32, "big")


def _from_u(Q, draw):
    """A signature valid for Q with chosen u1 = z/s and u2 = r/s: R = u1 G + u2 Q, r = x(R) mod n,
    s = r/u2, z = u1 s. `draw` is called again until s is low: the packer negates a high s, which
    flips the signs of u1 and u2 and with them the path through the verifier."""
    while True:
        u1, u2 = draw()
        R = add(mul(u1, G), mul(u2, Q))
        if R is None:
            continue
        r = R[0] % N
        s = r * pow(u2, -1, N) % N
        if r and 0 < s <= N // 2:
            return r, s, u1 * s % N, R


def _with_s(d: int, s: int, rng):
    """A signature (r, s, z) valid for the key d G with this very s: z = s k - r d."""
    k = rng.randrange(1, N)
    r = mul(k, G)[0] % N
    return r, s, (s * k - r * d) % N


@functools.lru_cache(maxsize=None)
def signature_vectors() -> tuple[SigVector, ...]:
    rng = random.Random(3)
    out: list[SigVector] = []

    def put(name, pub, r, s, msg, raw, final):
        out.append(SigVector(name, pub, r, s, msg if isinstance(msg, bytes) else _msg(msg), raw, final))

    d = rng.randrange(1, N)
    Q = mul(d, G)
    di = pow(d, -1, N)

    # The window loop over u2 leaves u2 Q = +-nb G in the accumulator and the comb's first row adds
    # nb G to it: P + P or P + (-P) inside an addition, which the kernel must hand to the host.
    # No vector is hunted for the window loop or the 3Q setup, which cannot get there: the loop
    # adds t Q (t = 1, 2, 3) to 4k Q where 4k + t is a prefix of u2, so 4 <= 4k < 4k + t <= u2 < n
    # and 4k = +-t (mod n) has no solution; 2Q = +-Q would need 3Q = O or Q = O in a group of
    # prime order n.
    for nb, sign, what in ((5, 1, "doubling"), (15, 1, "doubling"), (5, -1, "inverse"), (15, -1, "inverse")):
        r, s, z, _ = _from_u(Q, lambda: ((rng.randrange(1, N) & ~15) | nb, sign * nb * di % N))
        put(f"{what} in the comb nb={nb}", ser_key(Q), r, s, z, 2, True)

    # R = u1 G + u2 Q = O: z = -r d
    r, s = rng.randrange(1, N), rng.randrange(1, N // 2)
    put("R at infinity", ser_key(Q), r, s, -r * d % N, 2, False)

    # x(R) >= n: the first x above n on the curve is n + 2, so r = 2 and the verifier has to
    # compare against r + n as well
    xr = N + 1
    while lift_x(xr) is None:
        xr += 1
    assert xr == N + 2
    R = lift_x(xr)

    def key_for(u1, u2):
        return mul(pow(u2, -1, N), add(R, neg(mul(u1, G))))

    while True:
        u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
        s = 2 * pow(u2, -1, N) % N
        if 0 < s <= N // 2:
            break
    Qc, z = key_for(u1, u2), u1 * s % N
    put("x(R) >= n, key compressed", ser_key(Qc), 2, s, z, 1, True)
    put("x(R) >= n, key uncompressed", ser_key(Qc, 4), 2, s, z, 1, True)
    put("x(R) >= n, wrong r", ser_key(Qc), 3, s, z, 0, False)
    put("x(R) >= n, DER carries r + n", ser_key(Qc), 2 + N, s, z, 0, False)

    # key coordinates at and past p
    Q1 = lift_x(1)
    r, s, z, _ = _from_u(Q1, lambda: (rng.randrange(1, N), rng.randrange(1, N)))
    put("key x = 1", ser_key(Q1), r, s, z, 1, True)
    put("key x = 1 uncompressed", ser_key(Q1, 4), r, s, z, 1, True)
    par = bytes([2 + (Q1[1] & 1)])
    put("key x = p + 1, an alias of x = 1", par + (P + 1).to_bytes(32, "big"), r, s, z, 0, False)
    put("key x = p + 1 uncompressed", b"\x04" + (P + 1).to_bytes(32, "big") + Q1[1].to_bytes(32, "big"), r, s, z, 0, False)
    put("key x = p", par + P.to_bytes(32, "big"), r, s, z, 0, False)
    put("key x = p - 1", par + (P - 1).to_bytes(32, "big"), r, s, z, 0, False)
    xo = 2
    while lift_x(xo) is not None:
        xo += 1
    put(f"key x = {xo}, off the curve", par + xo.to_bytes(32, "big"), r, s, z, 0, False)

    # the message: z = 0 (the comb adds nothing), bytes that reduce mod n
    r, s, z, _ = _from_u(Q, lambda: (0, rng.randrange(1, N)))
    assert z == 0
    put("z = 0", ser_key(Q), r, s, z, 1, True)
    for name, zb in (("message bytes n", N), ("message bytes 2^256 - 1", M256)):
        while True:
            k = rng.randrange(1, N)
            r = mul(k, G)[0] % N
            s = pow(k, -1, N) * (zb + r * d) % N
            if r and 0 < s <= N // 2:
                break
        put(name, ser_key(Q), r, s, zb, 1, True)

    # s at its ends and around n/2; the packer turns a high s into n - s
    r, s, z = _with_s(d, 1, rng)
    put("s = 1", ser_key(Q), r, 1, z, 1, True)
    put("s = n - 1, normalised to 1", ser_key(Q), r, N - 1, z, 1, True)
    r, s, z = _with_s(d, N // 2, rng)
    put("s = n // 2", ser_key(Q), r, N // 2, z, 1, True)
    put("s = n // 2 + 1", ser_key(Q), r, N // 2 + 1, z, 1, True)
    put("r = 0", ser_key(Q), 0, s, z, 0, False)
    put("s = 0", ser_key(Q), r, 0, z, 0, False)
    put("r = n", ser_key(Q), N, s, z, 0, False)
    put("s = n", ser_key(Q), r, N, z, 0, False)

    # sparse scalars: the top windows of u2 empty, empty nibbles at the comb's first and last row
    for u2 in (1, 2, 3):
        r, s, z, _ = _from_u(Q, lambda: (rng.randrange(1, N), u2))
        put(f"u2 = {u2}", ser_key(Q), r, s, z, 1, True)
    r, s, z, _ = _from_u(Q, lambda: (rng.getrandbits(252) & ~15, rng.randrange(1, N)))
    put("u1 with empty first and last nibble", ser_key(Q), r, s, z, 1, True)

    # key encodings
    r, s, z, _ = _from_u(Q, lambda: (rng.randrange(1, N), rng.randrange(1, N)))
    x, y = Q
    put("uncompressed key", ser_key(Q, 4), r, s, z, 1, True)
    put("uncompressed key, y negated", ser_key(neg(Q), 4), r, s, z, 0, False)
    put("uncompressed key, y + 1", ser_key((x, (y + 1) % P), 4), r, s, z, 0, False)
    put("hybrid key, parity matches", ser_key(Q, 6), r, s, z, 1, True)
    put("hybrid key of -Q, parity matches", ser_key(neg(Q), 6), r, s, z, 0, False)
    put("hybrid key, parity mismatched", bytes([ser_key(Q, 6)[0] ^ 1]) + ser_key(Q, 6)[1:], r, s, z, 0, False)
    put("key of length 0", b"", r, s, z, 0, False)
    put("key of length 32", ser_key(Q)[1:], r, s, z, 0, False)
    put("key of length 64", ser_key(Q, 4)[1:], r, s, z, 0, False)
    put("key prefix 05, 33 bytes", b"\x05" + ser_key(Q)[1:], r, s, z, 0, False)
    put("key prefix 05, 65 bytes", b"\x05" + ser_key(Q, 4)[1:], r, s, z, 0, False)
    return tuple(out)
