"""Independent oracle for the Equihash(200,9) verifiers' tests: the solution rules on Python
integers and hashlib, written away from everything that is under test.

Three pieces of the project decide whether a solution is valid: the CPU golden model
(csrc/pow/equihash.cpp equihash_verify) and the two gfx950 kernels of hip/kernels/equihash.hip
(eq_verify over packed solutions, eq_verify_slots over the solver's output). Their tests compare
them with this module, never with each other. It imports nothing from the project.

* `leaf`, `failed_rules`, `expected_code`: the rules, all of them evaluated for every solution
  (a verifier stops at the first or reports the highest; the oracle says everything that is wrong);
* `pack` / `unpack`: 512 x 21-bit big-endian indices <-> 1344 bytes;
* `load_fixtures`: tests/data/equihash_adversarial.json (written by tools/equihash_gen_adversarial.py);
* `derived_cases`: the corruptions that can be made from a valid solution, shared by the CPU and
  the GPU test;
* `rules_of`: `failed_rules` memoised, so each (input, solution) is judged once per test run.
"""
import hashlib
import json
import os
import random
import struct

N = 200
K = 9
DIGIT = N // (K + 1)              # 20 collision bits per level
LEAVES = 1 << (DIGIT + 1)         # 2^21 leaf indices
SOL_INDICES = 1 << K              # 512
INDEX_BITS = DIGIT + 1            # 21
SOL_BYTES = SOL_INDICES * INDEX_BITS // 8   # 1344
PERSON = b"ZcashPoW" + struct.pack("<I", N) + struct.pack("<I", K)

# the kernels' verdict numbering (hip/kernels/kernel_params.h EQ_V_*); a solution that breaks
# several rules reports the largest
CODES = {"collision": 1, "order": 2, "duplicate": 3, "nonzero": 4}
CODE_OK = 0
CODE_EMPTY = 255

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "equihash_adversarial.json")

# the single-bit-defect classes the fixture file must hold: (level, bit). Level l < 9: a bit of the
# level's own digit, checked by that level's rule alone; level 9: a bit of the last 40.
DEFECT_CLASSES = (
    [(l, 20 * (l - 1)) for l in range(1, 9)] + [(l, 20 * l - 1) for l in range(1, 9)]      # digit edges
    + [(2, 31), (2, 32), (4, 63), (4, 64), (5, 95), (5, 96), (7, 127), (7, 128)]           # 32-bit word edges
    + [(9, 160), (9, 191), (9, 192), (9, 199)])                                            # root
# input lengths with a valid fixture: the leaf counter le32(i >> 1) follows the input, so it lands at
# byte 4 of a 64-bit message word (108), across two words (117: its low 24 bits in the first, and
# zeros in the second since i >> 1 < 2^20; 119: 8 bits in the first and 12 live bits in the second),
# and in the last word (124). 112 is the production length.
VALID_LENGTHS = (108, 112, 117, 119, 124)


# ------------------------------------------------------------------ the rules
def leaf(inp: bytes, i: int) -> int:
    """Leaf i as a 200-bit number (bit 0 of the rules = its most significant bit)."""
    d = hashlib.blake2b(inp + struct.pack("<I", i >> 1), digest_size=50, person=PERSON).digest()
    return int.from_bytes(d[25 * (i & 1):25 * (i & 1) + 25], "big")


def failed_rules(inp: bytes, indices) -> set:
    """Every rule the solution breaks: 'collision' (a node of level 1..8 whose XOR has a set bit
    among its first 20 * level), 'nonzero' (the root's XOR is not zero), 'order' (a node whose left
    subtree does not start with a smaller index than its right one), 'duplicate' (a repeated
    index). Empty = valid."""
    indices = [int(v) for v in indices]
    if len(indices) != SOL_INDICES or any(not 0 <= v < LEAVES for v in indices):
        raise ValueError("a solution is 512 indices below 2^21")
    failed = set()
    if len(set(indices)) != len(indices):
        failed.add("duplicate")
    xors = [leaf(inp, v) for v in indices]
    for level in range(1, K + 1):
        span = 1 << level  # leaves under one node of this level
        nxt = []
        for j in range(SOL_INDICES >> level):
            x = xors[2 * j] ^ xors[2 * j + 1]
            if level < K:
                if x >> (N - DIGIT * level):
                    failed.add("collision")
            elif x:
                failed.add("nonzero")
            if not indices[j * span] < indices[j * span + span // 2]:
                failed.add("order")
            nxt.append(x)
        xors = nxt
    return failed


def level_xors(inp: bytes, indices, level: int) -> list:
    """The 200-bit XOR of every node of `level` (512 >> level of them)."""
    xors = [leaf(inp, int(v)) for v in indices]
    for _ in range(level):
        xors = [xors[2 * j] ^ xors[2 * j + 1] for j in range(len(xors) // 2)]
    return xors


def order_failures(indices) -> list:
    """(level, node) of every node whose left subtree does not start with the smaller index."""
    return [(level, j) for level in range(1, K + 1) for j in range(SOL_INDICES >> level)
            if not indices[j << level] < indices[(j << level) + (1 << (level - 1))]]


def expected_code(failed: set) -> int:
    return max((CODES[r] for r in failed), default=CODE_OK)


_memo: dict = {}


def rules_of(inp: bytes, indices) -> frozenset:
    key = (bytes(inp), tuple(int(v) for v in indices))
    if key not in _memo:
        _memo[key] = frozenset(failed_rules(*key))
    return _memo[key]


# ------------------------------------------------------------------ packing
def pack(indices) -> bytes:
    v = 0
    for x in indices:
        if not 0 <= int(x) < LEAVES:
            raise ValueError("index out of range")
        v = (v << INDEX_BITS) | int(x)
    return v.to_bytes(len(indices) * INDEX_BITS // 8, "big")


def unpack(sol: bytes) -> list:
    n = len(sol) * 8 // INDEX_BITS
    v = int.from_bytes(sol, "big") >> (len(sol) * 8 - n * INDEX_BITS)
    return [(v >> (INDEX_BITS * (n - 1 - i))) & (LEAVES - 1) for i in range(n)]


# ------------------------------------------------------------------ fixtures and derived cases
class Case:
    """One (input, solution) pair put before a verifier. `cls` names how it was made, `rules` is the
    oracle's verdict of now, `recorded` what the fixture file stored (None for a derived case)."""

    def __init__(self, name, inp, indices, cls, rules=None, level=None, bit=None):
        self.name, self.inp, self.indices, self.cls = name, bytes(inp), [int(v) for v in indices], cls
        self.recorded, self.level, self.bit = rules, level, bit

    @property
    def rules(self) -> frozenset:
        return rules_of(self.inp, self.indices)

    @property
    def code(self) -> int:
        return expected_code(self.rules)

    @property
    def packed(self) -> bytes:
        return pack(self.indices)

    def __repr__(self):
        return f"<{self.name} len={len(self.inp)}>"


def load_fixtures(path: str = FIXTURES) -> list:
    with open(path) as f:
        doc = json.load(f)
    out = []
    for k, e in enumerate(doc["entries"]):
        sol = bytes.fromhex(e["solution"])
        if len(sol) != SOL_BYTES:
            raise ValueError(f"entry {k}: a packed solution is {SOL_BYTES} bytes")
        name = e["class"] + (f"-l{e['level']}-b{e['bit']}" if "bit" in e else "") + f"#{k}"
        out.append(Case(name, bytes.fromhex(e["input"]), unpack(sol), e["class"], frozenset(e["rules"]),
                        e.get("level"), e.get("bit")))
    return out


def canonical(indices) -> list:
    """The same tree with every node's children put in order (smaller first index on the left)."""
    s = list(indices)
    sz = 1
    while sz < len(s):
        for a in range(0, len(s), 2 * sz):
            if s[a] > s[a + sz]:
                s[a:a + sz], s[a + sz:a + 2 * sz] = s[a + sz:a + 2 * sz], s[a:a + sz]
        sz *= 2
    return s


def swap_children(indices, level: int, j: int) -> list:
    """Node j of `level` (it spans 2^level leaves) with its two subtrees exchanged."""
    span = 1 << level
    a, h = j * span, span // 2
    s = list(indices)
    s[a:a + h], s[a + h:a + span] = s[a + h:a + span], s[a:a + h]
    return s


def derived_cases(fixtures) -> list:
    """The corruptions made at test time from the valid solutions of the fixture file.

    * order-*: the children of one node swapped (levels 1..9; first, second, middle and last node):
      no XOR changes, the oracle gives exactly {order}. A swap under a left child (even node) also
      moves its ancestors' first index and usually fails an ancestor's test too; under a right child
      (odd node: the second and the last) the swapped node's own test is the only one that fails
      (`order_failures`), which is what shows an order test missing at one level;
    * dup-*: L+L for the left half L and three seeded permutations of it: the root XOR is zero, so
      'nonzero' cannot hide a duplicate pass that never fires (expected code 3);
    * graft-*, flip-*, input-*: large corruptions (a subtree taken from the other solution of the same
      input and put back in order, one flipped index bit, one changed input byte).
    """
    valid = [c for c in fixtures if c.cls == "valid"]
    out = []
    for v in valid:
        tag = f"{len(v.inp)}.{v.name.split('#')[1]}"
        for level in range(1, K + 1):
            n = SOL_INDICES >> level
            for j in sorted({0, min(1, n - 1), n // 2, n - 1}):
                out.append(Case(f"order-l{level}-n{j}@{tag}", v.inp, swap_children(v.indices, level, j), "order"))
        half = v.indices[:SOL_INDICES // 2]
        out.append(Case(f"dup-LL@{tag}", v.inp, half + half, "dup"))
        for seed in range(3):
            s = half + half
            random.Random(0xE9 + seed).shuffle(s)
            out.append(Case(f"dup-perm{seed}@{tag}", v.inp, s, "dup"))
        for k, b in ((0, 0), (255, 20), (511, 7)):
            s = list(v.indices)
            s[k] ^= 1 << b
            out.append(Case(f"flip-i{k}-b{b}@{tag}", v.inp, s, "flip"))
        for pos in (0, len(v.inp) - 1):
            inp = bytearray(v.inp)
            inp[pos] ^= 0x01
            out.append(Case(f"input-byte{pos}@{tag}", bytes(inp), v.indices, "input"))
    # a subtree of 2^(l-1) leaves from the second solution of the same input, children put back in order
    by_input: dict = {}
    for v in valid:
        by_input.setdefault(v.inp, []).append(v)
    for inp, vs in by_input.items():
        if len(vs) < 2:
            continue
        a, b = vs[0], vs[1]
        for level in range(1, K + 1):
            w = 1 << (level - 1)
            at = (SOL_INDICES - w) if level % 2 else 0   # alternate the two ends of the tree
            s = list(a.indices)
            s[at:at + w] = b.indices[at:at + w]
            out.append(Case(f"graft-l{level}@{len(inp)}", inp, canonical(s), "graft"))
    return out
