#!/usr/bin/env python3
"""Writes tests/data/equihash_adversarial.json: Equihash(200,9) solutions that a verifier with one
small defect would judge wrongly, mined on the CPU (NumPy + hashlib; deterministic, fixed nonces).

    python tools/equihash_gen_adversarial.py [--out PATH] [--cross-check]

Runs once (a few minutes, ~2 GB); the output is committed and the suite never runs this. The rule
set stored with every entry is the verdict of tests/equihash_oracle.py, which the tests recompute.

Contents
* valid: two solutions of one 112-byte input, one each for inputs of 108, 117, 119 and 124 bytes
  (the leaf counter lands at byte 4 of a message word, across two words with its live bits in the
  first only and in both, and in the last word).
* defect (level l, bit b): a solution whose only fault is bit b of the XOR of every level-l node.
  b lies in level l's own digit [20(l-1), 20l), so no lower level looks at it, and both children
  of every level-(l+1) node carry it, so it cancels above: only the level-l rule, at the right
  width, rejects the solution. At the root (l = 9) b is one of the last 40 bits. Such a solution
  cannot be made by editing a valid one. It is mined: a Wagner pass whose level l pairs rows that
  differ in exactly bit b of the digit (instead of rows equal in it), and that is ordinary above.
* duplicate: a candidate of an ordinary pass whose XORs and order are right and whose only fault is
  a repeated leaf, when the first nonce yields one.

--cross-check also asks the project's own CPU solver (core.equihash_solve_cpu) for the valid ones.
"""
import argparse
import hashlib
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import equihash_oracle as O  # noqa: E402

NEIGHBOURS = 9      # each row is paired with its next 9 neighbours in sorted order
MAX_NONCES = 12


def make_input(length: int, nonce: int) -> bytes:
    return bytes((37 * i + 11) & 0xFF for i in range(length - 4)) + struct.pack("<I", nonce)


def leaf_digits(inp: bytes) -> np.ndarray:
    """All 2^21 leaves as rows of ten 20-bit digits (uint32), digit 0 = bits 0..19."""
    base = hashlib.blake2b(inp, digest_size=50, person=O.PERSON)
    chunks = []
    for g in range(O.LEAVES // 2):
        h = base.copy()
        h.update(struct.pack("<I", g))
        chunks.append(h.digest())
    b = np.frombuffer(b"".join(chunks), dtype=np.uint8).reshape(O.LEAVES, 5, 5).astype(np.uint32)
    even = (b[:, :, 0] << 12) | (b[:, :, 1] << 4) | (b[:, :, 2] >> 4)
    odd = ((b[:, :, 2] & 15) << 16) | (b[:, :, 3] << 8) | b[:, :, 4]
    return np.stack([even, odd], axis=2).reshape(O.LEAVES, 10)


def pairs(key: np.ndarray, mask: int = 0):
    """Row pairs (a, b) equal in `key`, or with `mask` (one bit): equal but for exactly that bit."""
    bit = None
    if mask:
        bit = (key & key.dtype.type(mask)) != 0
        key = key & key.dtype.type(~mask & ((1 << 8 * key.itemsize) - 1))
    order = np.argsort(key, kind="stable")
    ks = key[order]
    bs = bit[order] if mask else None
    A, B = [], []
    for j in range(1, NEIGHBOURS + 1):
        m = ks[:-j] == ks[j:]
        if mask:
            m &= bs[:-j] != bs[j:]
        A.append(order[:-j][m])
        B.append(order[j:][m])
    return np.concatenate(A), np.concatenate(B)


def collide(rows: np.ndarray, level: int, mask: int = 0):
    """Level 1..8: the XOR rows of all pairs that collide on digit level-1, and their parents.
    Pairs whose whole remainder is zero are dropped (they only lead to repeated leaves)."""
    a, b = pairs(rows[:, level - 1], mask)
    x = rows[a] ^ rows[b]
    keep = x[:, level:].any(axis=1)
    return x[keep], (a[keep], b[keep])


def final_pairs(rows: np.ndarray, mask: int = 0):
    key = (rows[:, 8].astype(np.uint64) << np.uint64(20)) | rows[:, 9].astype(np.uint64)
    return pairs(key, mask)


def expand(refs, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(C, 512) leaf indices of the candidates (a[i], b[i]) of level-8 rows; refs[l] = parents of level l."""
    cur = np.stack([a, b], axis=1)
    for level in range(8, 0, -1):
        ra, rb = refs[level]
        cur = np.stack([ra[cur], rb[cur]], axis=2).reshape(len(cur), -1)
    # canonical order: every node's left subtree starts with the smaller index
    sz = 1
    while sz < 512:
        v = cur.reshape(len(cur), 512 // (2 * sz), 2, sz)
        swap = v[:, :, 0, 0] > v[:, :, 1, 0]
        v[swap] = v[swap][:, ::-1, :]
        cur = v.reshape(len(cur), 512)
        sz *= 2
    return cur


def distinct(cands: np.ndarray) -> np.ndarray:
    s = np.sort(cands, axis=1)
    return (s[:, 1:] != s[:, :-1]).all(axis=1)


class Pass:
    """An ordinary Wagner pass over one input, every level kept so a defect run can branch off."""

    def __init__(self, inp: bytes):
        self.inp = inp
        self.rows = [leaf_digits(inp)]
        self.refs = [None]
        for level in range(1, 9):
            x, ref = collide(self.rows[-1], level)
            self.rows.append(x)
            self.refs.append(ref)
        a, b = final_pairs(self.rows[8])
        self.cands = expand(self.refs, a, b) if len(a) else np.zeros((0, 512), dtype=np.int64)
        self.ok = distinct(self.cands) if len(self.cands) else np.zeros(0, dtype=bool)

    def valid(self) -> list:
        out = []
        for c in self.cands[self.ok].tolist():
            if c not in out and not O.failed_rules(self.inp, c):
                out.append(c)
        return out

    def duplicate_only(self, look: int = 64):
        for c in self.cands[~self.ok][:look].tolist():
            if O.failed_rules(self.inp, c) == {"duplicate"}:
                return c
        return None

    def defect(self, level: int, bit: int):
        """A solution whose only fault is `bit` at `level`, or None if this input has none."""
        refs = list(self.refs)
        if level < 9:
            rows, refs[level] = collide(self.rows[level - 1], level, 1 << (20 * level - 1 - bit))
            for l in range(level + 1, 9):
                rows, refs[l] = collide(rows, l)
            a, b = final_pairs(rows)
        else:
            a, b = final_pairs(self.rows[8], 1 << (199 - bit))
        if not len(a):
            return None
        cands = expand(refs, a, b)
        want = {"collision"} if level < 9 else {"nonzero"}
        for c in cands[distinct(cands)].tolist():
            if O.failed_rules(self.inp, c) == want:
                return c
        return None


def entry(cls: str, inp: bytes, sol: list, **more) -> dict:
    e = {"class": cls, "input": inp.hex(), "solution": O.pack(sol).hex(), "rules": sorted(O.failed_rules(inp, sol))}
    e.update(more)
    return e


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=O.FIXTURES)
    ap.add_argument("--cross-check", action="store_true", help="compare the valid solutions with core.equihash_solve_cpu")
    args = ap.parse_args()
    t0 = time.time()

    def log(*a):
        print(f"[{time.time() - t0:6.0f}s]", *a, file=sys.stderr, flush=True)

    valid: dict = {}        # input length -> entries
    defects: dict = {}      # (level, bit) -> entry
    bonus = None
    missing = list(O.DEFECT_CLASSES)
    for nonce in range(MAX_NONCES):
        if not missing and 112 in valid:
            break
        inp = make_input(112, nonce)
        p = Pass(inp)
        sols = p.valid()
        log(f"len 112 nonce {nonce}: rows {[len(r) for r in p.rows]}, {len(p.cands)} candidates, {len(sols)} valid")
        if 112 not in valid and len(sols) >= 2:
            valid[112] = [entry("valid", inp, s, nonce=nonce) for s in sols[:2]]
        if nonce == 0:
            d = p.duplicate_only()
            if d is not None:
                bonus = entry("duplicate", inp, d, nonce=nonce)
        for level, bit in list(missing):
            s = p.defect(level, bit)
            log(f"  defect level {level} bit {bit}: {'found' if s else 'none'}")
            if s:
                defects[(level, bit)] = entry("defect", inp, s, level=level, bit=bit, nonce=nonce)
                missing.remove((level, bit))
        del p
    if missing or 112 not in valid:
        log("not found:", missing, "" if 112 in valid else "two valid solutions of one input")
        return 1
    for length in (n for n in O.VALID_LENGTHS if n != 112):
        for nonce in range(MAX_NONCES):
            inp = make_input(length, nonce)
            sols = Pass(inp).valid()
            log(f"len {length} nonce {nonce}: {len(sols)} valid")
            if sols:
                valid[length] = [entry("valid", inp, sols[0], nonce=nonce)]
                break
        else:
            return 1

    entries = [e for length in sorted(valid) for e in valid[length]]
    entries += [defects[c] for c in O.DEFECT_CLASSES]
    if bonus:
        entries.append(bonus)
    for e in entries:
        want = {"valid": [], "duplicate": ["duplicate"], "defect": ["nonzero"] if e.get("level") == 9 else ["collision"]}
        assert e["rules"] == want[e["class"]], e
    if args.cross_check:
        sys.path.insert(0, ROOT)
        from nodexa_chain_core_amd import _build
        _build.build_core()
        from nodexa_chain_core_amd import _core
        prm = _core.EquihashParams(200, 9)
        for e in entries:
            if e["class"] == "valid":
                got, _ = _core.equihash_solve_cpu(prm, bytes.fromhex(e["input"]), 64, 0)
                assert O.unpack(bytes.fromhex(e["solution"])) in got, e["input"]
        log("cross-check: every valid solution is one of core.equihash_solve_cpu's")

    with open(args.out, "w") as f:
        f.write('{"about": "Equihash(200,9) adversarial solutions; written by tools/equihash_gen_adversarial.py, '
                'rules = verdict of tests/equihash_oracle.py",\n "entries": [\n')
        f.write(",\n".join("  " + json.dumps(e, sort_keys=True) for e in entries))
        f.write("\n ]}\n")
    log(f"wrote {len(entries)} entries to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
