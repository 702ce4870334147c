"""Shared by test_sighash_forms.py (CPU) and test_gpu_sighash_forms.py: seeded signatures of every
form of both signature versions at the edges of the gathered hash, and an arena / segment table /
job table built from them in Python. The layout here is this file's own (it differs from the native
packer's on purpose: other splits, other sharing), so the model and the kernel are checked against
tables the native packer never produced; the expected hashes come from sighash_ref."""
import random
import struct

import sighash_ref as R
import sighash_util as U

SEG = struct.Struct("<2I")   # off, len
JOB = struct.Struct("<4I")   # first_seg, n_seg, out_index, kind

# (sigversion, representative hash type) of the 12 forms
LEGACY_TYPES = (0x01, 0x02, 0x03, 0x81, 0x82, 0x83)
FORMS = [(sv, ht) for sv in (0, 1) for ht in LEGACY_TYPES]
FORM_NAMES = {0x01: "all", 0x02: "none", 0x03: "single", 0x81: "all|acp", 0x82: "none|acp", 0x83: "single|acp"}
# a full 32-bit and a negative type in each base class (ALL, NONE, SINGLE)
WIDE_TYPES = (0x7fffff01, 0x7fffff02, 0x7fffff03, -0x7fffffff, -0x7ffffffe, -0x7ffffffd, 0x7fffff83, -0x7fffff7e)
# sighash_util.edge_cases' OP_CODESEPARATOR scripts: separators removed, and a truncated push after one
CODESEP_CODES = (b"\x51\xab\x52\xab\xab\x53", b"\xab", b"\x76\xab\x4c\x05\x01\x02", b"\xab\x4e\xff",
                 b"\x02\xab\xab\x51\xab")
BIG_AMOUNT = 0x4123456789abcdef   # top byte set


def form_name(ht):
    base, acp = ht & 0x1f, bool(ht & 0x80)
    return ("none" if base == 2 else "single" if base == 3 else "all") + ("|acp" if acp else "")


def is_constant_one(case):
    """Legacy SINGLE without a matching output: nothing to hash, the host writes z = 1."""
    raw, i, _, ht, _, sv = case
    return sv == 0 and (ht & 0x1f) == 3 and i >= len(R.parse_tx(raw)["vout"])


def edge_cases(core, seed=7):
    """[(raw tx, input index, script code, hash type, amount, sigversion)], about 900."""
    rng = random.Random(seed)
    cases = []

    def add(raw, i, code, ht, sv, amount=None):
        cases.append((raw, i, code, ht, rng.randrange(1, 10**12) if amount is None else amount, sv))

    # every form at every padding residue: the code length sets the preimage length
    for sv, ht in FORMS:
        raw = U.make_tx(core, rng, 3, (25, 31, 22))
        base = len(R.preimage(bytes(25), raw, 1, ht, 1, sv))
        for residue in U.RESIDUES:
            add(raw, 1, U.plain_code(rng, 25 + (residue - base) % 64), ht, sv)
    # the code lengths (compact size widens at 253) and the separator scripts, in every form
    raw = U.make_tx(core, rng, 2, (25, 23))
    for sv, ht in FORMS:
        for n in U.CODE_LENS:
            add(raw, 1, U.plain_code(rng, n), ht, sv)
        for code in CODESEP_CODES + (U.plain_code(rng, 251) + b"\xab" + U.plain_code(rng, 2),):
            add(raw, 0, code, ht, sv)
    # the vin-count edges (compact size of vin widens at 253; 1 under ANYONECANPAY), first and last input,
    # with as many outputs as inputs so that SINGLE has its output
    big = {}
    for n_in in (1, 2, 252, 253):
        raw = big[n_in] = U.make_tx(core, rng, n_in, tuple(rng.randrange(0, 6) for _ in range(n_in)))
        for ht in (0x02, 0x03, 0x81, 0x82, 0x83):
            for i in sorted({0, n_in - 1}):
                add(raw, i, U.plain_code(rng, 25), ht, 0)
    # SINGLE along the blank run: empty at input 0, and 251 -> 252 widens the output count's compact size
    for i in (0, 1, 251, 252):
        for ht in (0x03, 0x83):
            add(big[253], i, U.plain_code(rng, 25), ht, 0)
    # SINGLE at the last output, at vout.size() (the constant one: host) and beyond
    raw252 = U.make_tx(core, rng, 253, tuple(rng.randrange(0, 6) for _ in range(252)))
    small = U.make_tx(core, rng, 4, (25, 9))
    for ht in (0x03, 0x83):
        for sv in (0, 1):
            add(raw252, 251, U.plain_code(rng, 25), ht, sv)
            add(raw252, 252, U.plain_code(rng, 25), ht, sv)
            for i in (1, 2, 3):
                add(small, i, U.plain_code(rng, 25), ht, sv)
    # wide and negative hash types in each base class, both versions; an amount with the top byte set
    raw = U.make_tx(core, rng, 3, (25, 25, 25))
    for ht in WIDE_TYPES + U.HASH_TYPES:
        for sv in (0, 1):
            add(raw, 2, U.plain_code(rng, 25), ht, sv)
    add(raw, 1, U.plain_code(rng, 25), 0x01, 1, BIG_AMOUNT)
    add(raw, 1, U.plain_code(rng, 25), 0x83, 1, -1)
    # random fill, forms mixed input by input
    types = LEGACY_TYPES + (0x01, 0x01, 0x00, 0x21)
    while len(cases) < 900:
        n_in = rng.randrange(1, 12)
        raw = U.make_tx(core, rng, n_in, tuple(rng.randrange(0, 80) for _ in range(rng.randrange(0, 5))))
        for i in range(n_in):
            add(raw, i, U.plain_code(rng, rng.choice((0, 25, 25, 35, 71, 105))), rng.choice(types), rng.randrange(2))
    return cases


def ref_hashes(cases):
    return [R.signature_hash(code, raw, i, ht, amount, sv) for raw, i, code, ht, amount, sv in cases]


def host_hashes(core, cases):
    return [core.signature_hash(code, raw, i, ht, amount, sv) for raw, i, code, ht, amount, sv in cases]


class _Tx:
    """One transaction's shared ranges: T (scripts blanked), and the offsets into it."""

    def __init__(self, raw):
        tx = self.tx = R.parse_tx(raw)
        t = struct.pack("<i", tx["version"]) + R.compact_size(len(tx["vin"]))
        self.script_off = []
        for h, n, _, seq in tx["vin"]:
            t += h + struct.pack("<I", n)
            self.script_off.append(len(t))
            t += b"\x00" + struct.pack("<I", seq)
        self.outs_off = len(t)
        t += R.compact_size(len(tx["vout"]))
        self.out_off = []
        for value, spk in tx["vout"]:
            self.out_off.append(len(t))
            t += struct.pack("<q", value) + R.compact_size(len(spk)) + spk
        self.out_off.append(len(t))
        self.t = t + struct.pack("<I", tx["lock_time"])
        z = bytearray(self.t[:self.outs_off])
        for o in self.script_off:
            z[o + 1:o + 5] = bytes(4)
        self.z = bytes(z)
        self.t_at = self.z_at = None


def pack_cases(cases, shift=0, out_index=None, kind=0, with_empty=True):
    """-> (arena, segment table, job table, job_case): one job per case that has something to hash
    (job_case[k] = its case index), then, with `with_empty`, one job of no segments at all
    (job_case = None). `shift` junk bytes precede the arena's content, moving every offset."""
    arena = bytearray(b"\xee" * shift)
    segs, jobs, job_case = bytearray(), bytearray(), []
    txs = {}
    blank_len = 9 * max([i for raw, i, _, ht, _, sv in cases if sv == 0 and (ht & 0x1f) == 3] or [0])
    blank_at = None
    n_segs = 0

    def put(b):
        at = len(arena)
        arena.extend(b)
        return at, len(b)

    for k, case in enumerate(cases):
        raw, i, code, ht, amount, sv = case
        if is_constant_one(case):
            continue
        x = txs.setdefault(raw, _Tx(raw))
        if x.t_at is None:
            x.t_at, _ = put(x.t)
        T = lambda a, b: (x.t_at + a, b - a)  # noqa: E731 — a range of the placed template
        so, end = x.script_off[i], len(x.t)
        base, acp = ht & 0x1f, bool(ht & 0x80)
        lt, ht4 = T(end - 4, end), struct.pack("<i", ht)
        if sv == 0 and base == 3 and blank_at is None:  # SINGLE's blanked outputs, once per arena
            blank_at, _ = put(b"\xff\xff\xff\xff\xff\xff\xff\xff\x00" * (blank_len // 9))
        s = []
        if sv == 1:
            pre = R.preimage(code, x.tx, i, ht, amount, 1)
            if k % 2:
                s.append(put(pre))                                   # one segment
            else:                                                    # the same bytes, what T holds taken from T
                e = R.compact_size(len(code)) + code
                s += [put(pre[:68]), T(so - 36, so), put(e + struct.pack("<q", amount)), T(so + 1, so + 5),
                      put(pre[-40:-8]), lt, put(ht4)]
        else:
            e = R.legacy_script_code(code)
            if base in (2, 3) and not acp:
                if x.z_at is None:
                    x.z_at, _ = put(x.z)
                s.append((x.z_at, so))
                if base == 2:
                    s += [put(e), T(so + 1, so + 5), (x.z_at + so + 5, x.outs_off - so - 5), put(b"\x00"), lt, put(ht4)]
                else:
                    s += [put(e + x.t[so + 1:so + 5]), (x.z_at + so + 5, x.outs_off - so - 5)]
            elif acp:
                s += [put(x.t[:4] + b"\x01"), T(so - 36, so)]
                if base == 2:
                    s += [put(e), T(so + 1, so + 5), put(b"\x00"), lt, put(ht4)]
                elif base == 3:
                    s.append(put(e + x.t[so + 1:so + 5]))
                else:
                    s += [put(e), T(so + 1, so + 5), T(x.outs_off, end), put(ht4)]
            else:
                s += [T(0, so), put(e), T(so + 1, end), put(ht4)]
            if base == 3:
                cs = put(R.compact_size(i + 1))
                if acp:  # the count follows the code and sequence directly: one range
                    s[-1] = (s[-1][0], s[-1][1] + cs[1])
                else:
                    s.append(cs)
                s += [(blank_at, 9 * i), T(x.out_off[i], x.out_off[i + 1]), lt, put(ht4)]
        for off, ln in s:
            segs += SEG.pack(off, ln)
        jobs += JOB.pack(n_segs, len(s), len(job_case) if out_index is None else out_index[len(job_case)], kind)
        n_segs += len(s)
        job_case.append(k)
    if with_empty:
        jobs += JOB.pack(n_segs, 0, len(job_case) if out_index is None else out_index[len(job_case)], kind)
        job_case.append(None)
    return bytes(arena), bytes(segs), bytes(jobs), job_case


def expected_digests(cases, job_case):
    ref = ref_hashes(cases)
    return b"".join(R.sha256d(b"") if k is None else ref[k] for k in job_case)


def seg_counts(segs, jobs):
    """Per job: (n_seg, lengths of its segments)."""
    out = []
    for k in range(len(jobs) // JOB.size):
        first, n, _, _ = JOB.unpack_from(jobs, k * JOB.size)
        out.append((n, [SEG.unpack_from(segs, (first + s) * SEG.size)[1] for s in range(n)]))
    return out
