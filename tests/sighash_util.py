"""Shared by test_sighash_pack.py (CPU) and test_gpu_sighash.py: seeded legacy transactions at the
edges of the gathered signature hash, and the arena / job table built from them in Python (the
layout of csrc/chain/sighash.hpp, written out independently of the native packer)."""
import itertools
import random
import struct

JOB = struct.Struct("<10I")  # off[4], len[4], out_index, kind

RESIDUES = (0, 1, 55, 56, 63)           # preimage length mod 64: the SHA-256 padding edges
CODE_LENS = (0, 1, 25, 252, 253, 520)   # compact-size widening of the script code at 253
HASH_TYPES = (0x01, 0x00, 0x04, 0x21, 0x7c)
PLAIN_OPS = bytes(range(0x51, 0x61)) + b"\x76\x87\x88\xa9\xac"  # no pushes, no OP_CODESEPARATOR


def plain_code(rng, n):
    return bytes(rng.choice(PLAIN_OPS) for _ in range(n))


def make_tx(core, rng, n_in, out_spk_lens=(25,)):
    tx = core.Transaction()
    tx.version = rng.choice((1, 2))
    vins = []
    for _ in range(n_in):
        vin = core.TxIn()
        op = core.OutPoint()
        op.hash, op.n = rng.randbytes(32), rng.randrange(4)
        vin.prevout = op
        vin.sequence = rng.choice((0xffffffff, 0xfffffffe, rng.randrange(1 << 32)))
        vin.script_sig = rng.randbytes(rng.randrange(0, 8))  # must not reach the hash
        vins.append(vin)
    tx.vin = vins
    tx.vout = [core.TxOut(rng.randrange(1, 10**9), rng.randbytes(n)) for n in out_spk_lens]
    tx.lock_time = rng.choice((0, rng.randrange(1 << 32)))
    return tx.serialize(False)


def preimage_len(core, raw, code):
    return len(core.sighash_template(raw)[0]) - 1 + len(core.sighash_script_code(code)) + 4


def tx_with_residue(core, rng, n_in, code, residue):
    """A transaction whose input preimages (for `code`) have length = residue mod 64."""
    base = preimage_len(core, make_tx(core, rng, n_in, (30,)), code)
    spk = 30 + (residue - base) % 64   # 30..93: the output script's compact size stays one byte
    raw = make_tx(core, rng, n_in, (spk,))
    assert preimage_len(core, raw, code) % 64 == residue
    return raw


def edge_cases(core, seed=1, big_vin=253):
    """[(raw tx, input index, script code, hash type)]: about 600 inputs, every one eligible for
    the gathered hash. Ends with every input of one `big_vin`-input transaction."""
    rng = random.Random(seed)
    cases = []
    hts = itertools.cycle(HASH_TYPES)
    # the padding edges, at every code length
    for residue in RESIDUES:
        for n in CODE_LENS:
            code = plain_code(rng, n)
            raw = tx_with_residue(core, rng, 3, code, residue)
            for i in (0, 2):
                cases.append((raw, i, code, next(hts)))
    # the vin-count edges (compact size of vin widens at 253), spliced at the first and the last input
    for n_in in (1, 2, 252, 253):
        raw = make_tx(core, rng, n_in, (25, 23))
        for n in CODE_LENS:
            for i in sorted({0, n_in - 1}):
                cases.append((raw, i, plain_code(rng, n), next(hts)))
    # every hash type of the ALL form on one input, and a full 32-bit type
    raw = make_tx(core, rng, 2)
    for ht in HASH_TYPES + (0x7fffff01, -0x7fffffff):
        cases.append((raw, 1, plain_code(rng, 25), ht))
    # OP_CODESEPARATORs (removed, the length prefix follows) and a truncated push after one (the
    # op walk stops there: the prefix overstates the bytes)
    for code in (b"\x51\xab\x52\xab\xab\x53", b"\xab", b"\x76\xab\x4c\x05\x01\x02", b"\xab\x4e\xff",
                 b"\x02\xab\xab\x51\xab", plain_code(rng, 251) + b"\xab" + plain_code(rng, 2)):
        for residue in (0, 55):
            cases.append((tx_with_residue(core, rng, 2, code, residue), 1, code, next(hts)))
    # random fill
    while len(cases) < 600 - big_vin:
        n_in = rng.randrange(1, 12)
        raw = make_tx(core, rng, n_in, tuple(rng.randrange(0, 80) for _ in range(rng.randrange(0, 4))))
        for i in range(n_in):
            cases.append((raw, i, plain_code(rng, rng.choice((0, 25, 25, 35, 71, 105))), next(hts)))
    # one long transaction: adjacent lanes walk one long shared template
    raw = make_tx(core, rng, big_vin, (25, 25))
    code = plain_code(rng, 25)
    for i in range(big_vin):
        cases.append((raw, i, code, 0x01))
    return cases


def pack_cases(core, cases, out_index=None, kind=0):
    """-> (arena, job table): one template per distinct transaction, then code and hash type per case."""
    arena = bytearray()
    placed = {}
    jobs = bytearray()
    for k, (raw, i, code, ht) in enumerate(cases):
        if raw not in placed:
            t, offs = core.sighash_template(raw)
            placed[raw] = (len(arena), len(t), offs)
            arena += t
        base, tlen, offs = placed[raw]
        emitted = core.sighash_script_code(code)
        at = len(arena)
        arena += emitted + struct.pack("<i", ht)
        jobs += JOB.pack(base, at, base + offs[i] + 1, at + len(emitted),
                         offs[i], len(emitted), tlen - offs[i] - 1, 4,
                         k if out_index is None else out_index[k], kind)
    return bytes(arena), bytes(jobs)


def host_hashes(core, cases):
    return b"".join(core.signature_hash(code, raw, i, ht, 0, 0) for raw, i, code, ht in cases)
