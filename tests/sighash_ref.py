"""SignatureHash in plain Python: the legacy form (CTransactionSignatureSerializer) and BIP143, as
src/script/interpreter.cpp states them. The yardstick of the all-forms tests, independent of the
native code (as secp_ref.py is for the curve): hashlib and struct only."""
import hashlib
import struct

OP_CODESEPARATOR = 0xab
OP_CLORE_ASSET = 0xc0
ONE = b"\x01" + bytes(31)


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


def compact_size(n):
    if n < 253:
        return bytes([n])
    if n <= 0xffff:
        return b"\xfd" + struct.pack("<H", n)
    if n <= 0xffffffff:
        return b"\xfe" + struct.pack("<I", n)
    return b"\xff" + struct.pack("<Q", n)


def _read_compact(b, at):
    n = b[at]
    if n < 253:
        return n, at + 1
    width = {253: 2, 254: 4, 255: 8}[n]
    return int.from_bytes(b[at + 1:at + 1 + width], "little"), at + 1 + width


def parse_tx(raw):
    """-> dict(version, vin=[(prev hash, prev n, script, sequence)], vout=[(value, script)], lock_time);
    a segwit serialisation's witnesses are skipped."""
    version, = struct.unpack_from("<i", raw, 0)
    at = 4
    segwit = raw[at] == 0 and raw[at + 1] != 0
    if segwit:
        at += 2
    n, at = _read_compact(raw, at)
    vin = []
    for _ in range(n):
        h, idx = raw[at:at + 32], struct.unpack_from("<I", raw, at + 32)[0]
        ln, at = _read_compact(raw, at + 36)
        vin.append((h, idx, raw[at:at + ln], struct.unpack_from("<I", raw, at + ln)[0]))
        at += ln + 4
    n, at = _read_compact(raw, at)
    vout = []
    for _ in range(n):
        value, = struct.unpack_from("<q", raw, at)
        ln, at = _read_compact(raw, at + 8)
        vout.append((value, raw[at:at + ln]))
        at += ln
    if segwit:
        for _ in vin:
            items, at = _read_compact(raw, at)
            for _ in range(items):
                ln, at = _read_compact(raw, at)
                at += ln
    lock_time, = struct.unpack_from("<I", raw, at)
    assert at + 4 == len(raw)
    return dict(version=version, vin=vin, vout=vout, lock_time=lock_time)


def _get_op(s, pc):
    """CScript::GetOp2 -> (ok, pc after, opcode): a short push fails with pc after what was read."""
    if pc >= len(s):
        return False, pc, None
    op = s[pc]
    pc += 1
    if op <= 0x4e:
        if op < 0x4c:
            size = op
        else:
            width = {0x4c: 1, 0x4d: 2, 0x4e: 4}[op]
            if len(s) - pc < width:
                return False, pc, None
            size = int.from_bytes(s[pc:pc + width], "little")
            pc += width
        if len(s) - pc < size:
            return False, pc, None
        pc += size
    if op == OP_CLORE_ASSET:
        pc = len(s)
    return True, pc, op


def legacy_script_code(code):
    """SerializeScriptCode: the code without its OP_CODESEPARATORs, with the reference's length
    prefix (size - separators) and its stop at the first op that does not parse."""
    seps, pc = 0, 0
    while True:
        ok, pc, op = _get_op(code, pc)
        if not ok:
            break
        seps += op == OP_CODESEPARATOR
    out = compact_size(len(code) - seps)
    begin = pc = 0
    while True:
        ok, pc, op = _get_op(code, pc)
        if not ok:
            break
        if op == OP_CODESEPARATOR:
            out += code[begin:pc - 1]
            begin = pc
    if begin != len(code):
        out += code[begin:pc]
    return out


def _out(o):
    return struct.pack("<q", o[0]) + compact_size(len(o[1])) + o[1]


def legacy_preimage(code, tx, n_in, hash_type):
    """None where SignatureHash returns the constant one instead of hashing."""
    base, anyone = hash_type & 0x1f, bool(hash_type & 0x80)
    if n_in >= len(tx["vin"]) or (base == 3 and n_in >= len(tx["vout"])):
        return None
    b = struct.pack("<i", tx["version"])
    ins = [n_in] if anyone else range(len(tx["vin"]))
    b += compact_size(len(ins))
    for i in ins:
        h, idx, _, seq = tx["vin"][i]
        b += h + struct.pack("<I", idx)
        b += legacy_script_code(code) if i == n_in else b"\x00"
        b += struct.pack("<I", 0 if i != n_in and base in (2, 3) else seq)
    n_out = 0 if base == 2 else n_in + 1 if base == 3 else len(tx["vout"])
    b += compact_size(n_out)
    for i in range(n_out):
        b += _out((-1, b"")) if base == 3 and i != n_in else _out(tx["vout"][i])
    return b + struct.pack("<I", tx["lock_time"]) + struct.pack("<i", hash_type)


def bip143_preimage(code, tx, n_in, hash_type, amount):
    base, anyone = hash_type & 0x1f, bool(hash_type & 0x80)
    zero = bytes(32)
    hp = zero if anyone else sha256d(b"".join(h + struct.pack("<I", i) for h, i, _, _ in tx["vin"]))
    hs = zero if anyone or base in (2, 3) else sha256d(b"".join(struct.pack("<I", s) for _, _, _, s in tx["vin"]))
    if base not in (2, 3):
        ho = sha256d(b"".join(_out(o) for o in tx["vout"]))
    elif base == 3 and n_in < len(tx["vout"]):
        ho = sha256d(_out(tx["vout"][n_in]))
    else:
        ho = zero
    h, idx, _, seq = tx["vin"][n_in]
    return (struct.pack("<i", tx["version"]) + hp + hs + h + struct.pack("<I", idx) + compact_size(len(code)) + code +
            struct.pack("<q", amount) + struct.pack("<I", seq) + ho + struct.pack("<I", tx["lock_time"]) +
            struct.pack("<i", hash_type))


def preimage(code, raw_tx, n_in, hash_type, amount=0, sigversion=0):
    tx = parse_tx(raw_tx) if isinstance(raw_tx, (bytes, bytearray)) else raw_tx
    return bip143_preimage(code, tx, n_in, hash_type, amount) if sigversion else legacy_preimage(code, tx, n_in, hash_type)


def signature_hash(code, raw_tx, n_in, hash_type, amount=0, sigversion=0):
    """32 bytes in the order of the native core's signature_hash (uint256 storage order)."""
    p = preimage(code, raw_tx, n_in, hash_type, amount, sigversion)
    return ONE if p is None else sha256d(p)
