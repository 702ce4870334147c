"""Shared by test_sig_groups.py (CPU) and test_gpu_sig_groups.py: the group table's packing, the
oracle of CHECKMULTISIG's walk over a full truth matrix, verdict arrays with sentinels around their
groups, multisig blocks of every shape, signer subset and script kind, and a hand-mined regtest
chain whose blocks spend multisig outputs signed by every subset of their keys."""
import itertools
import random
import struct

import sig_window_util as W

from nodexa_chain_core_amd.utils.synth_block import _coinbase, make_consolidation_block

GROUP = struct.Struct("<4I")  # SigGroup: first, n_sigs, n_keys, pad
OK, FAIL, ASK = 1, 0, 2
SENTINEL = 0xabcd0123         # no verdict: a resolver that touches it shows
VALUES = (0, 1, 2, 3, 0xffffffff)
# 8-of-15 has exactly 64 pairs
SEEDED_SHAPES = ((1, 1), (1, 2), (2, 3), (1, 20), (20, 20), (15, 15), (8, 15))


def table(groups):
    return b"".join(GROUP.pack(first, m, n, 0) for first, m, n in groups)


def untable(raw):
    return [GROUP.unpack_from(raw, o)[:3] for o in range(0, len(raw), GROUP.size)]


def pairs(m, n):
    return m * (n - m + 1)


# ---------------------------------------------------------------- the oracle
def walk_oracle(m, n, truth):
    """OP_CHECKMULTISIG's loop (`while (success && nsigs > 0)`) as the interpreter runs it, over the
    full m x n matrix: truth[a][b] is the raw verdict of signature a against key b, both in walk
    order. A 2 met on the way stops the walk: the host decides."""
    isig = ikey = 0
    nsigs, nkeys = m, n
    success = True
    while success and nsigs > 0:
        v = truth[isig][ikey]
        if v == 2:
            return ASK
        if v == 1:
            isig += 1
            nsigs -= 1
        ikey += 1
        nkeys -= 1
        if nsigs > nkeys:
            success = False
    return OK if success else FAIL


def band_of(m, n, truth):
    """The entries a group holds: signature a against keys a .. a + w - 1."""
    w = n - m + 1
    return [truth[a][a + d] for a in range(m) for d in range(w)]


def matrix_of(m, n, band, outside):
    """The full matrix of a band; outside(a, b) fills the cells no group holds."""
    w = n - m + 1
    return [[band[a * w + (b - a)] if 0 <= b - a < w else outside(a, b) for b in range(n)] for a in range(m)]


class Verdicts:
    """A verdict array built group by group, with sentinels before, between and after them."""

    def __init__(self):
        self.v, self.groups, self.want = [SENTINEL], [], [SENTINEL]

    def add(self, m, n, band, outcome, gap=1):
        assert len(band) == pairs(m, n)
        self.groups.append((len(self.v), m, n))
        self.v += band
        self.want += [outcome] * len(band)
        self.v += [SENTINEL] * gap
        self.want += [SENTINEL] * gap

    def table(self):
        return table(self.groups)


def exhaustive(max_n):
    """Every shape 1 <= m <= n <= max_n with every {0, 1} band, each against the oracle over three
    full matrices: the cells outside the band all 1, all 0, and 2 (the band suffices). -> Verdicts"""
    out = Verdicts()
    for n in range(1, max_n + 1):
        for m in range(1, n + 1):
            for band in itertools.product((0, 1), repeat=pairs(m, n)):
                band = list(band)
                want = {walk_oracle(m, n, matrix_of(m, n, band, lambda a, b, x=x: x)) for x in (1, 0, 2)}
                assert len(want) == 1, (m, n, band)
                out.add(m, n, band, want.pop(), gap=(m + n) % 2)
    return out


def seeded(seed=15, per_shape=40):
    """Bands over VALUES for SEEDED_SHAPES; half of them lean towards valid so that long walks get
    far. The cells outside the band are drawn too: the oracle never reads them."""
    rng = random.Random(seed)
    out = Verdicts()
    for m, n in SEEDED_SHAPES:
        for k in range(per_shape):
            weights = (1, 6, 1, 1, 1) if k % 2 else (4, 4, 1, 1, 1)
            if k % 4 == 3:
                weights = (1, 30, 0.3, 0.3, 0.3)
            band = rng.choices(VALUES, weights, k=pairs(m, n))
            truth = matrix_of(m, n, band, lambda a, b: rng.choice(VALUES))
            out.add(m, n, band, walk_oracle(m, n, truth), gap=k % 3)
    return out


# ---------------------------------------------------------------- multisig blocks
# (m, n, signers): 2-of-3 by each pair, 1-of-2 by either key, 2-of-2, 3-of-3
SHAPES = ((2, 3, (0, 1)), (2, 3, (0, 2)), (2, 3, (1, 2)), (1, 2, (0,)), (1, 2, (1,)), (2, 2, (0, 1)), (3, 3, (0, 1, 2)))
KINDS = ("p2sh", "bare", "p2wsh")
HASH_TYPES = W.HASH_TYPES


def shape_block(m, n, signers, kind, bad_at=None, seed=60):
    """10 inputs in two transactions, every second one an m-of-n of `kind` signed by `signers`, the
    others P2PKH; hash types cycle through all forms."""
    return make_consolidation_block(2, 5, seed=seed + 7 * m + n, hash_types=HASH_TYPES, multisig_every=2,
                                    multisig_mn=(m, n), multisig_signers=signers, multisig_kind=kind, bad_at=bad_at)


def connect(core, blk, view, height, mode=0, **kw):
    """connect_block as -gpusighash=`mode` defers."""
    return core.connect_block(blk, height, view, True, True, None, 0, core.BLOCK_SCRIPT_VERIFY_FLAGS, 2,
                              defer_sighash=mode >= 1, defer_all_forms=mode == 2, **kw)


def pushes(script):
    """The data pushes of a script made of direct pushes, OP_0 and small integers."""
    out, at = [], 0
    while at < len(script):
        op = script[at]
        at += 1
        if op == 0x4c:
            op = script[at]
            at += 1
        elif op == 0x4d:
            op = script[at] | script[at + 1] << 8
            at += 2
        elif op > 0x4d or op == 0:
            out.append(b"" if op == 0 else bytes([op]))
            continue
        out.append(script[at:at + op])
        at += op
    return out


def multisig_parts(core, vin, spk):
    """-> (script code, signatures in push order, keys in script order, sigversion) of a multisig input."""
    if spk[:2] == b"\x00\x20":
        code, sigs, sv = vin.witness[-1], list(vin.witness[1:-1]), 1
    elif spk[:2] == b"\xa9\x14":
        p = pushes(vin.script_sig)
        code, sigs, sv = p[-1], p[1:-1], 0
    else:
        code, sigs, sv = spk, pushes(vin.script_sig)[1:], 0
    keys = [k for k in pushes(code[:-1]) if len(k) == 33]
    return code, sigs, keys, sv


def resolved(core, res):
    """Per-entry golden verdicts of a result, then the model over its groups."""
    return core.sig_group_resolve_model([int(core.secp_verify(*it)) for it in res.sig_items()], res.sig_group_table())


def group_verifier(core, calls=None):
    """A window verifier on the host that answers as -gpumultisig asks: resolved entries."""
    def verify(results):
        if calls is not None:
            calls.append([(res.num_sigs, len(res.sig_groups)) for res in results])
        return [[v == 1 for v in resolved(core, res)] for res in results]
    return verify


def reverse_signatures(core, blk, t=1, i=0):
    """The signatures of a P2SH multisig input pushed in the opposite order (no key order fits them)."""
    vtx = list(blk.vtx)
    tx = vtx[t]
    vins = list(tx.vin)
    p = pushes(vins[i].script_sig)
    assert p[0] == b"" and len(p) >= 4
    vins[i].script_sig = b"\x00" + b"".join(core.script_push_data(s) for s in reversed(p[1:-1])) + \
        core.script_push_data(p[-1])
    tx.vin = vins
    vtx[t] = tx
    blk.vtx = vtx


def corrupt_multisig_signature(core, blk, t=1, i=0):
    """One bit inside S of the first pushed signature of a P2SH multisig input."""
    vtx = list(blk.vtx)
    tx = vtx[t]
    vins = list(tx.vin)
    p = pushes(vins[i].script_sig)
    sig = bytearray(p[1])
    sig[-4] ^= 1
    vins[i].script_sig = b"\x00" + b"".join(core.script_push_data(s) for s in [bytes(sig)] + p[2:-1]) + \
        core.script_push_data(p[-1])
    tx.vin = vins
    vtx[t] = tx
    blk.vtx = vtx


def one_input_block(core, spk, build_script_sig, value=100_000, height=1000):
    """-> (block, view, height): one transaction spending one coin that pays the bare script `spk`;
    build_script_sig(sign) makes its scriptSig, sign(secret) a SIGHASH_ALL signature of the input."""
    import hashlib

    view = core.CoinsView()
    prev = hashlib.sha256(b"sig-groups-" + spk).digest()
    view.add(prev, 0, value, spk, 1, False)
    tx = core.Transaction()
    tx.version = 2
    vin = core.TxIn()
    op = core.OutPoint()
    op.hash, op.n = prev, 0
    vin.prevout = op
    vin.sequence = 0xffffffff
    tx.vin = [vin]
    tx.vout = [core.TxOut(value - 1000, b"\x76\xa9\x14" + bytes(20) + b"\x88\xac")]
    raw = tx.serialize(True)
    vin.script_sig = build_script_sig(lambda sec: core.secp_sign(core.signature_hash(spk, raw, 0, 1, value, 0), sec) + b"\x01")
    tx.vin = [vin]
    blk = core.Block()
    blk.vtx = [_coinbase(height), tx]
    return blk, view, height


# ---------------------------------------------------------------- a regtest chain of multisig spends
N_OUT = 24
N_CHAIN = 4
PER_BLOCK = N_OUT // N_CHAIN


def _output(core, k):
    """Output k of the split: shape and signers SHAPES[k % 7], kind KINDS[k % 3]."""
    m, n, signers = SHAPES[k % len(SHAPES)]
    keys = [W._key(core, 1000 + 20 * k + j) for j in range(n)]
    script = core.script_push_int(m) + b"".join(core.script_push_data(pub) for _, pub in keys) + \
        core.script_push_int(n) + b"\xae"
    kind = KINDS[k % 3]
    spk = {"p2sh": b"\xa9\x14" + core.hash160(script) + b"\x87", "bare": script,
           "p2wsh": b"\x00\x20" + core.sha256(script)}[kind]
    return kind, script, spk, [keys[j][0] for j in signers], tuple(signers) == tuple(range(n - m, n))


def build_chain(core):
    """-> (base, chain, first_try): 101 and N_CHAIN serialized blocks. The last block of the base
    splits the first coinbase into N_OUT multisig outputs (_output); block j of the chain spends
    outputs 6j .. 6j + 5 in one transaction. first_try[j]: how many of block j's inputs are signed by
    the last m keys, the only ones a walk that pairs signature k with key k accepts."""
    from nodexa_chain_core_amd.miner.assembler import BlockAssembler

    st = W.new_state()
    act = st.params.kawpow_activation_time
    sec0, pub0 = W._key(core, 0)
    script0 = W._p2pkh(core, pub0)
    out = []

    def mine(txs=()):
        for tx, fee in txs:
            st.add_to_mempool(tx, fee)
        blk = W.solve(core, BlockAssembler(st).create_new_block(script0).block)
        assert len(blk.vtx) == 1 + len(txs)
        r = st.process_new_block(blk)
        assert r.ok, r.reject
        out.append(blk.serialize(act))
        return blk

    first = mine()
    for _ in range(W.N_BASE - 2):
        mine()
    cb = first.vtx[0]
    outs = [_output(core, k) for k in range(N_OUT)]
    split = core.Transaction()
    split.version = 2
    vin = core.TxIn()
    op = core.OutPoint()
    op.hash, op.n = cb.txid(), 0
    vin.prevout = op
    vin.sequence = 0xffffffff
    each = (cb.vout[0].value - 100_000) // N_OUT
    split.vout = [core.TxOut(each, o[2]) for o in outs]
    split.vin = [vin]
    msg = core.signature_hash(script0, split.serialize(True), 0, 1, cb.vout[0].value, 0)
    vin.script_sig = core.script_push_data(core.secp_sign(msg, sec0) + b"\x01") + core.script_push_data(pub0)
    split.vin = [vin]
    mine([(split, cb.vout[0].value - N_OUT * each)])
    base, out[:] = list(out), []
    txid = split.txid()
    dest = W._p2pkh(core, W._key(core, 99)[1])
    first_try = []
    for j in range(N_CHAIN):
        picks = range(PER_BLOCK * j, PER_BLOCK * (j + 1))
        tx = core.Transaction()
        tx.version = 2
        vins = []
        for k in picks:
            vin = core.TxIn()
            op = core.OutPoint()
            op.hash, op.n = txid, k
            vin.prevout = op
            vin.sequence = 0xffffffff
            vins.append(vin)
        tx.vin = vins
        fee = 10_000 * PER_BLOCK
        share = (each * PER_BLOCK - fee) // PER_BLOCK
        tx.vout = [core.TxOut(share, dest) for _ in picks]
        raw = tx.serialize(True)
        for i, k in enumerate(picks):
            kind, script, _, secs, _ = outs[k]
            ht = HASH_TYPES[k % len(HASH_TYPES)]
            msg = core.signature_hash(script, raw, i, ht, each, 1 if kind == "p2wsh" else 0)
            sigs = [core.secp_sign(msg, sec) + bytes([ht & 0xff]) for sec in secs]
            if kind == "p2wsh":
                vins[i].witness = [b""] + sigs + [script]
            else:
                vins[i].script_sig = b"\x00" + b"".join(core.script_push_data(s) for s in sigs) + \
                    (core.script_push_data(script) if kind == "p2sh" else b"")
        tx.vin = vins
        mine([(tx, each * PER_BLOCK - share * PER_BLOCK)])
        first_try.append(sum(outs[k][4] for k in picks))
    return base, out, first_try
