"""Shared by test_sig_window.py (CPU) and test_gpu_sig_window.py: five small connected blocks for the
window packer and verifier, the block-size and verdict-pattern set of the per-block records, and a
hand-mined regtest chain (a base that splits a matured coinbase, then 8 blocks that spend the split)
with variants that carry a corrupted signature or a wrong coinbase amount."""
import hashlib
import struct

from nodexa_chain_core_amd.utils.synth_block import make_consolidation_block

JOB = struct.Struct("<10I")     # SighashJob: off[4], len[4], out_index, kind
VAR_JOB = struct.Struct("<4I")  # SighashVarJob: first_seg, n_seg, out_index, kind
SEG = struct.Struct("<2I")
RECORD = struct.Struct("<4I")   # n_valid, n_invalid, n_ask_host, first_not_valid
NONE = 0xffffffff

# ---------------------------------------------------------------- five blocks
# (n_txs, inputs per tx): 2, 15, 0, 40 and 14 inputs; the multisig inputs carry two signatures
FIVE = ((1, 2), (3, 5), (0, 1), (4, 10), (2, 7))
HASH_TYPES = (1, 0x81, 2, 3, 0x82, 0x83, 0)


def five_blocks(core, mode, order=(0, 1, 2, 3, 4), bad=None):
    """-> ([ConnectResult], [info]) of the five blocks in `order`, each connected against its own
    view as -gpusighash=`mode` connects it. bad = (block, input): that input's signature is corrupted."""
    results, infos = [], []
    for b in order:
        n_txs, n_in = FIVE[b]
        blk, view, height, info = make_consolidation_block(
            n_txs, n_in, seed=40 + b, hash_types=HASH_TYPES, witness_every=4, multisig_every=5,
            bad_at=bad[1] if bad is not None and bad[0] == b else None)
        res, _ = core.connect_block(blk, height, view, True, True, None, 0, core.BLOCK_SCRIPT_VERIFY_FLAGS, 4,
                                    defer_sighash=mode >= 1, defer_all_forms=mode == 2)
        assert res.ok and res.num_sigs == info["sigs"]
        results.append(res)
        infos.append(info)
    return results, infos


# ---------------------------------------------------------------- records
SIZES = (0, 1, 63, 64, 65, 0, 130)


def sig_begin_of(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + n)
    return out


def verdict_patterns(sizes=SIZES):
    """[(name, verdicts)] over blocks of `sizes`: all valid; one invalid at the first position of
    each block in turn, then at the last; verdict 2s; an out-of-range verdict."""
    sb = sig_begin_of(sizes)
    n = sb[-1]
    out = [("all-valid", [1] * n)]
    for b, size in enumerate(sizes):
        if size == 0:
            continue
        for where, at in (("first", sb[b]), ("last", sb[b + 1] - 1)):
            v = [1] * n
            v[at] = 0
            out.append((f"invalid-{where}-of-block-{b}", v))
    v = [1] * n
    for at in (sb[2] + 5, sb[2] + 62, sb[4], sb[6] + 64, sb[6] + 129):
        v[at] = 2
    out.append(("ask-host", v))
    v = [1] * n
    v[sb[3] + 63], v[sb[6] + 1], v[sb[6] + 70] = 3, 0xffffffff, 0x80000001
    out.append(("out-of-range", v))
    v = [(1, 0, 2, 1, 7)[(k * 7 + k // 5) % 5] for k in range(n)]
    out.append(("mixed", v))
    out.append(("none-valid", [0] * n))
    return out


def records_ref(verdicts, sig_begin):
    """The records as the issue defines them, in Python."""
    out = b""
    for b in range(len(sig_begin) - 1):
        vs = verdicts[sig_begin[b]:sig_begin[b + 1]]
        not_valid = [k for k, v in enumerate(vs) if v != 1]
        out += RECORD.pack(sum(v == 1 for v in vs), sum(v not in (1, 2) for v in vs), sum(v == 2 for v in vs),
                           not_valid[0] if not_valid else NONE)
    return out


# ---------------------------------------------------------------- a regtest chain
N_BASE = 101      # 100 empty blocks and the block that splits the first coinbase
N_CHAIN = 8
EMPTY_BLOCK = 7   # of the 8: no transaction but the coinbase
N_SPLIT = 32
WITNESS_COMMITMENT_HEADER = b"\x6a\x24\xaa\x21\xa9\xed"


def _key(core, i):
    k = hashlib.sha256(f"sig-window-{i}".encode()).digest()
    assert core.secp_seckey_valid(k)
    return k, core.secp_pubkey_create(k, True)


def _p2pkh(core, pub):
    return b"\x76\xa9\x14" + core.hash160(pub) + b"\x88\xac"


def new_state(datadir=None):
    from nodexa_chain_core_amd.chain.state import REGTEST_KAWPOW_FROM_GENESIS, ChainState, make_params

    st = ChainState(make_params("regtest", REGTEST_KAWPOW_FROM_GENESIS), datadir)
    st.gpu_signatures = "off"
    return st


def solve(core, blk):
    ctx = core.get_epoch_context(0)
    h = blk.header
    for n in range(256):  # regtest target 2^255
        fin, mix = core.kawpow_hash(ctx, h.height, h.kawpow_header_hash()[::-1], n)
        if fin[0] < 0x80:
            h.nonce64, h.mix_hash = n, mix[::-1]
            blk.header = h
            return blk
    raise AssertionError("no nonce found")


def _spend(core, coins, dest_spk, hash_types):
    """One transaction spending `coins` [(txid, n, value, secret, pub, witness)] into as many equal outputs."""
    tx = core.Transaction()
    tx.version = 2
    vins = []
    for txid, n, _, _, _, _ in coins:
        vin = core.TxIn()
        op = core.OutPoint()
        op.hash, op.n = txid, n
        vin.prevout = op
        vin.sequence = 0xffffffff
        vins.append(vin)
    tx.vin = vins
    total = sum(c[2] for c in coins)
    fee = 10_000 * len(coins)
    # as many outputs as inputs, so that SINGLE has its output
    share = (total - fee) // len(coins)
    tx.vout = [core.TxOut(share, dest_spk) for _ in coins]
    raw = tx.serialize(True)
    for i, (_, _, value, sec, pub, witness) in enumerate(coins):
        ht = hash_types[i % len(hash_types)]
        msg = core.signature_hash(_p2pkh(core, pub), raw, i, ht, value, 1 if witness else 0)
        sig = core.secp_sign(msg, sec) + bytes([ht & 0xff])
        if witness:
            vins[i].witness = [sig, pub]
            vins[i].script_sig = b""
        else:
            vins[i].script_sig = core.script_push_data(sig) + core.script_push_data(pub)
    tx.vin = vins
    return tx, total - share * len(coins)


def build_chain(core):
    """-> (base, chain): N_BASE and N_CHAIN serialized blocks. Block N_BASE splits the first coinbase
    into 32 outputs (every fourth P2WPKH); block k of the chain (but EMPTY_BLOCK) spends three of them
    in one transaction whose first input is P2PKH signed ALL, the others with other hash types."""
    from nodexa_chain_core_amd.miner.assembler import BlockAssembler

    st = new_state()
    act = st.params.kawpow_activation_time
    sec0, pub0 = _key(core, 0)
    script = _p2pkh(core, pub0)
    out = []

    def mine(txs=()):
        for tx, fee in txs:
            st.add_to_mempool(tx, fee)
        blk = solve(core, BlockAssembler(st).create_new_block(script).block)
        assert len(blk.vtx) == 1 + len(txs)
        r = st.process_new_block(blk)
        assert r.ok, r.reject
        out.append(blk.serialize(act))
        return blk

    first = mine()
    for _ in range(N_BASE - 2):
        mine()
    assert st.height() == core.COINBASE_MATURITY
    cb = first.vtx[0]
    keys = [_key(core, 1 + k) for k in range(N_SPLIT)]
    split = core.Transaction()
    split.version = 2
    vin = core.TxIn()
    op = core.OutPoint()
    op.hash, op.n = cb.txid(), 0
    vin.prevout = op
    vin.sequence = 0xffffffff
    each = (cb.vout[0].value - 100_000) // N_SPLIT
    split.vout = [core.TxOut(each, (b"\x00\x14" + core.hash160(pub)) if k % 4 == 3 else _p2pkh(core, pub))
                  for k, (_, pub) in enumerate(keys)]
    split.vin = [vin]
    msg = core.signature_hash(script, split.serialize(True), 0, 1, cb.vout[0].value, 0)
    vin.script_sig = core.script_push_data(core.secp_sign(msg, sec0) + b"\x01") + core.script_push_data(pub0)
    split.vin = [vin]
    mine([(split, cb.vout[0].value - N_SPLIT * each)])
    base, out[:] = list(out), []
    txid = split.txid()
    dest = _p2pkh(core, _key(core, 99)[1])
    hash_types = ((1, 0x81, 3), (1, 2, 0x83), (1, 1, 0x82), (1, 3, 1))
    slot = 0
    for k in range(1, N_CHAIN + 1):
        if k == EMPTY_BLOCK:
            mine()
            continue
        # P2PKH first; outputs 3, 7, ... are P2WPKH
        picks = [n for n in range(N_SPLIT) if n % 4 != 3][slot * 2:slot * 2 + 2] + [4 * slot + 3]
        coins = [(txid, n, each, keys[n][0], keys[n][1], n % 4 == 3) for n in picks]
        mine([_spend(core, coins, dest, hash_types[slot % 4])])
        slot += 1
    return base, out


def corrupt_signature(core, blk):
    """Flip a bit inside the DER signature of the first input of the block's first spend."""
    vtx = list(blk.vtx)
    tx = vtx[1]
    vins = list(tx.vin)
    sig = bytearray(vins[0].script_sig)
    assert sig[0] in (0x47, 0x48, 0x46) and sig[sig[0]] == 0x01  # a signature push ending in hash type ALL
    sig[10] ^= 1
    vins[0].script_sig = bytes(sig)
    tx.vin = vins
    vtx[1] = tx
    blk.vtx = vtx


def overpay_community(core, blk):
    """The community-fund output one unit too high: refused at connection, by the reward rule."""
    vtx = list(blk.vtx)
    cb = vtx[0]
    outs = list(cb.vout)
    outs[1] = core.TxOut(outs[1].value + 1, outs[1].script_pubkey)
    cb.vout = outs
    vtx[0] = cb
    blk.vtx = vtx


def variant(core, params, chain, mutations):
    """`chain` with mutations {k: fn(core, block)} applied to its blocks k (1-based): the witness
    commitment and merkle root are recomputed, the later blocks are re-parented, all are solved again."""
    act = params.kawpow_activation_time
    hc = core.HeaderChain(params)
    out, prev, changed = [], None, False
    for k, raw in enumerate(chain, 1):
        blk = core.Block.deserialize(raw, act)
        if k in mutations:
            mutations[k](core, blk)
            vtx = list(blk.vtx)
            cb = vtx[0]
            outs = list(cb.vout)
            at = blk.witness_commitment_index()
            assert at >= 0
            outs[at] = core.TxOut(0, WITNESS_COMMITMENT_HEADER + core.sha256d(blk.witness_merkle_root() + bytes(32)))
            cb.vout = outs
            vtx[0] = cb
            blk.vtx = vtx
            changed = True
        if changed:
            h = blk.header
            if prev is not None:
                h.prev = prev
            h.merkle_root = blk.merkle_root()[0]
            blk.header = h
            solve(core, blk)
        prev = hc.block_hash(blk.header)
        out.append(blk.serialize(act))
    return out


def feed(st, raws, one_walk=False):
    """process_new_block for each serialized block -> the states. `one_walk`: every block but the
    last is only stored, so that the last one's activation connects them all in one walk."""
    act = st.params.kawpow_activation_time
    states = []
    real = st._activate
    for k, raw in enumerate(raws):
        if one_walk and k < len(raws) - 1:
            st._activate = lambda: {}
        try:
            states.append(st.process_new_block(type(st.params.genesis).deserialize(raw, act)))
        finally:
            st._activate = real
    return states


def host_verifier(core, calls=None):
    """A window verifier on the host: the golden model over each result's sig_items()."""
    def verify(results):
        out = [[bool(core.secp_verify(*it)) for it in res.sig_items()] for res in results]
        if calls is not None:
            calls.append([res.num_sigs for res in results])
        return out
    return verify
