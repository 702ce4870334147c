"""Shared by test_script_cache.py (CPU) and test_gpu_script_cache.py: a regtest base (the hand-mined
base of sig_window_util, whose last block splits a coinbase into 32 P2PKH / P2WPKH outputs, plus one
block that pays two of them to a 2-of-3 P2SH script), single-input spends of those outputs, and
blocks assembled from a node's mempool with further transactions put in at chosen positions."""
import sig_window_util as W

N_BASE = W.N_BASE + 1
WITNESS_OUTPUTS = tuple(range(3, W.N_SPLIT, 4))                          # P2WPKH outputs of the split
LEGACY_OUTPUTS = tuple(n for n in range(2, W.N_SPLIT) if n % 4 != 3)     # P2PKH ones (0 and 1 fund the P2SH)
MULTISIG_KEYS = (201, 202, 203)


def _p2pkh_tx_in(core, txid, n):
    vin = core.TxIn()
    op = core.OutPoint()
    op.hash, op.n = txid, n
    vin.prevout = op
    vin.sequence = 0xffffffff
    return vin


def redeem_script(core):
    pubs = [W._key(core, k)[1] for k in MULTISIG_KEYS]
    return core.script_push_int(2) + b"".join(core.script_push_data(p) for p in pubs) + core.script_push_int(3) + b"\xae"


def make_base(core):
    """-> {"base": N_BASE serialized blocks, "params", "split": txid, "each": value of a split output,
    "fund": txid of the transaction with the two P2SH outputs, "fund_value"}."""
    base, _ = W.build_chain(core)
    st = W.new_state()
    st.min_relay_fee = 0
    W.feed(st, base)
    act = st.params.kawpow_activation_time
    split = core.Block.deserialize(base[-1], act).vtx[1]
    fx = {"params": st.params, "split": split.txid(), "each": split.vout[0].value}
    redeem = redeem_script(core)
    p2sh = b"\xa9\x14" + core.hash160(redeem) + b"\x87"
    coins = [coin(core, fx, n) for n in (0, 1)]
    fund, fee = W._spend(core, coins, p2sh, (1,))
    ok, why, _ = st.accept_to_mempool(fund)
    assert ok, why
    raw = assemble(core, st)
    assert all(s.ok for s in W.feed(st, [raw])) and st.height() == N_BASE
    fx.update(base=base + [raw], fund=fund.txid(), fund_value=fund.vout[0].value)
    return fx


def coin(core, fx, n):
    sec, pub = W._key(core, 1 + n)
    return (fx["split"], n, fx["each"], sec, pub, n % 4 == 3)


def pay(core, fx, n, hash_type=1):
    """One input, one output: split output n (P2WPKH when n % 4 == 3, else P2PKH) signed with `hash_type`."""
    dest = W._p2pkh(core, W._key(core, 99)[1])
    return W._spend(core, [coin(core, fx, n)], dest, (hash_type,))[0]


def pay_multisig(core, fx, k, signers=(0, 2)):
    """Spends P2SH output k of the funding transaction, signed by the keys `signers` of its three."""
    redeem = redeem_script(core)
    tx = core.Transaction()
    tx.version = 2
    vin = _p2pkh_tx_in(core, fx["fund"], k)
    tx.vin = [vin]
    tx.vout = [core.TxOut(fx["fund_value"] - 10_000, W._p2pkh(core, W._key(core, 99)[1]))]
    msg = core.signature_hash(redeem, tx.serialize(True), 0, 1, fx["fund_value"], 0)
    sigs = [core.secp_sign(msg, W._key(core, MULTISIG_KEYS[j])[0]) + b"\x01" for j in signers]
    vin.script_sig = b"\x00" + b"".join(core.script_push_data(s) for s in sigs) + core.script_push_data(redeem)
    tx.vin = [vin]
    return tx


def corrupt(tx):
    """Flip a bit inside the DER signature of the transaction's first input (witness or scriptSig)."""
    vins = list(tx.vin)
    if vins[0].witness:
        wit = list(vins[0].witness)
        sig = bytearray(wit[0])
        sig[9] ^= 1
        wit[0] = bytes(sig)
        vins[0].witness = wit
    else:
        s = bytearray(vins[0].script_sig)
        assert s[0] in (0x46, 0x47, 0x48)  # a signature push first
        s[10] ^= 1
        vins[0].script_sig = bytes(s)
    tx.vin = vins
    return tx


def fresh(fx, **attrs):
    """A node at the base; `attrs` are set on it once the base is connected."""
    st = W.new_state()
    W.feed(st, fx["base"])
    assert st.height() == N_BASE
    st.min_relay_fee = 0  # -minrelaytxfee=0: the spends pay 10000 per input
    for k, v in attrs.items():
        setattr(st, k, v)
    return st


def accept(st, txs):
    for tx in txs:
        ok, why, _ = st.accept_to_mempool(tx)
        assert ok, why


def assemble(core, st, edit=None):
    """The next block from the node's mempool, solved and serialized. `edit`(list of the block's
    non-coinbase transactions) -> the list to mine instead; the commitment and merkle root follow."""
    from nodexa_chain_core_amd.miner.assembler import BlockAssembler

    script = W._p2pkh(core, W._key(core, 0)[1])
    blk = BlockAssembler(st).create_new_block(script).block
    act = st.params.kawpow_activation_time

    def mutate(core_, b):
        vtx = list(b.vtx)
        b.vtx = vtx[:1] + list(edit(vtx[1:]) if edit is not None else vtx[1:])

    return W.variant(core, st.params, [blk.serialize(act)], {1: mutate})[0]


def block_of(core, fx, raw):
    return core.Block.deserialize(raw, fx["params"].kawpow_activation_time)


def block_hash(core, fx, raw):
    return core.HeaderChain(fx["params"]).block_hash(block_of(core, fx, raw).header)


def put_at(positions_txs):
    """An `edit` for assemble: the given {position: tx} land at exactly these positions of the result."""
    def edit(txs):
        out, rest = [], list(txs)
        for pos in range(len(txs) + len(positions_txs)):
            out.append(positions_txs[pos] if pos in positions_txs else rest.pop(0))
        return out
    return edit
