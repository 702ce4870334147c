"""Synthetic signed blocks for block-connection tests and benchmarks.

`make_signed_block(n_txs, ...)` returns a CoinsView holding one P2PKH (or P2WPKH) coin per
transaction and a block whose transactions each spend one of them with a real ECDSA signature
(RFC 6979, csrc/crypto/secp256k1.cpp) — the shape of an ordinary payments block. Keys are
derived deterministically from the seed so runs are reproducible.
"""
from __future__ import annotations

import hashlib

from .. import core

_core = core()


def _key(seed: int, i: int) -> bytes:
    while True:
        k = hashlib.sha256(f"nodexa-synth-{seed}-{i}".encode()).digest()
        if _core.secp_seckey_valid(k):
            return k
        i += 1 << 32


def _coinbase(height: int):
    cb = _core.Transaction()
    cb.version = 1
    cin = _core.TxIn()
    cin.script_sig = _core.script_push_int(height) + b"\x00"
    cb.vin = [cin]
    cb.vout = [_core.TxOut(0, b"\x51")]
    return cb


def make_consolidation_block(n_txs: int, inputs_per_tx, seed: int = 0, hash_types=(1,), witness_every: int = 0,
                             multisig_every: int = 0, bad_at: int | None = None, height: int = 1000):
    """-> (block, view, height, info): `n_txs` transactions that each spend many seeded coins into
    two outputs, the shape whose legacy signature hashes cost the host quadratic work.

    `inputs_per_tx` is a count, or a (low, high) pair from which each transaction's count is drawn
    with the seed. Inputs are numbered through the block (0 = first input of the first
    transaction); input g signs with hash_types[g % len(hash_types)], is P2WPKH when
    `witness_every` divides g + 1, else P2SH 2-of-3 when `multisig_every` divides g + 1 (two
    signatures), else P2PKH. With `bad_at`, the first signature of that input is corrupted.
    `info` counts what the block implies: "inputs", "sigs", "device_sigs" (legacy signatures whose
    hash has the SIGHASH_ALL form: no ANYONECANPAY, base type neither NONE nor SINGLE),
    "host_sigs" (the rest), and "bad_sig" (index of the corrupted signature among "sigs")."""
    import random

    rng = random.Random(seed)
    view = _core.CoinsView()
    txs = [_coinbase(height)]
    info = {"inputs": 0, "sigs": 0, "device_sigs": 0, "host_sigs": 0, "bad_sig": None}
    g = 0
    for t in range(n_txs):
        n_in = inputs_per_tx if isinstance(inputs_per_tx, int) else rng.randint(*inputs_per_tx)
        spends, vins, total = [], [], 0
        for i in range(n_in):
            gi = g + i
            witness = witness_every > 0 and (gi + 1) % witness_every == 0
            multisig = not witness and multisig_every > 0 and (gi + 1) % multisig_every == 0
            secs = [_key(seed, 3 * gi + k) for k in range(3 if multisig else 1)]
            pubs = [_core.secp_pubkey_create(s, True) for s in secs]
            if multisig:
                redeem = b"\x52" + b"".join(_core.script_push_data(p) for p in pubs) + b"\x53\xae"
                spk, code = b"\xa9\x14" + _core.hash160(redeem) + b"\x87", redeem
            else:
                redeem = None
                code = b"\x76\xa9\x14" + _core.hash160(pubs[0]) + b"\x88\xac"
                spk = (b"\x00\x14" + _core.hash160(pubs[0])) if witness else code
            prev = hashlib.sha256(f"consolidate-{seed}-{gi}".encode()).digest()
            value = 50_000 + gi
            total += value
            view.add(prev, 0, value, spk, 1, False)
            vin = _core.TxIn()
            op = _core.OutPoint()
            op.hash, op.n = prev, 0
            vin.prevout = op
            vin.sequence = 0xffffffff
            vins.append(vin)
            spends.append((witness, redeem, code, secs, pubs, value, hash_types[gi % len(hash_types)]))
        tx = _core.Transaction()
        tx.version = 2
        tx.vin = vins
        keep = b"\x76\xa9\x14" + bytes(20) + b"\x88\xac"
        tx.vout = [_core.TxOut(total // 2, keep), _core.TxOut(total - total // 2 - 1000 * n_in, keep)]
        raw = tx.serialize(True)  # the hashes do not cover the scripts still to be filled in
        for i, (witness, redeem, code, secs, pubs, value, ht) in enumerate(spends):
            msg = _core.signature_hash(code, raw, i, ht, value, 1 if witness else 0)
            sigs = []
            # 2-of-3: the last two keys sign, so that CHECKMULTISIG's walk (last signature against
            # last key first) pairs every signature with its key at the first try, as a deferring
            # checker assumes
            for k, sec in enumerate(secs[-2:]):
                sig = bytearray(_core.secp_sign(msg, sec))
                if bad_at == g + i and k == 0:
                    sig[-3] ^= 0x01  # inside S: still valid DER, wrong signature
                    # position in connect_block's deferred order, where a multisig input's
                    # signatures come last first
                    info["bad_sig"] = info["sigs"] + (1 if redeem is not None else 0)
                sigs.append(bytes(sig) + bytes([ht & 0xff]))
                info["sigs"] += 1
                legacy_all = not witness and not (ht & 0x80) and (ht & 0x1f) not in (2, 3)
                info["device_sigs" if legacy_all else "host_sigs"] += 1
            if witness:
                vins[i].witness = [sigs[0], pubs[0]]
                vins[i].script_sig = b""
            elif redeem is not None:
                vins[i].script_sig = b"\x00" + b"".join(_core.script_push_data(s) for s in sigs) + \
                    _core.script_push_data(redeem)
            else:
                vins[i].script_sig = _core.script_push_data(sigs[0]) + _core.script_push_data(pubs[0])
        tx.vin = vins
        txs.append(tx)
        g += n_in
    info["inputs"] = g
    blk = _core.Block()
    blk.vtx = txs
    return blk, view, height, info


def make_signed_block(n_txs: int, seed: int = 0, witness_every: int = 0, height: int = 1000,
                      bad_at: int | None = None):
    """-> (block, view, height). Every `witness_every`-th spend is P2WPKH (0 = none); with
    `bad_at` the signature of that transaction is corrupted (a block ConnectBlock must reject)."""
    view = _core.CoinsView()
    cb = _core.Transaction()
    cb.version = 1
    cin = _core.TxIn()
    cin.script_sig = _core.script_push_int(height) + b"\x00"
    cb.vin = [cin]
    cb.vout = [_core.TxOut(0, b"\x51")]
    txs = [cb]
    for t in range(n_txs):
        sec = _key(seed, t)
        pub = _core.secp_pubkey_create(sec, True)
        h = _core.hash160(pub)
        witness = witness_every > 0 and t % witness_every == witness_every - 1
        spk = (b"\x00\x14" + h) if witness else (b"\x76\xa9\x14" + h + b"\x88\xac")
        prev = hashlib.sha256(f"prev-{seed}-{t}".encode()).digest()
        value = 50_000 + t
        view.add(prev, 0, value, spk, 1, False)
        tx = _core.Transaction()
        tx.version = 2
        vin = _core.TxIn()
        op = _core.OutPoint()
        op.hash, op.n = prev, 0
        vin.prevout = op
        vin.sequence = 0xffffffff
        tx.vin = [vin]
        tx.vout = [_core.TxOut(value - 1000, b"\x76\xa9\x14" + bytes(20) + b"\x88\xac")]
        raw = tx.serialize(True)
        if witness:
            msg = _core.signature_hash(b"\x76\xa9\x14" + h + b"\x88\xac", raw, 0, 1, value, 1)
        else:
            msg = _core.signature_hash(spk, raw, 0, 1, value, 0)
        sig = bytearray(_core.secp_sign(msg, sec))
        if bad_at == t:
            sig[-3] ^= 0x01  # inside S: still valid DER, wrong signature
        sig = bytes(sig) + b"\x01"
        if witness:
            vin.witness = [sig, pub]
            vin.script_sig = b""
        else:
            vin.script_sig = _core.script_push_data(sig) + _core.script_push_data(pub)
        tx.vin = [vin]
        txs.append(tx)
    blk = _core.Block()
    blk.vtx = txs
    return blk, view, height
