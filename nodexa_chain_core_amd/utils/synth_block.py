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


def _multisig_key(seed: int, gi: int, k: int) -> bytes:
    # the first three keys of an input are the ones its 2-of-3 has always had
    return _key(seed, 3 * gi + k) if k < 3 else _key(seed, (1 << 24) + 32 * gi + k)


def make_consolidation_block(n_txs: int, inputs_per_tx, seed: int = 0, hash_types=(1,), witness_every: int = 0,
                             multisig_every: int = 0, bad_at: int | None = None, height: int = 1000,
                             multisig_mn=(2, 3), multisig_signers=None, multisig_kind: str = "p2sh"):
    """-> (block, view, height, info): `n_txs` transactions that each spend many seeded coins into
    two outputs, the shape whose legacy signature hashes cost the host quadratic work.

    `inputs_per_tx` is a count, or a (low, high) pair from which each transaction's count is drawn
    with the seed. Inputs are numbered through the block (0 = first input of the first
    transaction); input g signs with hash_types[g % len(hash_types)], is P2WPKH when
    `witness_every` divides g + 1, else P2SH 2-of-3 when `multisig_every` divides g + 1 (two
    signatures), else P2PKH. With `bad_at`, the first signature of that input is corrupted.
    The multisig inputs are m-of-n for `multisig_mn` = (m, n), paid to a script hash ("p2sh"), to the
    bare script ("bare") or to a witness script hash ("p2wsh") as `multisig_kind` says.
    `multisig_signers` names the keys that sign, by their index in the script: None for the last m,
    a tuple of m indices for the same keys in every input, or "cycle" for every m-subset in turn, one
    per multisig input. Signatures are pushed in key order, as CHECKMULTISIG demands.
    `info` counts what the block implies: "inputs", "sigs", "device_sigs" (legacy signatures whose
    hash has the SIGHASH_ALL form: no ANYONECANPAY, base type neither NONE nor SINGLE),
    "host_sigs" (the rest), and "bad_sig" (index of the corrupted signature among "sigs", where
    CHECKMULTISIG's walk meets every signature's key at the first try: the last m keys signing)."""
    import itertools
    import random

    ms_m, ms_n = multisig_mn
    if multisig_kind not in ("p2sh", "bare", "p2wsh"):
        raise ValueError("multisig_kind: p2sh, bare or p2wsh")
    if multisig_signers is None:
        subsets = [tuple(range(ms_n - ms_m, ms_n))]
    elif multisig_signers == "cycle":
        subsets = list(itertools.combinations(range(ms_n), ms_m))
    else:
        subsets = [tuple(sorted(multisig_signers))]
        if len(set(subsets[0])) != ms_m or not all(0 <= j < ms_n for j in subsets[0]):
            raise ValueError("multisig_signers: m distinct key indices below n")
    n_multisig = 0

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
            secs = [_multisig_key(seed, gi, k) for k in range(ms_n)] if multisig else [_key(seed, 3 * gi)]
            pubs = [_core.secp_pubkey_create(s, True) for s in secs]
            if multisig:
                redeem = _core.script_push_int(ms_m) + b"".join(_core.script_push_data(p) for p in pubs) + \
                    _core.script_push_int(ms_n) + b"\xae"
                code = redeem
                if multisig_kind == "p2sh":
                    spk = b"\xa9\x14" + _core.hash160(redeem) + b"\x87"
                elif multisig_kind == "bare":
                    spk = redeem
                else:
                    spk = b"\x00\x20" + hashlib.sha256(redeem).digest()
                    witness = True  # signs the BIP143 hash
                secs = [secs[j] for j in subsets[n_multisig % len(subsets)]]
                n_multisig += 1
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
            # m-of-n: by default the last m keys sign, so that CHECKMULTISIG's walk (last signature
            # against last key first) meets every signature's key at the first try. A deferring
            # checker without defer_multisig tries no other key: any other choice of signers
            # (multisig_signers) sends the input to the host re-check there
            for k, sec in enumerate(secs):
                sig = bytearray(_core.secp_sign(msg, sec))
                if bad_at == g + i and k == 0:
                    sig[-3] ^= 0x01  # inside S: still valid DER, wrong signature
                    # position in connect_block's deferred order, where a multisig input's
                    # signatures come last first
                    info["bad_sig"] = info["sigs"] + (len(secs) - 1 if redeem is not None else 0)
                sigs.append(bytes(sig) + bytes([ht & 0xff]))
                info["sigs"] += 1
                legacy_all = not witness and not (ht & 0x80) and (ht & 0x1f) not in (2, 3)
                info["device_sigs" if legacy_all else "host_sigs"] += 1
            if witness and redeem is not None:
                vins[i].witness = [b""] + sigs + [redeem]
                vins[i].script_sig = b""
            elif witness:
                vins[i].witness = [sigs[0], pubs[0]]
                vins[i].script_sig = b""
            elif redeem is not None:
                vins[i].script_sig = b"\x00" + b"".join(_core.script_push_data(s) for s in sigs) + \
                    (_core.script_push_data(redeem) if multisig_kind == "p2sh" else b"")
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
