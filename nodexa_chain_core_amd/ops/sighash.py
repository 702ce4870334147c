"""Legacy signature hashes on the GPU (hip/kernels/sighash.hip), feeding the batch ECDSA verifier.

The reference computes SignatureHash (src/script/interpreter.cpp) on the host once per signature;
for a legacy input that re-serialises and double-SHA-256es the whole transaction, so a transaction
with many inputs costs quadratic work before a single signature is checked. With
`connect_block(defer_sigs=True, defer_sighash=True)` the native core leaves those hashes out and
`ConnectResult.sighash_pack()` lays the block out as one arena (one blanked template per
transaction, one script code and hash type per signature) plus a job table of four (offset, length)
segments per signature. `sighash_gather_batch` hashes one job per lane and writes the digest
straight into the `z` limbs of the packed secp job, whose `kind` it sets in the same pass:
the records are uploaded INVALID, so a signature the kernel never reached can only fail.

`digests` is the kernel on its own; `verify_block_sigs` is the block path: gather, then
`secp_verify_batch` on the same stream, verdicts only coming back.

A block connected with `defer_all_forms=True` leaves every form of both signature versions out
(NONE, SINGLE, ANYONECANPAY, witness v0). `ConnectResult.sighash_pack_var()` names each message
through a table of up to SIGHASH_VAR_MAX_SEGMENTS arena ranges and `sighash_gather_var`
(hip/kernels/sighash_var.hip) hashes them; `digests_var` and `gather_var_into_secp` are that
kernel on its own, and `verify_block_sigs` takes this path for such a result.

`verify_window` is the same pass over a run of consecutive blocks (-gpusigwindow):
`_core.sig_window_pack` concatenates the blocks' tables, the gather and the verifier run once over
all of them, and `sig_window_verdicts` (hip/kernels/sig_window.hip) condenses the verdicts to one
16-byte record per block, the only thing that comes back while every signature is valid.
`verdict_records` is that kernel on its own.

A result connected with `defer_multisig=True` carries CHECKMULTISIG groups (`res.sig_groups`): all
candidate (signature, key) pairs of the opcode's walk are entries of the batch.
`sig_group_resolve` (hip/kernels/sig_group.hip) runs between the verifier and
`sig_window_verdicts`, on the same stream, and rewrites each group's verdicts to the outcome of
its walk, so an entry is True if its signature is valid, or if its group's walk succeeded.
`resolve_groups` is that kernel on its own.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _core
from ..utils.trace import traced
from . import runtime, secp

JOB_BYTES = _core.SIGHASH_JOB_BYTES
VAR_JOB_BYTES = _core.SIGHASH_VAR_JOB_BYTES
SEG_BYTES = _core.SIGHASH_SEG_BYTES


def _upload_arena(arena: bytes, dev: torch.device) -> torch.Tensor:
    """The arena on the device, followed by the zeroed slack the kernel's aligned dword reads may touch."""
    buf = bytearray(arena)
    buf += bytes((-len(buf)) % 4 + _core.SIGHASH_ARENA_SLACK)
    return torch.frombuffer(buf, dtype=torch.uint8).to(dev)


def _upload_jobs(arena: bytes, jobs: bytes, n_out: int, dev: torch.device):
    # nothing malformed reaches the device: every segment inside the arena, every output in range
    _core.sighash_check_jobs(len(arena), jobs, n_out)
    return _upload_arena(arena, dev), torch.frombuffer(bytearray(jobs), dtype=torch.int32).to(dev)


def _device(device: int | None) -> torch.device:
    return torch.device("cuda", torch.cuda.current_device() if device is None else int(device))


def digests(arena: bytes, jobs: bytes, device: int | None = None) -> np.ndarray:
    """(n, 32) uint8: SHA256d of each job's four arena segments, row = the job's output index
    (which must be below the job count). Equals `_core.sighash_gather_model` row for row when the
    output indices are 0..n-1."""
    n = len(jobs) // JOB_BYTES
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    runtime.require_gpu()
    dev = _device(device)
    with torch.cuda.device(dev):
        d_arena, d_jobs = _upload_jobs(arena, jobs, n, dev)
        out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        runtime.hip().launch_sighash_gather(runtime.static_kernel("sighash", "sighash_gather_batch"),
                                            d_arena.data_ptr(), d_jobs.data_ptr(), n, out.data_ptr(), 0,
                                            runtime.current_stream_handle())
        return out.cpu().numpy()


def gather_into_secp(arena: bytes, jobs: bytes, secp_jobs: bytes, device: int | None = None) -> bytes:
    """Run the gather over a packed SecpVerifyJob array and return the array as the device holds it
    afterwards: the records the job table names carry their z limbs and real kind, all others are
    untouched."""
    n = len(jobs) // JOB_BYTES
    n_secp = len(secp_jobs) // _core.SECP_JOB_BYTES
    if n == 0:
        return bytes(secp_jobs)
    runtime.require_gpu()
    dev = _device(device)
    with torch.cuda.device(dev):
        d_arena, d_jobs = _upload_jobs(arena, jobs, n_secp, dev)
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        runtime.hip().launch_sighash_gather(runtime.static_kernel("sighash", "sighash_gather_batch"),
                                            d_arena.data_ptr(), d_jobs.data_ptr(), n, 0, d_secp.data_ptr(),
                                            runtime.current_stream_handle())
        return d_secp.cpu().numpy().tobytes()


def _upload_var(arena: bytes, segs: bytes, jobs: bytes, n_out: int, dev: torch.device):
    # nothing malformed reaches the device: every segment inside the arena, every job inside the
    # segment table, every output in range
    _core.sighash_var_check(len(arena), segs, jobs, n_out)
    # a job table may name no segment at all: the kernel still gets a valid (unread) table
    d_segs = torch.frombuffer(bytearray(segs or bytes(SEG_BYTES)), dtype=torch.int32).to(dev)
    return _upload_arena(arena, dev), d_segs, torch.frombuffer(bytearray(jobs), dtype=torch.int32).to(dev)


def digests_var(arena: bytes, segs: bytes, jobs: bytes, device: int | None = None) -> np.ndarray:
    """(n, 32) uint8: SHA256d of each job's segments in order, row = the job's output index (which
    must be below the job count). Equals `_core.sighash_var_model` row for row when the output
    indices are 0..n-1."""
    n = len(jobs) // VAR_JOB_BYTES
    if n == 0:
        _core.sighash_var_check(len(arena), segs, jobs, 0)
        return np.zeros((0, 32), np.uint8)
    runtime.require_gpu()
    dev = _device(device)
    with torch.cuda.device(dev):
        d_arena, d_segs, d_jobs = _upload_var(arena, segs, jobs, n, dev)
        out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        runtime.hip().launch_sighash_gather_var(runtime.static_kernel("sighash_var", "sighash_gather_var"),
                                                d_arena.data_ptr(), d_segs.data_ptr(), len(segs) // SEG_BYTES,
                                                d_jobs.data_ptr(), n, out.data_ptr(), 0,
                                                runtime.current_stream_handle())
        return out.cpu().numpy()


def gather_var_into_secp(arena: bytes, segs: bytes, jobs: bytes, secp_jobs: bytes, device: int | None = None) -> bytes:
    """`gather_into_secp` for a segment-table job set: the SecpVerifyJob array as the device holds
    it after sighash_gather_var."""
    n = len(jobs) // VAR_JOB_BYTES
    n_secp = len(secp_jobs) // _core.SECP_JOB_BYTES
    if n == 0:
        return bytes(secp_jobs)
    runtime.require_gpu()
    dev = _device(device)
    with torch.cuda.device(dev):
        d_arena, d_segs, d_jobs = _upload_var(arena, segs, jobs, n_secp, dev)
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        runtime.hip().launch_sighash_gather_var(runtime.static_kernel("sighash_var", "sighash_gather_var"),
                                                d_arena.data_ptr(), d_segs.data_ptr(), len(segs) // SEG_BYTES,
                                                d_jobs.data_ptr(), n, 0, d_secp.data_ptr(),
                                                runtime.current_stream_handle())
        return d_secp.cpu().numpy().tobytes()


GROUP_BYTES = _core.SIG_GROUP_BYTES


def _launch_groups(h, d_out: torch.Tensor, n: int, table: bytes, dev: torch.device, stream) -> None:
    """sig_group_resolve over the verifier's out[] in place; nothing malformed reaches the device."""
    _core.sig_group_check(n, table)
    if not table:
        return
    d_groups = torch.frombuffer(bytearray(table), dtype=torch.int32).to(dev)
    h.launch_sig_group_resolve(runtime.static_kernel("sig_group", "sig_group_resolve"), d_out.data_ptr(),
                               d_groups.data_ptr(), len(table) // GROUP_BYTES, stream)


def resolve_groups(verdicts, table: bytes, device: int | None = None) -> list[int]:
    """`sig_group_resolve` on its own: the verdict array with every group's entries rewritten to the
    outcome of its CHECKMULTISIG walk. Equals `_core.sig_group_resolve_model(verdicts, table)`."""
    v = np.asarray(verdicts, dtype=np.uint32)
    _core.sig_group_check(len(v), table)
    if not table:
        return [int(x) for x in v]
    runtime.require_gpu()
    dev = _device(device)
    with torch.cuda.device(dev):
        d_out = torch.from_numpy(v.view(np.int32).copy()).to(dev)
        _launch_groups(runtime.hip(), d_out, len(v), table, dev, runtime.current_stream_handle())
        return [int(x) for x in d_out.cpu().numpy().view(np.uint32)]


@traced("sighash.verify_block_sigs")
def verify_block_sigs(res, device: int | None = None) -> list[bool]:
    """CPubKey::Verify's answer for every deferred signature of a `connect_block(defer_sigs=True,
    defer_sighash=True)` result (with or without `defer_all_forms`), in the order of
    `res.sig_items()`. The message hashes left to the
    batch are computed on the device and never come back; only the verdicts do. A verdict 2
    (degenerate addition) is re-checked on the host with the host-computed message. With
    `defer_multisig` groups in the result, an entry is True if its signature is valid, or if its
    group's CHECKMULTISIG walk succeeded."""
    n = res.num_sigs
    if n == 0:
        return []
    runtime.require_gpu()
    h = runtime.hip()
    dev = _device(device)
    var = res.all_forms
    if var:
        arena, segs, jobs, secp_jobs, n_dev, _n_host = res.sighash_pack_var()
    else:
        arena, jobs, secp_jobs, n_dev, _n_host = res.sighash_pack()
    with torch.cuda.device(dev):
        stream = runtime.current_stream_handle()
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        gtab = secp._gen_table(dev)  # uploaded on first use: before the launches, not between them
        if n_dev and var:
            d_arena, d_segs, d_jobs = _upload_var(arena, segs, jobs, n, dev)
            h.launch_sighash_gather_var(runtime.static_kernel("sighash_var", "sighash_gather_var"), d_arena.data_ptr(),
                                        d_segs.data_ptr(), len(segs) // SEG_BYTES, d_jobs.data_ptr(), n_dev, 0,
                                        d_secp.data_ptr(), stream)
        elif n_dev:
            d_arena, d_jobs = _upload_jobs(arena, jobs, n, dev)
            h.launch_sighash_gather(runtime.static_kernel("sighash", "sighash_gather_batch"), d_arena.data_ptr(),
                                    d_jobs.data_ptr(), n_dev, 0, d_secp.data_ptr(), stream)
        h.launch_secp_verify(runtime.static_kernel("secp256k1_verify", "secp_verify_batch"), d_secp.data_ptr(), n,
                             gtab.data_ptr(), out.data_ptr(), stream)
        _launch_groups(h, out, n, res.sig_group_table(), dev, stream)
        verdicts = out.cpu().tolist()
    if 2 in verdicts:
        items = res.sig_items()
        return [bool(_core.secp_verify(*items[k])) if v == 2 else v == 1 for k, v in enumerate(verdicts)]
    return [v == 1 for v in verdicts]


# ---------------------------------------------------------------- a window of consecutive blocks
RECORD_BYTES = _core.SIG_WINDOW_RECORD_BYTES
NONE = _core.SIG_WINDOW_NONE


def _check_sig_begin(sig_begin, n: int) -> np.ndarray:
    """The prefix table as the kernel reads it; nothing malformed reaches the device."""
    sb = np.asarray(sig_begin, dtype=np.int64)
    if sb.ndim != 1 or len(sb) < 1 or sb[0] < 0 or np.any(np.diff(sb) < 0) or sb[-1] > n or n >= 1 << 31:
        raise ValueError("signature window: the prefix table does not fit the verdicts")
    return sb.astype(np.uint32)


def _launch_records(h, d_out: torch.Tensor, sig_begin: np.ndarray, dev: torch.device, stream) -> torch.Tensor:
    nb = len(sig_begin) - 1
    d_begin = torch.from_numpy(sig_begin.view(np.int32).copy()).to(dev)
    records = torch.empty((nb, RECORD_BYTES // 4), dtype=torch.int32, device=dev)
    h.launch_sig_window_verdicts(runtime.static_kernel("sig_window", "sig_window_verdicts"), d_out.data_ptr(),
                                 d_begin.data_ptr(), nb, records.data_ptr(), stream)
    return records


def verdict_records(verdicts, sig_begin, device: int | None = None) -> bytes:
    """`sig_window_verdicts` on its own: the per-block records of a verdict array, as raw bytes.
    Equals `_core.sig_window_verdicts_model(verdicts, sig_begin)` byte for byte."""
    v = np.asarray(verdicts, dtype=np.uint32)
    sb = _check_sig_begin(sig_begin, len(v))
    if len(sb) == 1:
        return b""
    runtime.require_gpu()
    dev = _device(device)
    with torch.cuda.device(dev):
        # an empty verdict array still gets a valid (unread) buffer
        d_out = torch.from_numpy(np.concatenate([v, np.zeros(1, np.uint32)]).view(np.int32)).to(dev)
        rec = _launch_records(runtime.hip(), d_out, sb, dev, runtime.current_stream_handle())
        return rec.cpu().numpy().tobytes()


def _window_pass(results, device: int | None):
    """One pack, one upload of each table, gather (if any hash is left to the device),
    secp_verify_batch, sig_group_resolve (if any result carries groups), sig_window_verdicts: ->
    (records (nb, 4) uint32, verdicts on the device, sig_begin), or None for a window without
    signatures, which launches nothing."""
    mode, arena, segs, jobs, secp_jobs, sig_begin, n_dev, _n_host = _core.sig_window_pack(list(results))
    n = sig_begin[-1]
    if n == 0:
        return None
    runtime.require_gpu()
    h = runtime.hip()
    dev = _device(device)
    sb = _check_sig_begin(sig_begin, n)
    with torch.cuda.device(dev):
        stream = runtime.current_stream_handle()
        d_secp = torch.frombuffer(bytearray(secp_jobs), dtype=torch.int32).to(dev)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        gtab = secp._gen_table(dev)  # uploaded on first use: before the launches, not between them
        if n_dev and mode == 2:
            d_arena, d_segs, d_jobs = _upload_var(arena, segs, jobs, n, dev)
            h.launch_sighash_gather_var(runtime.static_kernel("sighash_var", "sighash_gather_var"), d_arena.data_ptr(),
                                        d_segs.data_ptr(), len(segs) // SEG_BYTES, d_jobs.data_ptr(), n_dev, 0,
                                        d_secp.data_ptr(), stream)
        elif n_dev:
            d_arena, d_jobs = _upload_jobs(arena, jobs, n, dev)
            h.launch_sighash_gather(runtime.static_kernel("sighash", "sighash_gather_batch"), d_arena.data_ptr(),
                                    d_jobs.data_ptr(), n_dev, 0, d_secp.data_ptr(), stream)
        h.launch_secp_verify(runtime.static_kernel("secp256k1_verify", "secp_verify_batch"), d_secp.data_ptr(), n,
                             gtab.data_ptr(), out.data_ptr(), stream)
        _launch_groups(h, out, n, _core.sig_window_groups(list(results)), dev, stream)
        records = _launch_records(h, out, sb, dev, stream).cpu().numpy().view(np.uint32)
    return records, out, sb


def window_records(results, device: int | None = None) -> list[tuple[int, int, int, int]]:
    """The raw per-block records of `verify_window`'s device pass: (n_valid, n_invalid,
    n_ask_host, first_not_valid) for each result, first_not_valid relative to the block's first
    signature and SIG_WINDOW_NONE when every verdict is valid."""
    got = _window_pass(results, device)
    if got is None:
        return [(0, 0, 0, NONE) for _ in results]
    return [tuple(int(x) for x in row) for row in got[0]]


@traced("sighash.verify_window")
def verify_window(results, device: int | None = None) -> list[list[bool]]:
    """CPubKey::Verify's answer for every deferred signature of a run of consecutive blocks'
    `connect_block(defer_sigs=True, ...)` results, verified in one device pass: entry b equals what
    `verify_block_sigs(results[b])` (or `secp.verify_batch(results[b].sig_items())` for a result
    whose hashes came from the host) returns. All results are of one -gpusighash mode. Only one
    16-byte record per block comes back; the verdicts of a block are fetched when its record shows
    one that is not valid, and a verdict 2 is re-checked on the host with the host-computed message.
    Groups (`defer_multisig`) are resolved on the device before the records are made."""
    got = _window_pass(results, device)
    if got is None:
        return [[] for _ in results]
    records, out, sb = got
    answers = []
    for b, res in enumerate(results):
        lo, hi = int(sb[b]), int(sb[b + 1])
        if records[b][3] == NONE and records[b][0] == hi - lo:
            answers.append([True] * (hi - lo))
            continue
        verdicts = out[lo:hi].cpu().tolist()
        if 2 in verdicts:
            items = res.sig_items()
            answers.append([bool(_core.secp_verify(*items[k])) if v == 2 else v == 1 for k, v in enumerate(verdicts)])
        else:
            answers.append([v == 1 for v in verdicts])
    return answers
