"""KawPow nonce search and batch hashing on one MI355X.

Wraps the per-period gfx950 kernel (hip/kernels/kawpow_search.hip + the
generated program, see ops/jit.py). Reference behaviour: progpow::search /
hash (src/crypto/ethash/lib/ethash/progpow.cpp:357-429, 567-579); unlike the
reference's "first nonce wins" scan, one launch evaluates a whole nonce window
and returns every share whose final hash passes the 64-bit target prefix; the
host then re-checks each share bit-exactly (`Share.verify_host`). While a period's kernel is not
compiled yet the searcher can run the same window on the period-agnostic kernel
(hip/kernels/kawpow_anyperiod.hip, the program as data) instead of waiting: `jit_mode`.

Hashes here are in ethash storage order (the bytes progpow consumes); the
node-level byte reversal of the SHA256d header hash lives in chain/header.py.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import torch

from .. import _core
from . import jit, runtime
from ..utils.trace import traced
from .ethash import DeviceEpoch

SHARE_FMT = "<Q8I8I"
SHARE_SIZE = struct.calcsize(SHARE_FMT)


@dataclass
class Share:
    nonce: int
    mix_hash: bytes   # 32 bytes, storage order
    final_hash: bytes  # 32 bytes, storage order

    def verify_host(self, block_number: int, header_hash: bytes, boundary: bytes | None = None) -> bool:
        """Mix-only recomputation (cheap: the final keccak from the GPU's own mix) + optional full
        256-bit boundary check. A wrong DAG gather or program would pass this; `verify_full` not."""
        fin = _core.kawpow_hash_no_verify(block_number, header_hash, self.mix_hash, self.nonce)
        if fin != self.final_hash:
            return False
        return boundary is None or _core.hash_le(fin, boundary)

    def verify_full(self, block_number: int, header_hash: bytes, boundary: bytes | None = None, ctx=None) -> bool:
        """Full light-mode KawPow on the host (progpow::verify, src/crypto/ethash/lib/ethash/
        progpow.cpp:431-495): recompute mix and final from the epoch's light cache and require both
        to equal what the GPU reported (+ optional 256-bit boundary check)."""
        ctx = ctx if ctx is not None else _core.get_epoch_context(block_number // _core.EPOCH_LENGTH)
        fin, mix = _core.kawpow_hash(ctx, block_number, header_hash, self.nonce)
        if fin != self.final_hash or mix != self.mix_hash:
            return False
        return boundary is None or _core.hash_le(fin, boundary)


def parse_results(raw: bytes, max_shares: int) -> tuple[list[Share], int, int]:
    """(shares sorted by nonce, appended count, skipped workgroups) of one KawpowResults ring."""
    count, skipped = struct.unpack_from("<II", raw, 0)
    shares = []
    for i in range(min(count, max_shares)):
        vals = struct.unpack_from(SHARE_FMT, raw, 16 + i * SHARE_SIZE)
        shares.append(Share(vals[0], struct.pack("<8I", *vals[1:9]), struct.pack("<8I", *vals[9:17])))
    shares.sort(key=lambda s: s.nonce)
    return shares, count, skipped


def target_prefix(boundary: bytes) -> int:
    """Upper 64 bits (big-endian) of a 32-byte boundary, rounded so the GPU
    prefix test never rejects a hash the full compare would accept."""
    return int.from_bytes(boundary[:8], "big")


class KawpowSearcher:
    """Search / hash engine for one (device, epoch, period).

    `jit_mode` (ops/jit.KernelChooser): "wait" blocks in `set_block` until the period's compiled
    kernel exists; "auto" mines on the period-agnostic kernel (hip/kernels/kawpow_anyperiod.hip)
    while the compile runs and swaps to the compiled one between two launches; "off" never
    compiles. `kernel_kind` is the kernel the last launch used ("jit" / "generic")."""

    PROGRAMS_RESIDENT = 8  # periods whose 256-byte program stays on the device

    def __init__(self, epoch_dev: DeviceEpoch, block_number: int, prefetch_next: bool = False,
                 jit_mode: str = "wait"):
        self.prefetch_next = prefetch_next
        self.epoch_dev = epoch_dev
        self.device = epoch_dev.device
        self.h = runtime.hip()
        self.block_number = -1
        self.period = -1
        self.kernel = None
        self.hash_kernel = None
        self.jit_mode = jit_mode
        self.defines = jit.defines_for(epoch_dev.dag_bytes)
        self.granule = jit.granule_for(epoch_dev.dag_bytes)
        self.chooser = jit.KernelChooser(jit_mode, lambda p: jit.ready(p, self.defines),
                                         lambda p: jit.prefetch(p, self.defines))
        self.kernel_kind = "jit" if jit_mode == "wait" else "generic"
        self._kind = self.kernel_kind  # the kernel the next launch will use
        self._programs: dict[int, torch.Tensor] = {}
        self._any = self._any_hash = None
        self._scratch: torch.Tensor | None = None
        nbytes = self.h.sizeof_results()
        with torch.cuda.device(self.device):
            self.results = torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device)
            self.results_host = torch.zeros(nbytes // 4, dtype=torch.int32).pin_memory()
        self.set_block(block_number)

    def set_block(self, block_number: int) -> None:
        if block_number // _core.EPOCH_LENGTH != self.epoch_dev.epoch:
            raise ValueError(f"block {block_number} is not in epoch {self.epoch_dev.epoch}")
        period = block_number // 3
        if period != self.period:
            self._choose(period)
            self.period = period
            if self.prefetch_next and self.jit_mode != "off":
                jit.prefetch(period + 1, self.defines)  # next period compiles while this one mines
        elif self._kind == "generic" and self.jit_mode == "auto":
            self._choose(period)  # swap to the compiled kernel once its compile is done
        self.block_number = block_number

    def _choose(self, period: int) -> None:
        """Ask the chooser which kernel this period runs on now; load what it names. Called from
        `set_block` and at the top of `launch`, so a swap never happens inside a launch."""
        c = self.chooser.choose(period)
        if c.log:
            from ..utils import log

            log.log_printf(c.log)
        with torch.cuda.device(self.device):
            if c.kind == "jit":
                co = runtime.load_code_object(c.path, key=c.path)
                kernel = co.function("kawpow_search")
                if self.jit_mode != "wait" and int(kernel.max_threads) != self.granule:
                    raise RuntimeError(f"{c.path}: block {kernel.max_threads} is not the launch granule {self.granule}")
                self.kernel, self.hash_kernel = kernel, co.function("kawpow_hash_batch")
            else:
                if self._any is None:
                    self._any = runtime.static_kernel("kawpow_anyperiod", "kawpow_search_any")
                    self._any_hash = runtime.static_kernel("kawpow_anyperiod", "kawpow_hash_any")
                self._program(period)
                self.kernel = self.hash_kernel = None  # an earlier period's compiled kernel is not this one's
        self._kind = c.kind

    def _program(self, period: int) -> torch.Tensor:
        """The period's 64 program words on the device (uploaded once, the last few kept)."""
        t = self._programs.get(period)
        if t is None:
            raw = _core.kawpow_programs_bytes([period])
            assert len(raw) == 256
            t = torch.frombuffer(bytearray(raw), dtype=torch.int32).to(self.device)
            self._programs[period] = t
            while len(self._programs) > self.PROGRAMS_RESIDENT:
                self._programs.pop(next(iter(self._programs)))
        return t

    @property
    def block(self) -> int:
        """The nonce granularity of a launch: threads per workgroup of the compiled variant, which
        the period-agnostic kernel covers per workgroup too (ops/jit.granule_for)."""
        if self.jit_mode == "wait":
            return int(self.kernel.max_threads)
        return self.granule

    # ------------------------------------------------------------------
    def launch(self, header_hash: bytes, start_nonce: int, num_nonces: int, target64: int,
               stream: int | None = None, results: torch.Tensor | None = None, gen_word: int = 0,
               generation: int = 0) -> None:
        """Queue one search window on `stream` (no host sync). `results`: the share ring to append
        to (default: this searcher's own; the caller clears a ring it passes). `gen_word`: host-mapped
        generation word; workgroups that start after it moved past `generation` search nothing."""
        if self._kind == "generic" and self.jit_mode == "auto":
            self._choose(self.period)  # the compile may have finished since set_block
        if num_nonces % self.block:
            raise ValueError(f"num_nonces must be a multiple of {self.block}")
        with torch.cuda.device(self.device):
            s = runtime.current_stream_handle() if stream is None else stream
            if results is None:
                results = self.results
                results[:4].zero_()
            if self._kind == "generic":
                self.h.launch_kawpow_search_any(self._any, self.epoch_dev.dag.data_ptr(), self.epoch_dev.items2048,
                                                results.data_ptr(), header_hash, start_nonce, target64, num_nonces, s,
                                                self._program(self.period).data_ptr(), self.epoch_dev.l1.data_ptr(),
                                                self.granule, gen_word, generation)
            else:
                scratch = self.scratch(num_nonces)
                self.h.launch_kawpow_search(self.kernel, self.epoch_dev.dag.data_ptr(), self.epoch_dev.items2048,
                                            results.data_ptr(), header_hash, start_nonce, target64, num_nonces, s,
                                            scratch.data_ptr(), scratch.numel() * 4, gen_word, generation)
        self.kernel_kind = self._kind

    def scratch(self, num_nonces: int) -> torch.Tensor:
        """Per-nonce digest parking space (8 words/nonce) for the launch; grown on demand.
        Reused across launches: kernels on one stream are ordered."""
        need = num_nonces * 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.int32, device=self.device)
        return self._scratch

    def collect(self) -> list[Share]:
        """Copy the share ring back (synchronises the current stream)."""
        with torch.cuda.device(self.device):
            self.results_host.copy_(self.results, non_blocking=False)
        return parse_results(self.results_host.numpy().tobytes(), self.h.KAWPOW_MAX_SHARES)[0]

    @traced("kawpow.search")
    def search(self, header_hash: bytes, start_nonce: int, num_nonces: int, boundary: bytes) -> list[Share]:
        """All shares in [start, start+num) with final <= boundary (bit-exact, host-checked).
        The launch is rounded up to whole workgroups; shares past the window are dropped. Nonces
        count mod 2^64, as the kernel's do: a window may run past 2^64 - 1 and go on from 0."""
        padded = -(-num_nonces // self.block) * self.block
        self.launch(header_hash, start_nonce, padded, target_prefix(boundary))
        return [s for s in self.collect()
                if (s.nonce - start_nonce) & 0xFFFFFFFFFFFFFFFF < num_nonces and _core.hash_le(s.final_hash, boundary)]

    def hash_batch(self, header_hashes: list[bytes], nonces: list[int]) -> list[tuple[bytes, bytes]]:
        """(final, mix) for each (header, nonce) at this searcher's block height."""
        n = len(nonces)
        if n == 0:
            return []
        job = struct.Struct("<8IQII")
        buf = bytearray(job.size * n)
        for i, (hh, nonce) in enumerate(zip(header_hashes, nonces)):
            job.pack_into(buf, i * job.size, *struct.unpack("<8I", hh), nonce, self.block_number, 0)
        with torch.cuda.device(self.device):
            jobs = torch.frombuffer(buf, dtype=torch.uint8).to(self.device)
            out = torch.empty(n * 16, dtype=torch.int32, device=self.device)
            if self._kind == "generic":
                self.h.launch_kawpow_hash_any(self._any_hash, self.epoch_dev.dag.data_ptr(), self.epoch_dev.items2048,
                                              jobs.data_ptr(), n, out.data_ptr(), self._program(self.period).data_ptr(),
                                              self.epoch_dev.l1.data_ptr(), runtime.current_stream_handle())
            else:
                self.h.launch_kawpow_hash_batch(self.hash_kernel, self.epoch_dev.dag.data_ptr(),
                                                self.epoch_dev.items2048, jobs.data_ptr(), n, out.data_ptr(),
                                                runtime.current_stream_handle())
            raw = out.cpu().numpy().tobytes()
        res = []
        for i in range(n):
            mix = raw[i * 64:i * 64 + 32]
            fin = raw[i * 64 + 32:i * 64 + 64]
            res.append((fin, mix))
        return res
