"""Pipelined nonce search on one device — the loop the node mines with and bench.py times.

Reference behaviour: the miner's inner loop (CloreMiner, src/miner.cpp:566-726: search, check
for a stale tip, count hashes), progpow::search (src/crypto/ethash/lib/ethash/progpow.cpp:
553-579) and generateBlocks' legacy nNonce scan (src/rpc/mining.cpp:141-149). One work packet
format and one two-slot device protocol carry every proof of work the chain knows:

* **KawPow** (GpuSearchDevice / CpuSearchDevice). Each GPU launch searches 2^25 nonces (~120 ms at
  epoch 384: ~43k workgroups, far past the 512 that fill the chip). The device owns two share
  rings; the host queues window k+1 before it reads window k, and each ring is copied to pinned
  host memory on the search stream right behind its kernel, so the GPU is never idle waiting for
  the host. Every launch carries a generation number that the kernel reads once per workgroup from
  a host-mapped word: `abort()` bumps it when the template changes, so queued work of the old
  template stops within one workgroup's lifetime (~1.4 ms). The kernel tests the top 64 bits of the
  final hash; the host applies the full 256-bit boundary and the leader fully re-hashes a share
  (light mode) before it builds a block from it (service.ChainLeader).
* **Equihash(200,9)** (miner/equihash_search.py). A window is `count` nonce256 values
  (le64(nonce) || 24 zero bytes) appended to the 80-byte header prefix; the GPU solves them in one
  launch sequence, verifies every solution on the device and the host keeps the solutions whose
  SHA256d(header) meets the boundary.
* **X16R / X16RV2** (LegacyGpuDevice on a GPU rank, LegacyHostDevice otherwise): templates before
  the KawPow activation (the default on regtest) scan the 32-bit nNonce, 2^20 nonces per GPU
  window (hip/kernels/x16r.hip, search mode) or 2^16 on the host cores (csrc/pow/x16r.cpp).

`RankDevice` routes each slot to the device of its work packet's algorithm, so one loop, one set
of collectives and one failure path serve every era of the chain; `FaultInjectingDevice`
(-gpufailrate / -dropshare) and `HangingDevice` wrap any of them for the failure tests.
"""
from __future__ import annotations

import hashlib
import struct
import threading
import time
from dataclasses import dataclass, field

from .. import core

_core = core()

# Work packet (collective #1): broadcast from rank 0 on every step of the mining loop.
#   header 80 (KawPow: the header hash in bytes 0..31; Equihash: the 80-byte CKAWPOWInput-layout
#   prefix the nonce256 is appended to; X16R: the 80-byte legacy header with nNonce 0) |
#   boundary 32 (big-endian 256-bit target) | height u32 | algo u32 | job_id u64 |
#   nonce_base u64 | flags u64  = 144 bytes
WORK_FMT = "<80s32sIIQQQ"
WORK_SIZE = struct.calcsize(WORK_FMT)
assert WORK_SIZE == 144

FLAG_IDLE = 1    # nothing to mine: drain and wait for the next packet
FLAG_STOP = 2    # leave the mining loop
FLAG_CLEAN = 4   # the previous job is stale: abort its queued work
FLAG_REFORM = 8  # drain, then make the world again over the members named under the rendezvous store's
#                  key "m<nonce_base>/members" (parallel/world.reform): a lost rank comes back
# bits 8..15 of the flags: rank_shift s. Rank r owns [nonce_base + (r << s), nonce_base + ((r + 1) << s));
# 0 (every packet without a pool-assigned nonce prefix) means 56 and an unbounded cursor, as ever
RANK_SHIFT_LSB, RANK_SHIFT_MASK, RANK_SHIFT_DEFAULT = 8, 0xFF00, 56

ALGO_KAWPOW, ALGO_EQUIHASH, ALGO_X16R, ALGO_X16RV2 = 0, 1, 2, 3
ALGO_NAMES = ("kawpow", "equihash", "x16r", "x16rv2")

EPOCH_PREBUILD_WINDOW = 120  # blocks before an epoch boundary at which the next DAG is prebuilt
LEGACY_WINDOW = 1 << 16      # nNonce values per host X16R window
LEGACY_GPU_WINDOW = 1 << 20  # nNonce values per GPU X16R window (~0.6 ms at 1.9 M hashes/s)
EQ_SOLUTION_PREFIX = b"\xfd\x40\x05"  # CompactSize(1344) in front of the packed solution


@dataclass(frozen=True)
class Work:
    header: bytes = bytes(80)
    boundary: bytes = bytes(32)      # share/block target, big-endian
    height: int = 0
    job_id: int = 0
    nonce_base: int = 0
    flags: int = FLAG_IDLE
    algo: int = ALGO_KAWPOW

    def __post_init__(self):
        if len(self.header) != 80:
            object.__setattr__(self, "header", bytes(self.header)[:80].ljust(80, b"\0"))

    @property
    def header_hash(self) -> bytes:
        """KawPow header hash (progpow storage order)."""
        return self.header[:32]

    @property
    def epoch(self) -> int:
        return self.height // _core.EPOCH_LENGTH

    @property
    def idle(self) -> bool:
        return bool(self.flags & (FLAG_IDLE | FLAG_STOP))

    @property
    def stop(self) -> bool:
        return bool(self.flags & FLAG_STOP)

    @property
    def rank_shift(self) -> int:
        return (self.flags & RANK_SHIFT_MASK) >> RANK_SHIFT_LSB or RANK_SHIFT_DEFAULT

    @property
    def rank_bounded(self) -> bool:
        """The packet names its rank_shift: a rank's windows end where its range ends."""
        return bool(self.flags & RANK_SHIFT_MASK)

    def pack(self) -> bytes:
        return struct.pack(WORK_FMT, self.header, self.boundary, self.height, self.algo, self.job_id,
                           self.nonce_base, self.flags)

    @classmethod
    def unpack(cls, raw: bytes) -> "Work":
        hdr, b, height, algo, job, base, flags = struct.unpack(WORK_FMT, raw)
        return cls(hdr, b, height, job, base, flags, algo)

    def target64(self) -> int:
        """Upper 64 bits of the boundary: the kernel's prefix test never rejects a hash the full
        256-bit compare would accept."""
        return int.from_bytes(self.boundary[:8], "big")

    def target(self) -> int:
        return int.from_bytes(self.boundary, "big")


def rank_shift_flags(shift: int) -> int:
    """The flag bits that carry rank_shift `shift` (1..64 - 1)."""
    if not 0 < int(shift) < 64:
        raise ValueError(f"rank_shift {shift} out of range")
    return int(shift) << RANK_SHIFT_LSB


def equihash_nonce256(nonce: int) -> bytes:
    """The nonce256 a window's 64-bit nonce stands for (the rest of the space is left unused)."""
    return struct.pack("<Q", nonce & 0xFFFFFFFFFFFFFFFF) + bytes(24)


def equihash_block_hash(prefix80: bytes, nonce: int, solution: bytes) -> bytes:
    """SHA256d of the serialized extended header (storage order, as uint256): the Equihash
    extension's block hash (csrc/chain/primitives.cpp BlockHeader::equihash_hash)."""
    ser = prefix80 + equihash_nonce256(nonce) + EQ_SOLUTION_PREFIX + solution
    return hashlib.sha256(hashlib.sha256(ser).digest()).digest()


@dataclass
class EquihashShare:
    nonce: int           # the 64-bit nonce of equihash_nonce256
    solution: bytes      # 1344-byte packed solution
    block_hash: bytes    # SHA256d(header), storage order

    def nonce256(self) -> bytes:
        return equihash_nonce256(self.nonce)


@dataclass
class LegacyShare:
    nonce: int           # 32-bit nNonce
    block_hash: bytes    # X16R / X16RV2 hash, storage order


@dataclass
class SlotResult:
    """One finished window: the shares that pass the full 256-bit boundary and the work that was
    actually done (nonces hashed; Equihash: solutions found). An aborted window counts only the
    workgroups that ran; `aborted` is the number that did not."""
    job_id: int
    start: int
    count: int
    hashes: int
    shares: list = field(default_factory=list)
    device_ms: float = 0.0
    aborted: int = 0
    algo: int = ALGO_KAWPOW
    end_ms: float = 0.0  # device clock: the window's end, ms after the device's first window began
    kernel: str = ""     # KawPow on a GPU: "jit" (per-period compiled kernel) or "generic" (period-agnostic)
    dropped: int = 0     # hits the device found but its share ring had no room for


class DeviceHung(RuntimeError):
    """A window did not finish within the watchdog limit."""


class DeviceFault(RuntimeError):
    """A window failed on the device (a kernel error, a lost device, an injected fault)."""


def dag_build_mode(resident_by_rank, pending_by_rank, epoch: int) -> str:
    """How a rank that lacks `epoch`'s DAG builds it in a world that shares DAG builds.

    "collective": sharded over the ranks and all-gathered; right only when every rank builds on the
    same step, that is when no rank of the current world has the epoch resident or pending.
    "solo": this rank builds the whole DAG alone, because a peer already holds the epoch or is
    building it (a rank that joined late; its peers would never enter the all-gather).
    `resident_by_rank` / `pending_by_rank`: per rank of the current world, the epochs it holds / is
    building, as the last gathered records told (the same on every rank). None for the first: this
    rank joined a running world and has seen no records yet; it assumes that its peers hold the
    epoch."""
    if resident_by_rank is None:
        return "solo"
    pending_by_rank = pending_by_rank or [()] * len(resident_by_rank)
    for res, pend in zip(resident_by_rank, pending_by_rank):
        if epoch in res or epoch in pend:
            return "solo"
    return "collective"


class WorldEpochView:
    """What one rank knows of the DAGs of every rank of its world: the epoch fields of the last
    gathered records, and the epochs whose prebuild vote was unanimous (from that step on the epoch
    is pending on every rank; all ranks see the same votes, so no wire field carries it)."""

    def __init__(self, joined_late: bool = False):
        self.joined_late = bool(joined_late)
        self.resident: list | None = None
        self.voted: set[int] = set()

    def reset(self) -> None:
        """The world was re-formed: the old records describe other ranks."""
        self.resident = None
        self.joined_late = True  # until the first records: whoever is in the new world may hold any epoch

    def update(self, resident_by_rank) -> None:
        self.resident = [set(r) for r in resident_by_rank]
        self.voted = {e for e in self.voted if not all(e in r for r in self.resident)}

    def vote_passed(self, epoch: int) -> None:
        self.voted.add(int(epoch))

    def mode(self, epoch: int, world_size: int) -> str:
        if self.resident is None:
            if self.joined_late:
                return dag_build_mode(None, None, epoch)
            resident = [set()] * world_size  # the start of the whole world: nobody holds anything
        else:
            resident = self.resident
        return dag_build_mode(resident, [self.voted] * len(resident), epoch)


class GpuSearchDevice:
    """One MI355X: resident epoch DAGs, per-period kernels, two share rings, the generation word.

    `collective_dag`: build DAGs sharded over the current process group and all-gather them
    (parallel/dag.py); every rank must then prepare the same epoch at the same step, which the
    mining service guarantees (all ranks act on the same broadcast work packet). A build is
    collective only if no rank of the world has the epoch resident or pending (dag_build_mode, fed
    by the service with every step's gathered records); otherwise, as on a rank that joined the
    world late (`joined_late`), the rank that lacks the epoch builds the whole DAG alone.
    `dag_build_mode[epoch]` records which it was, next to `dag_build_s[epoch]`.

    `jit_mode` (-kawpowjit, ops/kawpow.KawpowSearcher): "wait" stalls the loop in `submit` until a
    new period's kernel is compiled; "auto" runs such windows on the period-agnostic kernel and
    swaps to the compiled one between two windows; "off" never compiles.

    `dag_check` (-dagcheck, NODEXA_DAG_CHECK; default on): builds are checked (parallel/dag.DagCheck:
    every received shard against its owner's digest, a sampled audit against the light cache) and
    sealed with per-chunk digests. `dag_scrub_s` (-dagscrub, NODEXA_DAG_SCRUB_S; default 0 = off):
    every so many seconds `submit` queues a digest of the current epoch's DAG on the side stream and
    a later `submit` compares it with the seal; damaged chunks are repaired from the light cache
    while the search goes on, and a chunk that cannot be repaired raises DeviceFault. Scrubbing
    needs the seal, so it is off when `dag_check` is. With both off nothing of this runs and the
    counters (`dag_scrubs`, `dag_bad_chunks`, `dag_repaired_items`, `dag_last_scrub_ms`,
    `dag_check_events`) do not exist."""

    name = "gpu"
    MAX_EPOCHS = 2  # current + next (two 4 GiB DAGs are ~3 % of 288 GB)

    def __init__(self, device: int = 0, collective_dag: bool = False, jit_mode: str = "wait",
                 joined_late: bool = False, dag_check: bool | None = None, dag_scrub_s: float | None = None):
        import os

        import torch

        from ..ops import jit, runtime

        if jit_mode not in jit.JIT_MODES:
            raise ValueError(f"kawpow jit mode must be one of {', '.join(jit.JIT_MODES)}, not {jit_mode!r}")
        self.jit_mode = jit_mode
        self.kernel_kind = ""  # kernel of the last window submitted
        runtime.require_gpu()
        self.device = int(device)
        self.collective_dag = collective_dag
        self.h = runtime.hip()
        self.torch = torch
        self.epochs: dict[int, object] = {}
        self.searchers: dict[int, object] = {}
        self.lock = threading.Lock()
        self.dag_build_s: dict[int, float] = {}
        self.dag_build_mode: dict[int, str] = {}
        self.dag_builds = 0  # DAG builds this device took part in
        self.world_view = WorldEpochView(joined_late)
        nbytes = self.h.sizeof_results()
        with torch.cuda.device(self.device):
            # one stream per slot: the queued window starts on the CUs the running one's last
            # workgroups leave idle instead of waiting for its whole grid to drain (the tail of a
            # 2^25-nonce window is ~0.8 % of it; +0.3 % against one stream, profiles/README r4f)
            self.stream = torch.cuda.Stream(device=self.device)
            self.slot_streams = [self.stream, torch.cuda.Stream(device=self.device)]
            self.side = torch.cuda.Stream(device=self.device)  # next-epoch DAG builds
            self.rings = [torch.zeros(nbytes // 4, dtype=torch.int32, device=self.device) for _ in range(2)]
            self.host = [torch.zeros(nbytes // 4, dtype=torch.int32).pin_memory() for _ in range(2)]
            self.events = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            self.starts = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        self.meta: list[tuple | None] = [None, None]
        self.anchor = None  # timing event before the first window: SlotResult.end_ms is relative to it
        self.gen_ptr = self.h.host_words_alloc(1)
        self.generation = 0
        self.pending_build: dict[int, object] = {}
        if dag_check is None:
            dag_check = os.environ.get("NODEXA_DAG_CHECK", "1") != "0"
        if dag_scrub_s is None:
            dag_scrub_s = float(os.environ.get("NODEXA_DAG_SCRUB_S", "0") or 0)
        self.dag_check = bool(dag_check)
        self.dag_scrub_s = max(0.0, float(dag_scrub_s)) if self.dag_check else 0.0
        if self.dag_check:
            self.dag_checks: dict[int, object] = {}  # epoch -> DagCheck of a build not yet finished
            self.dag_scrubs = 0           # scrubs compared with the seal
            self.dag_bad_chunks = 0       # chunks found damaged, by a scrub or on arrival in a checked build
            self.dag_repaired_items = 0   # items rewritten from the light cache
            self.dag_last_scrub_ms = 0.0  # device time of the last scrub's digest
            self.dag_check_events = 0     # scrubs and builds that found something
            self.dag_bad_flag = False     # something was found since take_dag_bad() (the record's STATUS_DAG_BAD)
            self._scrub_buf: dict = {}    # epoch -> (DeviceEpoch, device table, pinned table, two events)
            self._scrub = None            # (epoch, DeviceEpoch, pinned table, start event, end event) in flight
            self._scrub_last = time.monotonic()

    def close(self) -> None:
        if self.gen_ptr:
            self.torch.cuda.synchronize(self.device)
            self.h.host_words_free(self.gen_ptr)
            self.gen_ptr = 0

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ epochs / kernels
    def _build_epoch(self, epoch: int, stream=None):
        from ..ops.ethash import DeviceEpoch
        from ..parallel import dag as pdag
        from ..parallel import world as W

        torch = self.torch
        ws = W.get().world_size if self.collective_dag else 1
        collective = self.collective_dag and self.world_view.mode(epoch, ws) == "collective"
        self.dag_build_mode[epoch] = "collective" if collective else "solo"
        self.dag_builds += 1
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):
            e = DeviceEpoch(epoch, device=self.device, world_size=ws if collective else 1)
            with torch.cuda.stream(stream or self.stream):
                if self.dag_check:
                    self.dag_checks[epoch] = pdag.build_dag_checked(e) if collective else pdag.build_solo_checked(e)
                elif collective:
                    pdag.build_dag(e)
                else:
                    e.build()
        self.dag_build_s[epoch] = time.perf_counter() - t0  # host-side issue time; completion below
        return e

    def epoch_ready(self, epoch: int) -> bool:
        return epoch in self.epochs

    def resident_epochs(self) -> list[int]:
        return sorted(self.epochs)

    def pending_epochs(self) -> list[int]:
        return sorted(self.pending_build)

    def prebuild(self, epoch: int) -> None:
        """Queue epoch's DAG build on the side stream (collective when sharded; every rank calls this
        at the same step). The search stream keeps running; the epoch becomes usable once its build
        event has completed."""
        if epoch in self.epochs or epoch in self.pending_build:
            return
        torch = self.torch
        e = self._build_epoch(epoch, stream=self.side)
        with torch.cuda.device(self.device):
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.pending_build[epoch] = (e, ev)

    def _epoch(self, epoch: int):
        if epoch in self.epochs:
            return self.epochs[epoch]
        torch = self.torch
        t0 = time.perf_counter()
        if epoch in self.pending_build:
            e, ev = self.pending_build.pop(epoch)
            for st in self.slot_streams:
                st.wait_event(ev)  # search kernels after the build, without a host sync
        else:
            e = self._build_epoch(epoch)
        with torch.cuda.device(self.device):
            for st in self.slot_streams:
                st.synchronize()
            if not e.l1_matches():
                raise RuntimeError(f"gpu{self.device}: epoch {epoch} DAG failed its L1 self-check")
            if self.dag_check:
                self._finish_dag_check(epoch)
                if self.dag_scrub_s:
                    self._scrub_buffers(epoch, e)
        self.dag_build_s[epoch] = self.dag_build_s.get(epoch, 0.0) + time.perf_counter() - t0
        from ..ops import verify as V

        V.share_epoch(self.device, epoch, e)  # header batches of this epoch verify against it too
        for old in [k for k in self.epochs if k < epoch - 1]:
            self.epochs.pop(old)
            self.searchers.pop(old, None)
        self.epochs[epoch] = e
        return e

    # ------------------------------------------------------------------ DAG integrity
    def _finish_dag_check(self, epoch: int) -> None:
        """After the build's streams are synchronised: compare the tables, repair, seal (raises
        RuntimeError as the L1 check does when the DAG cannot be made right)."""
        check = self.dag_checks.pop(epoch, None)
        if check is None:
            return
        try:
            check.finish()
        except RuntimeError as exc:
            raise RuntimeError(f"gpu{self.device}: epoch {epoch} DAG failed its build check: {exc}") from exc
        if check.events:
            self.dag_bad_chunks += check.bad_chunks
            self.dag_repaired_items += check.repaired_items
            self._dag_event(f"epoch {epoch} build check: {check.bad_chunks} received chunks damaged, "
                            f"{check.repaired_items} items repaired")

    def _dag_event(self, what: str) -> None:
        from ..utils.log import log_printf

        self.dag_check_events += 1
        self.dag_bad_flag = True
        log_printf(f"gpu{self.device}: DAG check: {what}")

    def take_dag_bad(self) -> bool:
        """A scrub or a build check found something since the last call (one record carries it)."""
        if not self.dag_check:
            return False
        bad, self.dag_bad_flag = self.dag_bad_flag, False
        return bad

    def dag_counters(self) -> dict:
        if not self.dag_check:
            return {}
        return {"dag_scrubs": self.dag_scrubs, "dag_bad_chunks": self.dag_bad_chunks,
                "dag_repaired_items": self.dag_repaired_items, "dag_last_scrub_ms": round(self.dag_last_scrub_ms, 3),
                "dag_check_events": self.dag_check_events}

    def _scrub_buffers(self, epoch: int, e):
        """The scrub's device and pinned tables and its two events, made once per epoch when the
        epoch becomes resident: no allocation, pinned ones least of all, inside the mining loop."""
        buf = self._scrub_buf.get(epoch)
        if buf is None or buf[0] is not e:
            torch = self.torch
            with torch.cuda.device(self.device):
                buf = (e, torch.empty(e.chunks, dtype=torch.int64, device=self.device),
                       torch.empty(e.chunks, dtype=torch.int64).pin_memory(),
                       torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self._scrub_buf = {epoch: buf}
        return buf

    def _scrub_tick(self, epoch: int) -> None:
        """Never blocks unless damage was found: queue a digest of the epoch's DAG on the side stream
        when the interval has passed, or, once a queued one has finished, compare it with the seal."""
        torch = self.torch
        if self._scrub is None:
            now = time.monotonic()
            e = self.epochs.get(epoch)
            if now - self._scrub_last < self.dag_scrub_s or e is None or e.seal_table is None:
                return
            self._scrub_last = now
            buf = self._scrub_buffers(epoch, e)
            _, table, host, ev0, ev1 = buf
            side = int(self.side.cuda_stream)
            with torch.cuda.device(self.device):
                ev0.record(self.side)
                e.digest(stream=side, out=table)
                self.h.memcpy_async(host.data_ptr(), table.data_ptr(), table.numel() * 8, side, "dtoh")
                ev1.record(self.side)
            self._scrub = (epoch, e, host, ev0, ev1)
            return
        ep, e, host, ev0, ev1 = self._scrub
        if not ev1.query():
            return
        self._scrub = None
        self.dag_scrubs += 1
        self.dag_last_scrub_ms = ev0.elapsed_time(ev1)
        bad = e.chunks_differing(host)
        if not bad:
            return
        # a repair writes correct bytes over wrong ones: the running search windows are safe
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            left = e.repair_chunks(bad)
        self.dag_bad_chunks += len(bad)
        self.dag_repaired_items += e.last_repaired
        self._dag_event(f"epoch {ep} scrub: chunks {bad} differ from the seal, {e.last_repaired} items repaired")
        if left:
            raise DeviceFault(f"gpu{self.device}: epoch {ep} DAG chunks {left} still differ from the seal after a "
                              f"repair (damaged light cache?)")

    def searcher(self, height: int):
        from ..ops.kawpow import KawpowSearcher

        epoch = height // _core.EPOCH_LENGTH
        with self.lock:
            ep = self._epoch(epoch)
            s = self.searchers.get(epoch)
            if s is None:
                with self.torch.cuda.device(self.device):
                    s = KawpowSearcher(ep, height, prefetch_next=True, jit_mode=self.jit_mode)
                self.searchers[epoch] = s
            else:
                s.set_block(height)
            return s

    def block_for(self, height: int) -> int:
        return self.searcher(height).block

    def window_for(self, work: Work, window: int) -> int:
        b = self.block_for(work.height)
        return max(b, window // b * b)

    # ------------------------------------------------------------------ the two slots
    def submit(self, slot: int, work: Work, start: int, count: int) -> None:
        torch = self.torch
        s = self.searcher(work.height)
        if self.dag_scrub_s:
            self._scrub_tick(work.height // _core.EPOCH_LENGTH)
        b = s.block
        count = max(b, count // b * b)
        st = self.slot_streams[slot]
        with torch.cuda.device(self.device), torch.cuda.stream(st):
            ring = self.rings[slot]
            ring[:4].zero_()
            if self.anchor is None:
                self.anchor = torch.cuda.Event(enable_timing=True)
                self.anchor.record(st)
            self.starts[slot].record(st)
            s.launch(work.header_hash, start, count, work.target64(), stream=int(st.cuda_stream),
                     results=ring, gen_word=self.gen_ptr, generation=self.generation)
            self.host[slot].copy_(ring, non_blocking=True)
            self.events[slot].record(st)
        self.kernel_kind = s.kernel_kind
        self.meta[slot] = (work, start, count, b, s.kernel_kind)

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        from ..ops.kawpow import parse_results

        ev = self.events[slot]
        if timeout_s is not None:
            deadline = time.monotonic() + timeout_s
            while not ev.query():
                if time.monotonic() > deadline:
                    raise DeviceHung(f"gpu{self.device}: search window did not finish in {timeout_s:.0f}s")
                time.sleep(0.0005)
        ev.synchronize()
        work, start, count, block, kind = self.meta[slot]
        self.meta[slot] = None
        shares, n, skipped = parse_results(self.host[slot].numpy().tobytes(), self.h.KAWPOW_MAX_SHARES)
        shares = [x for x in shares if _core.hash_le(x.final_hash, work.boundary)]
        hashes = max(0, count - skipped * block)
        return SlotResult(work.job_id, start, count, hashes, shares, self.starts[slot].elapsed_time(ev), skipped,
                          ALGO_KAWPOW, self.anchor.elapsed_time(ev), kind, max(0, n - self.h.KAWPOW_MAX_SHARES))

    def abort(self) -> None:
        """Make every queued or running window stale (its remaining workgroups exit at start)."""
        self.generation = (self.generation + 1) & 0xFFFFFFFF
        self.h.host_word_store(self.gen_ptr, 0, self.generation)

    def synchronize(self) -> None:
        for st in self.slot_streams:
            st.synchronize()


class CpuSearchDevice:
    """The same two-slot protocol on the host: light-mode search (progpow::search_light,
    src/crypto/ethash/lib/ethash/progpow.cpp:553-565), first share of each window. For CPU-only
    nodes and for rehearsing the multi-rank loop over gloo."""

    name = "cpu"
    device = -1

    def __init__(self, max_window: int = 4096):
        self.max_window = int(max_window)
        self.meta: list[tuple | None] = [None, None]
        self.generation = 0
        self.collective_dag = False

    def block_for(self, height: int) -> int:
        return 1

    def window_for(self, work: Work, window: int) -> int:
        return max(1, min(int(window), self.max_window))

    def epoch_ready(self, epoch: int) -> bool:
        return True

    def resident_epochs(self) -> list[int]:
        return []

    def prebuild(self, epoch: int) -> None:
        _core.get_epoch_context(epoch)

    def submit(self, slot: int, work: Work, start: int, count: int) -> None:
        self.meta[slot] = (work, start, min(count, self.max_window), self.generation)

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        from ..ops.kawpow import Share

        work, start, count, gen = self.meta[slot]
        self.meta[slot] = None
        if gen != self.generation:  # aborted before it ran
            return SlotResult(work.job_id, start, count, 0, [], 0.0, 1, ALGO_KAWPOW)
        t0 = time.perf_counter()
        ctx = _core.get_epoch_context(work.epoch)
        ok, nonce, fin, mix = _core.kawpow_search_light(ctx, work.height, work.header_hash, work.boundary,
                                                         start, count)
        dt = (time.perf_counter() - t0) * 1e3
        if ok:
            return SlotResult(work.job_id, start, count, nonce - start + 1, [Share(nonce, mix, fin)], dt)
        return SlotResult(work.job_id, start, count, count, [], dt)

    def abort(self) -> None:
        self.generation += 1

    def synchronize(self) -> None:
        pass

    def close(self) -> None:
        pass


class LegacyHostDevice:
    """X16R / X16RV2 templates (before the KawPow activation; the regtest default): the 32-bit
    nNonce scanned on the host cores by the native multi-threaded search (csrc/pow/x16r.cpp,
    `_core.x16r_search`), first hit of each window — generateBlocks' loop (src/rpc/mining.cpp:
    141-149) in windows. The 32-bit space is split 2^28 per rank (`start` wraps inside it)."""

    name = "host-x16r"
    device = -1

    def __init__(self):
        self.meta: list[tuple | None] = [None, None]
        self.generation = 0

    def window_for(self, work: Work, window: int) -> int:
        return LEGACY_WINDOW

    def submit(self, slot: int, work: Work, start: int, count: int) -> None:
        self.meta[slot] = (work, start & 0xFFFFFFFF, count, self.generation)

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        work, start, count, gen = self.meta[slot]
        self.meta[slot] = None
        if gen != self.generation:
            return SlotResult(work.job_id, start, count, 0, [], 0.0, 1, work.algo)
        count = min(count, (1 << 32) - start)
        t0 = time.perf_counter()
        target_le = work.boundary[::-1]
        res, hashes = _core.x16r_search(work.header, work.algo == ALGO_X16RV2, target_le, start, count)
        dt = (time.perf_counter() - t0) * 1e3
        shares = [LegacyShare(int(res[0]), bytes(res[1]))] if res is not None else []
        return SlotResult(work.job_id, start, count, int(hashes), shares, dt, 0, work.algo)

    def abort(self) -> None:
        self.generation += 1

    def synchronize(self) -> None:
        pass

    def close(self) -> None:
        pass


class LegacyGpuDevice(LegacyHostDevice):
    """The same X16R / X16RV2 windows on this rank's GPU (ops/x16r.X16rSearcher: every nonce of a
    window runs the same 16 slots, one launch per step, the lowest hit kept on the device)."""

    name = "gpu-x16r"

    def __init__(self, device: int = 0, window: int = LEGACY_GPU_WINDOW):
        super().__init__()
        self.device = int(device)
        self._window = int(window)
        self._searcher = None

    def window_for(self, work: Work, window: int) -> int:
        return self._window

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        work, start, count, gen = self.meta[slot]
        self.meta[slot] = None
        if gen != self.generation:
            return SlotResult(work.job_id, start, count, 0, [], 0.0, 1, work.algo)
        count = min(count, (1 << 32) - start)
        if self._searcher is None:
            from ..ops.x16r import X16rSearcher

            self._searcher = X16rSearcher(self.device, window=self._window)
        t0 = time.perf_counter()
        res, hashes = self._searcher.search(work.header, work.algo == ALGO_X16RV2, work.boundary[::-1], start, count)
        dt = (time.perf_counter() - t0) * 1e3
        shares = [LegacyShare(int(res[0]), bytes(res[1]))] if res is not None else []
        return SlotResult(work.job_id, start, count, int(hashes), shares, dt, 0, work.algo)


class RankDevice:
    """Everything one rank mines with, behind the two-slot protocol: the KawPow device (GPU or host),
    the Equihash device (made on first use: GPU solver or host golden solver) and the host X16R
    search. Each slot goes to the device of its work's algorithm, so a chain crossing an activation
    time switches algorithms between two windows with no change to the loop."""

    def __init__(self, kawpow, equihash=None, legacy=None, equihash_factory=None):
        self.kawpow = kawpow
        self._equihash = equihash
        self._eq_factory = equihash_factory
        self.legacy = legacy if legacy is not None else LegacyHostDevice()
        self.slot_dev: list[object | None] = [None, None]
        self.name = getattr(kawpow, "name", "dev")
        self.device = getattr(kawpow, "device", -1)

    @property
    def collective_dag(self) -> bool:
        return getattr(self.kawpow, "collective_dag", False)

    @property
    def equihash(self):
        if self._equihash is None:
            if self._eq_factory is None:
                from .equihash_search import EquihashCpuDevice

                self._equihash = EquihashCpuDevice()
            else:
                self._equihash = self._eq_factory()
        return self._equihash

    def dev_for(self, work: Work):
        if work.algo == ALGO_KAWPOW:
            return self.kawpow
        if work.algo == ALGO_EQUIHASH:
            return self.equihash
        return self.legacy

    def window_for(self, work: Work, window: int) -> int:
        return self.dev_for(work).window_for(work, window)

    def block_for(self, height: int) -> int:
        return self.kawpow.block_for(height)

    def epoch_ready(self, epoch: int) -> bool:
        return self.kawpow.epoch_ready(epoch)

    def resident_epochs(self) -> list[int]:
        return self.kawpow.resident_epochs() if hasattr(self.kawpow, "resident_epochs") else []

    def pending_epochs(self) -> list[int]:
        return self.kawpow.pending_epochs() if hasattr(self.kawpow, "pending_epochs") else []

    @property
    def world_view(self):
        """The KawPow device's view of its peers' DAGs (None: a device that shares no builds)."""
        return getattr(self.kawpow, "world_view", None)

    def prebuild(self, epoch: int) -> None:
        self.kawpow.prebuild(epoch)

    def submit(self, slot: int, work: Work, start: int, count: int) -> None:
        d = self.dev_for(work)
        self.slot_dev[slot] = d
        d.submit(slot, work, start, count)

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        d, self.slot_dev[slot] = self.slot_dev[slot], None
        return d.wait(slot, timeout_s)

    def abort(self) -> None:
        for d in (self.kawpow, self._equihash, self.legacy):
            if d is not None:
                d.abort()

    def synchronize(self) -> None:
        for d in (self.kawpow, self._equihash):
            if d is not None:
                d.synchronize()

    def close(self) -> None:
        for d in (self.kawpow, self._equihash, self.legacy):
            if d is not None and hasattr(d, "close"):
                d.close()


def as_rank_device(dev) -> RankDevice:
    """A bare device becomes a rank's device for its own algorithm: an Equihash device serves the
    Equihash windows (a KawPow or X16R packet would find no device of its kind and fail), any
    other device the KawPow ones."""
    if isinstance(dev, (RankDevice, FaultInjectingDevice, HangingDevice)):
        return dev
    if getattr(dev, "algo", None) == ALGO_EQUIHASH:
        return RankDevice(_NoKawpow(dev), equihash=dev)
    return RankDevice(dev)


class _NoKawpow:
    """The KawPow slot of a rank that only has an Equihash device (bench.py's Equihash loop)."""

    def __init__(self, eq):
        self.name, self.device = eq.name, eq.device

    def window_for(self, work, window):
        raise DeviceFault("this rank has no KawPow device")

    submit = block_for = window_for

    def epoch_ready(self, epoch: int) -> bool:
        return True

    def resident_epochs(self) -> list[int]:
        return []

    def prebuild(self, epoch: int) -> None:
        pass

    def abort(self) -> None:
        pass

    def synchronize(self) -> None:
        pass


class SearchPipeline:
    """Two windows in flight: `step` queues the next window, then returns the previous one's result.
    The device never waits for the host between windows; the host's share handling, collectives
    and bookkeeping overlap the window that is running."""

    def __init__(self, dev, watchdog_s: float | None = None):
        self.dev = dev
        self.watchdog_s = watchdog_s
        self.inflight: int | None = None
        self.next_slot = 0

    def step(self, work: Work, start: int, count: int) -> SlotResult | None:
        slot = self.next_slot
        self.dev.submit(slot, work, start, count)
        prev, self.inflight = self.inflight, slot
        self.next_slot ^= 1
        return self.dev.wait(prev, self.watchdog_s) if prev is not None else None

    def drain(self) -> SlotResult | None:
        if self.inflight is None:
            return None
        prev, self.inflight = self.inflight, None
        return self.dev.wait(prev, self.watchdog_s)


class _Wrapper:
    def __init__(self, inner):
        self.inner = inner

    def __getattr__(self, name):
        return getattr(self.inner, name)


class FaultInjectingDevice(_Wrapper):
    """-gpufailrate / -dropshare (SURVEY §5 fault injection; never on by default): each window fails
    with probability `fail_rate` (wait() raises DeviceFault after the window ran, as a device error
    surfaces), and each share is silently lost with probability `drop_rate` (a share lost between
    device and host). Wraps any device of the two-slot protocol."""

    def __init__(self, inner, fail_rate: float = 0.0, drop_rate: float = 0.0, seed: int | None = None):
        import random

        super().__init__(inner)
        self.fail_rate, self.drop_rate = float(fail_rate), float(drop_rate)
        self.rng = random.Random(seed)
        self.dropped = 0
        self.faults = 0

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        res = self.inner.wait(slot, timeout_s)
        if self.fail_rate and self.rng.random() < self.fail_rate:
            self.faults += 1
            raise DeviceFault(f"injected device fault on {getattr(self.inner, 'name', 'dev')}")
        if self.drop_rate and res.shares:
            kept = [s for s in res.shares if self.rng.random() >= self.drop_rate]
            self.dropped += len(res.shares) - len(kept)
            res.shares = kept
        return res


class HangingDevice(_Wrapper):
    """Fault injection (tests, `NODEXA_MINER_HANG_AFTER`): behaves like `inner` for `after` windows,
    then every window hangs — wait() blocks until the watchdog limit and raises DeviceHung, which is
    what a GPU whose kernel never returns looks like to the mining loop."""

    def __init__(self, inner, after: int):
        super().__init__(inner)
        self.after = int(after)
        self.waits = 0

    def wait(self, slot: int, timeout_s: float | None = None) -> SlotResult:
        self.waits += 1
        if self.waits <= self.after:
            return self.inner.wait(slot, timeout_s)
        time.sleep(timeout_s if timeout_s is not None else 1e9)
        raise DeviceHung(f"{getattr(self.inner, 'name', 'dev')}: injected hang")
