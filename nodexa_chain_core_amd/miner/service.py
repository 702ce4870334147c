"""The node's miner: one process per GPU, nonce-space data parallelism over RCCL.

Reference: GenerateClores / CloreMiner (src/miner.cpp:566-759) run N host threads, each with its
own template and a 32-bit nonce scan; generateBlocks (src/rpc/mining.cpp:117-173) is a second,
separate loop; getmininginfo reports nHashesPerSec (src/rpc/mining.cpp:209-250). Here there is
one loop for everything. Every GPU is a rank of one torch.distributed world (backend "nccl" =
RCCL over xGMI on the MI355X node; "gloo" for CPU rehearsals; a single CPU-only rank needs no
process group at all) and all ranks run the same step, `MiningService.step`:

  1. queue the next window on this rank's device and take the previous window's result
     (miner/search.SearchPipeline: the GPU never waits for the host). The work packet says which
     proof of work: KawPow (2^25-nonce GPU windows), Equihash(200,9) (16 solver instances per
     window) or X16R/X16RV2 (host windows of 2^16 nNonce values, before the KawPow activation);
  2. all-gather every rank's record (fixed 5592-byte slot: job, work done, shares, and the rank's
     own telemetry: device time, aborted workgroups, collective wait, failures, resident epochs,
     next-epoch readiness vote); every rank sums the work counters and votes from it;
  3. rank 0 (the node: chain state, RPC) checks shares again (KawPow: full light-mode re-hash;
     Equihash: the golden verifier; X16R: the block check), builds the block of the share's job
     and runs ProcessNewBlock; then it decides the next work packet;
  4. broadcast the 144-byte work packet from rank 0; a new job with FLAG_CLEAN makes every rank
     abort its queued window of the stale job on the device.

Nonce partition: rank r of n searches job-local windows from nonce_base + (r << 56) (X16R's 32-bit
nNonce: r << 28), so ranks never overlap and a job change (new extranonce -> new header) restarts
every cursor. A packet that names a `rank_shift` s (bits 8..15 of its flags; a pool's nonce prefix,
miner/stratum_client.py) gives rank r the range [nonce_base + (r << s), nonce_base + ((r + 1) << s))
instead: a window is clipped to the range's end in whole launch granules, and a rank that has used
its range up sends records without work (STATUS_EXHAUSTED) until the job changes; it never wraps
into another rank's or another connection's range.
DAGs are built sharded over the ranks and all-gathered (parallel/dag.py); the next
epoch's DAG is prebuilt on a side stream once every rank reports its light cache ready (a vote in
the gathered records, so the collective build starts on the same step everywhere). On RCCL the two
collectives run from a high-priority stream with persistent pinned/device buffers, so they never
queue behind a search window on a shared hardware queue.

Failure handling (the reference's miner just exits on errors, src/miner.cpp:716-725):
* a window that raises (a device fault; -gpufailrate injects them) counts a failure; after
  `max_failures` in a row the rank's device is evicted: a follower rank exits with
  EXIT_DEVICE_FAILED and the survivors re-form without it, rank 0 keeps leading without searching;
* a rank whose window outlives the watchdog exits with EXIT_DEVICE_HUNG (a fresh process on
  restart, never a re-exec). Survivors see their next collective fail or time out, register in the
  rendezvous store under a new membership epoch, wait out a grace period, rebuild the group over
  the ranks that registered (parallel/world.shrink) and carry on; rank 0 then issues a clean job
  so the nonce space is re-partitioned over the new ranks.
* with -minerrejoin=<seconds> the lost rank comes back. A new process cannot enter an existing
  torch.distributed default group, so such a world is made over a stand-alone rendezvous store that
  rank 0 hosts (parallel/world.init(store_port=...)) and can be made again with other members
  (parallel/world.reform). Rank 0 has initialised its GPU by then and must not start processes, so
  the followers belong to a GPU-free supervisor that rank 0 starts before it touches a GPU
  (miner/supervisor.py). The protocol is driven by rank 0 (Rejoiner), so no collective has to
  fail first: the supervisor reports the exit (75 / 76 / a signal), the survivors shrink as above,
  after the delay the supervisor starts a new process for that GPU, the newcomer prepares alone
  (imports, its device, the light cache of the epoch rank 0 named), sets "join/<k>/ready/<id>" and
  blocks on "m<k>/members"; rank 0 checks the ready key once per step without blocking, then names
  the members and sets FLAG_REFORM in the next work packet; every rank drains, re-forms the world,
  rebinds its communicator and resets cursor and work, rank 0 issues a clean job and the nonce
  partition re-derives from (rank, world_size). The newcomer ends up in the same place: a
  MiningService constructed after its world exists. Its first job's DAG it builds alone
  (search.dag_build_mode), within one step, so the collective timeout must cover a DAG build (the
  default 60 s does). A newcomer that dies before it is ready cancels the attempt (the survivors
  never see FLAG_REFORM); one lost while the world is being re-formed makes the others re-form over
  the members they were. A GPU that ends -minerrejoinmax times within -minerrejoinwindow seconds
  stays evicted. The leader (id 0) is never replaced: its own device being evicted keeps today's
  behaviour, it leads without searching. A torchrun world never re-joins (the launcher owns the
  processes). getmininginfo.gpus[] keeps the entry of a rank that is out (state, lives, last_exit,
  rejoin_in_s); counters miner_rejoins_total / miner_rejoin_failed_total / miner_rejoin_refused_total.
Test hooks (environment only, never flags; the faults are the software ones of FaultInjectingDevice):
NODEXA_MINER_FAIL_COLLECTIVE_AT=<n> makes the n-th collective of the loop raise;
NODEXA_MINER_FAILRATE_LIVES=<n> applies the injected fail rate only while NODEXA_MINER_LIFE < n;
NODEXA_MINER_FAILRATE_RANK=<id> applies it only to that rank; NODEXA_MINER_REFORM_AT=<step> makes
rank 0 of a store world re-form the same membership once at that step.
Resume: the leader persists {tip, extranonce} (miner_state.json); a restart on the same tip
continues the extranonce sequence, so no template searched before the restart is searched again.
"""
from __future__ import annotations

import datetime
import json
import os
import struct
import sys
import threading
import time
from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

from .. import core
from ..utils import log
from .search import (ALGO_EQUIHASH, ALGO_KAWPOW, ALGO_NAMES, ALGO_X16R, ALGO_X16RV2, EPOCH_PREBUILD_WINDOW,
                     FLAG_CLEAN, FLAG_IDLE, FLAG_REFORM, FLAG_STOP, WORK_SIZE, DeviceFault, DeviceHung, EquihashShare,
                     LegacyShare, SearchPipeline, SlotResult, Work, as_rank_device)

_core = core()

EXIT_DEVICE_HUNG = 75
EXIT_DEVICE_FAILED = 76
MAX_SHARES = {ALGO_KAWPOW: 16, ALGO_EQUIHASH: 4, ALGO_X16R: 16, ALGO_X16RV2: 16}
MAX_SHARES_PER_STEP = MAX_SHARES[ALGO_KAWPOW]
# job, work done, nshares, algo, device_us, aborted workgroups, collective wait us (previous step),
# consecutive failures, first resident epoch, resident epochs, status bits, device index
_REC_HEAD = struct.Struct("<QQIIIIIIIIIi")
_SHARE = {ALGO_KAWPOW: struct.Struct("<Q32s32s"),        # nonce, mix, final
          ALGO_EQUIHASH: struct.Struct("<Q1344s32s"),    # nonce, packed solution, block hash
          ALGO_X16R: struct.Struct("<Q32s"),             # nNonce, block hash
          ALGO_X16RV2: struct.Struct("<Q32s")}
RECORD_PAYLOAD = max(MAX_SHARES[a] * s.size for a, s in _SHARE.items())  # 5536
RECORD_SIZE = _REC_HEAD.size + RECORD_PAYLOAD                           # 5592
STATUS_RESULT, STATUS_ALIVE, STATUS_VOTE = 1, 2, 4  # VOTE: next-epoch light cache ready
STATUS_KERNEL_JIT, STATUS_KERNEL_GENERIC = 8, 16     # the KawPow kernel of the record's window (neither: not a GPU KawPow window)
STATUS_EXHAUSTED = 32  # the rank has searched its whole nonce range of the current job (Work.rank_shift)
STATUS_DAG_BAD = 64    # a DAG scrub or build check of this rank found damage in this step (search.GpuSearchDevice)
_KERNEL_BITS = {"jit": STATUS_KERNEL_JIT, "generic": STATUS_KERNEL_GENERIC}


class CollectiveError(RuntimeError):
    """A collective of the mining loop failed or timed out (a peer rank is gone or hung)."""


class DeviceEvicted(RuntimeError):
    """This rank's device failed `max_failures` windows in a row."""


@dataclass
class RankRecord:
    """One rank's gathered step record."""
    job_id: int = 0
    hashes: int = 0
    shares: list = field(default_factory=list)
    algo: int = ALGO_KAWPOW
    device_ms: float = 0.0
    aborted: int = 0
    coll_ms: float = 0.0
    failures: int = 0
    epochs: list = field(default_factory=list)
    has_result: bool = False
    alive: bool = True
    device: int = -1
    kernel: str = ""  # "jit" / "generic": the KawPow kernel of this window on a GPU rank
    dropped: int = 0  # shares of this window lost to the device ring or to the record's share cap
    exhausted: bool = False  # the rank's nonce range of the current job is used up
    dag_bad: bool = False    # the rank's DAG check found (and repaired) damage in this step


def _as_record(r) -> RankRecord:
    if isinstance(r, RankRecord):
        return r
    job, hashes, shares = r  # (job_id, hashes, shares) tuples: tests, remote leader
    return RankRecord(job, hashes, list(shares), has_result=True)


def pack_record(res: SlotResult | None, *, coll_ms: float = 0.0, failures: int = 0, epochs=(),
                alive: bool = True, device: int = -1, vote: bool = False, exhausted: bool = False,
                dag_bad: bool = False) -> bytes:
    out = bytearray(RECORD_SIZE)
    ep = sorted(epochs)
    lo, n = (ep[0], ep[-1] - ep[0] + 1) if ep else (0, 0)
    status = (STATUS_RESULT if res is not None else 0) | (STATUS_ALIVE if alive else 0) | (STATUS_VOTE if vote else 0)
    status |= (STATUS_EXHAUSTED if exhausted else 0) | (STATUS_DAG_BAD if dag_bad else 0)
    if res is None:
        _REC_HEAD.pack_into(out, 0, 0, 0, 0, 0, 0, 0, int(coll_ms * 1e3), failures, lo, n, status, device)
        return bytes(out)
    status |= _KERNEL_BITS.get(getattr(res, "kernel", ""), 0)
    fmt = _SHARE[res.algo]
    shares = res.shares[:MAX_SHARES[res.algo]]
    # the share count is what the window found: the payload holds the first MAX_SHARES of them, and
    # the reader counts the rest (and what the device ring had no room for) as dropped
    found = min(len(res.shares) + getattr(res, "dropped", 0), 2**32 - 1)
    _REC_HEAD.pack_into(out, 0, res.job_id, res.hashes, found, res.algo, min(int(res.device_ms * 1e3), 2**32 - 1),
                        res.aborted, min(int(coll_ms * 1e3), 2**32 - 1), failures, lo, n, status, device)
    for i, s in enumerate(shares):
        off = _REC_HEAD.size + i * fmt.size
        if res.algo == ALGO_KAWPOW:
            fmt.pack_into(out, off, s.nonce, s.mix_hash, s.final_hash)
        elif res.algo == ALGO_EQUIHASH:
            fmt.pack_into(out, off, s.nonce, s.solution, s.block_hash)
        else:
            fmt.pack_into(out, off, s.nonce, s.block_hash)
    return bytes(out)


def record_totals(gathered: list[bytes]) -> tuple[int, int]:
    """(hashes, next-epoch votes) summed over the gathered records: the loop's counters ride in
    the record all-gather instead of an all-reduce of their own (one collective less per step)."""
    hashes = votes = 0
    for raw in gathered:
        _job, h, *_rest, status, _dev = _REC_HEAD.unpack_from(raw, 0)
        hashes += h
        votes += bool(status & STATUS_VOTE)
    return hashes, votes


def record_epochs(gathered: list[bytes]) -> list[range]:
    """Per rank, the epochs its record names (resident or being built)."""
    out = []
    for raw in gathered:
        *_head, lo, n, _status, _dev = _REC_HEAD.unpack_from(raw, 0)
        out.append(range(lo, lo + n))
    return out


def publish_members(store, k: int, members, membership: int) -> None:
    """Rank 0 names the members of the next world under the store key "m<k>/members": the sorted
    ids, the leader's first, and the membership number the new world gets (at least k)."""
    store.set(f"m{k}/members", json.dumps({"members": [int(x) for x in members], "membership": int(membership)}))


def unpack_record(raw: bytes) -> RankRecord:
    from ..ops.kawpow import Share

    job, hashes, n, algo, dev_us, aborted, coll_us, failures, lo, nep, status, device = _REC_HEAD.unpack_from(raw, 0)
    fmt = _SHARE.get(algo, _SHARE[ALGO_KAWPOW])
    shares = []
    for i in range(min(n, MAX_SHARES.get(algo, 0))):
        vals = fmt.unpack_from(raw, _REC_HEAD.size + i * fmt.size)
        if algo == ALGO_KAWPOW:
            shares.append(Share(*vals))
        elif algo == ALGO_EQUIHASH:
            shares.append(EquihashShare(*vals))
        else:
            shares.append(LegacyShare(*vals))
    return RankRecord(job, hashes, shares, algo, dev_us / 1e3, aborted, coll_us / 1e3, failures,
                      list(range(lo, lo + nep)), bool(status & STATUS_RESULT), bool(status & STATUS_ALIVE), device,
                      "jit" if status & STATUS_KERNEL_JIT else "generic" if status & STATUS_KERNEL_GENERIC else "",
                      n - len(shares), bool(status & STATUS_EXHAUSTED), bool(status & STATUS_DAG_BAD))


class Comm:
    """The loop's collectives on the current world group, each bounded by a timeout.

    RCCL: tensors live on the GPU and the collectives are issued from a stream of their own, so
    they never queue behind the search kernel that is running on the search stream. gloo: host
    tensors. Without a process group (a single CPU rank) there is nothing to exchange. A world
    initialised with forced collectives (parallel/world.init(force_collectives=True)) runs them
    even at world size 1, so a one-GPU box executes the same RCCL path as an 8-GPU node."""

    def __init__(self, timeout_s: float):
        from ..parallel import world as W

        self.W = W
        self.timeout = datetime.timedelta(seconds=timeout_s)
        self.fail_at_step = int(os.environ.get("NODEXA_MINER_FAIL_COLLECTIVE_AT", "0"))  # test hook
        self.calls = 0
        self.rebind()

    def rebind(self) -> None:
        """Bind to the current world. The loop gets a communicator of its own (not the default
        group), so a failed one can be aborted (RCCL) and replaced without touching the default
        group or its rendezvous store."""
        self.w = self.W.get()
        self.active = self.w.collective
        self.gpu = self.w.backend == "nccl"
        self.stream = None
        self._buf: dict[str, tuple] = {}
        self.group = self.w.group
        if self.active:
            import torch

            self.torch = torch
            dist = self.W.dist
            if self.gpu:
                # the highest priority: its copies must not share a hardware queue with the search
                # stream, where they would wait behind the window queued for the next step and
                # drain the two-window pipeline every step (profiles/README r4b)
                self.stream = torch.cuda.Stream(device=self.w.device, priority=-16)
            if self.W.is_init_group(self.group):
                # gloo connects the group's full mesh under the group timeout, and ranks reach this
                # point seconds apart on a loaded host (a DAG build, a cold import): connect under the
                # rendezvous timeout. Every collective stays bounded by self.timeout (_wait), and a
                # dead gloo peer fails its pair at once.
                conn = self.timeout if self.gpu else max(self.timeout,
                                                         datetime.timedelta(seconds=self.W.rendezvous_timeout()))
                self.group = dist.new_group(ranks=list(range(self.w.world_size)), timeout=conn)

    def abort(self) -> None:
        """Tear down the loop's communicator after a failure: RCCL kernels still waiting for a dead
        peer are cancelled (ncclCommAbort); gloo needs nothing (its ops already raised)."""
        if self.gpu and self.group is not None:
            try:
                self.W.dist.distributed_c10d._abort_process_group(self.group)
            except Exception as e:  # noqa: BLE001 — best effort; the survivors re-form regardless
                log.log_printf(f"miner: aborting the failed communicator: {e}")
        if self.w.group is None:
            self.group = None  # rebind() makes a fresh loop communicator

    def _wait(self, work, what: str) -> None:
        try:
            ok = work.wait(timeout=self.timeout)
        except Exception as e:  # noqa: BLE001 — gloo raises on a closed peer, RCCL on timeout
            raise CollectiveError(f"{what}: {e}") from e
        if ok is False:
            raise CollectiveError(f"{what}: timed out")

    def _run(self, fn, what: str):
        self.calls += 1
        if self.fail_at_step and self.calls == self.fail_at_step:
            raise CollectiveError(f"{what}: timed out (injected, NODEXA_MINER_FAIL_COLLECTIVE_AT)")
        torch = self.torch
        if self.gpu:
            with torch.cuda.device(self.w.device), torch.cuda.stream(self.stream):
                out = fn()
                self.stream.synchronize()
                return out
        return fn()

    def _bufs(self, key: str, n: int):
        """Persistent (pinned host, device) byte buffers of a collective (RCCL): no allocation and
        no pageable copy per step."""
        b = self._buf.get(key)
        if b is None or b[0].numel() < n:
            torch = self.torch
            b = (torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.uint8, device=self.w.device))
            self._buf[key] = b
        return b[0][:n], b[1][:n]

    def broadcast(self, payload: bytes | None, size: int) -> bytes:
        if not self.active:
            return payload
        torch, dist = self.torch, self.W.dist

        def go():
            if self.gpu:
                host, dev = self._bufs("bcast", size)
                if self.w.rank == 0:
                    host.numpy()[:] = np.frombuffer(payload, dtype=np.uint8, count=size)
                    dev.copy_(host, non_blocking=True)
                self._wait(dist.broadcast(dev, src=self.w.global_rank(0), group=self.group, async_op=True), "broadcast")
                host.copy_(dev, non_blocking=True)
                self.stream.synchronize()
                return host.numpy().tobytes()
            t = torch.zeros(size, dtype=torch.uint8)
            if self.w.rank == 0:
                t.copy_(torch.frombuffer(bytearray(payload), dtype=torch.uint8))
            self._wait(dist.broadcast(t, src=self.w.global_rank(0), group=self.group, async_op=True), "broadcast")
            return bytes(t.numpy().tobytes())

        return self._run(go, "broadcast")

    def all_gather(self, record: bytes) -> list[bytes]:
        if not self.active:
            return [record]
        torch, dist = self.torch, self.W.dist
        n, ws = len(record), self.w.world_size

        def go():
            if self.gpu:
                host, mine = self._bufs("rec", n)
                hout, out = self._bufs("gather", ws * n)
                host.numpy()[:] = np.frombuffer(record, dtype=np.uint8)
                mine.copy_(host, non_blocking=True)
                self._wait(dist.all_gather_into_tensor(out, mine, group=self.group, async_op=True), "all_gather")
                hout.copy_(out, non_blocking=True)
                self.stream.synchronize()
                raw = hout.numpy().tobytes()
            else:
                out = torch.empty(ws * n, dtype=torch.uint8)
                parts = list(out.view(ws, n).unbind(0))
                mine = torch.frombuffer(bytearray(record), dtype=torch.uint8)
                self._wait(dist.all_gather(parts, mine, group=self.group, async_op=True), "all_gather")
                raw = bytes(out.numpy().tobytes())
            return [raw[i * n:(i + 1) * n] for i in range(ws)]

        return self._run(go, "all_gather")

    def all_reduce_sum(self, vals: list[int]) -> list[int]:
        if not self.active:
            return list(vals)
        torch, dist = self.torch, self.W.dist

        def go():
            t = torch.tensor(vals, dtype=torch.int64)
            if self.gpu:
                t = t.to(self.w.device, non_blocking=True)
            self._wait(dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True), "all_reduce")
            return [int(x) for x in t.cpu().tolist()]

        return self._run(go, "all_reduce")


class RateMeter:
    """Work per second over a sliding window (getmininginfo.hashespersec)."""

    def __init__(self, window_s: float = 8.0):
        self.window_s = window_s
        self.samples: list[tuple[float, int]] = []
        self.lock = threading.Lock()

    def add(self, hashes: int, now: float | None = None) -> None:
        now = time.monotonic() if now is None else now
        with self.lock:
            self.samples.append((now, hashes))
            while len(self.samples) > 2 and now - self.samples[1][0] > self.window_s:
                self.samples.pop(0)

    def rate(self) -> float:
        with self.lock:
            if len(self.samples) < 2:
                return 0.0
            dt = self.samples[-1][0] - self.samples[0][0]
            return sum(h for _, h in self.samples[1:]) / dt if dt > 0 else 0.0


@dataclass
class MiningRequest:
    """generate / setgenerate on rank 0: mine with `script` until `blocks` are found (None =
    until stopped) or `max_tries` units of work (hashes; Equihash: solutions) are spent."""
    script: bytes
    blocks: int | None = None
    max_tries: int | None = None
    found: list = field(default_factory=list)
    tries: int = 0
    done: threading.Event = field(default_factory=threading.Event)
    error: str | None = None


@dataclass
class Job:
    job_id: int
    block: object
    height: int
    header: bytes         # the work packet's header field
    boundary: bytes
    prev: bytes
    tx_updated: int
    created: float
    script: bytes
    algo: int = ALGO_KAWPOW
    tries: int = 0


def algo_for_time(params, t: int) -> int:
    """Which proof of work a header with nTime `t` carries (src/primitives/block.cpp:38-74 +
    the Equihash extension's activation)."""
    if t >= params.equihash_activation_time:
        return ALGO_EQUIHASH
    if t >= params.kawpow_activation_time:
        return ALGO_KAWPOW
    return ALGO_X16RV2 if t >= params.x16rv2_activation_time else ALGO_X16R


def solved_block(params, block, algo: int, sh):
    """A copy of a job's template `block` with the share's proof of work in its header (the mining
    loop's leader and the Stratum server build their blocks with it)."""
    from ..chain.header import from_progpow

    act = params.kawpow_activation_time
    blk = _core.Block.deserialize(block.serialize(act), act)
    hdr = blk.header
    if algo == ALGO_KAWPOW:
        hdr.nonce64 = sh.nonce
        hdr.mix_hash = from_progpow(sh.mix_hash)
    elif algo == ALGO_EQUIHASH:
        hdr.nonce256 = sh.nonce256()
        hdr.solution = sh.solution
    else:
        hdr.nonce = sh.nonce
    blk.header = hdr
    return blk


class ChainLeader:
    """Rank 0's side of the loop: templates -> work packets, shares -> blocks.

    Templates come from BlockAssembler (src/miner.cpp:123-256) with IncrementExtraNonce
    (:508-525) per job; a job is replaced when the tip moves, when the pool changed and the job is
    older than `refresh_s` (the reference's 60 s mempool check, src/miner.cpp:700-705), when a
    legacy job has spent its 2^28 nNonce values per rank, or when the world was re-partitioned.
    Every share is checked again before its block is built; only shares of a job whose parent is
    still the tip are submitted (the reference's "generated block is stale" check,
    ProcessBlockFound)."""

    def __init__(self, state, *, refresh_s: float = 10.0, target_bits: int = 0, on_block=None,
                 state_path: str | None = None):
        from .assembler import ExtraNonce

        self.state = state
        self.refresh_s = float(refresh_s)
        self.miner_target = (1 << (256 - int(target_bits))) - 1 if target_bits else None
        self.on_block = on_block
        self.jobs: OrderedDict[int, Job] = OrderedDict()
        self.job_seq = 0
        self.extranonce = ExtraNonce()
        self.request: MiningRequest | None = None
        self.lock = threading.Lock()
        self.force_new = False
        self.stopping = False
        self.stats = {"shares": 0, "stale_shares": 0, "bad_shares": 0, "blocks": 0, "rejected": 0}
        self.per_rank: dict[int, dict] = {}
        self.rank_ids: tuple = ()  # ids of the world's ranks (MiningService tells): per_rank is keyed by id
        self.state_path = state_path
        self._resume = self._load_state()

    # ---------------------------------------------------------------- resume state
    def _load_state(self) -> dict:
        if not self.state_path or not os.path.exists(self.state_path):
            return {}
        try:
            with open(self.state_path) as f:
                return json.load(f)
        except (OSError, ValueError):
            return {}

    def save_state(self) -> None:
        if not self.state_path:
            return
        data = {"tip": _core.u256_hex(self.extranonce.prev) if self.extranonce.prev else None,
                "extranonce": self.extranonce.n, "job": self.job_seq, "time": int(time.time())}
        tmp = self.state_path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(data, f)
        os.replace(tmp, self.state_path)

    # ---------------------------------------------------------------- called from RPC threads
    def mine(self, script: bytes, blocks: int | None = None, max_tries: int | None = None) -> MiningRequest:
        req = MiningRequest(script, blocks, max_tries)
        with self.lock:
            old, self.request = self.request, req
            self.force_new = True
        if old is not None and not old.done.is_set():
            old.error = old.error or "superseded"
            old.done.set()
        return req

    def stop_mining(self) -> None:
        with self.lock:
            req, self.request = self.request, None
        if req is not None:
            req.done.set()

    def fail(self, why: str) -> None:
        """The loop cannot mine any more (every device evicted): end the request with an error."""
        with self.lock:
            req = self.request
        if req is not None and not req.done.is_set():
            req.error = why
            req.done.set()

    def shutdown(self) -> None:
        self.stop_mining()
        self.stopping = True

    # ---------------------------------------------------------------- called from the loop thread
    def _new_job(self, req: MiningRequest) -> Job:
        from ..chain.header import to_progpow
        from .assembler import BlockAssembler

        st = self.state
        tpl = BlockAssembler(st).create_new_block(req.script)
        blk = tpl.block
        hdr = blk.header
        if self.extranonce.prev != hdr.prev and self._resume.get("tip") == _core.u256_hex(hdr.prev):
            # a restart on the tip of a saved run: continue its extranonce sequence
            self.extranonce.prev, self.extranonce.n = hdr.prev, int(self._resume.get("extranonce", 0))
        self.extranonce.increment(blk, tpl.height)
        hdr = blk.header
        algo = algo_for_time(st.params, hdr.time)
        target = tpl.target if self.miner_target is None else min(tpl.target, self.miner_target)
        if algo == ALGO_KAWPOW:
            header = to_progpow(hdr.kawpow_header_hash())
        elif algo == ALGO_EQUIHASH:
            header = hdr.kawpow_input()  # version (with the extension bit), prev, merkle, time, bits, height
        else:
            header = hdr.legacy80()
        self.job_seq += 1
        job = Job(self.job_seq, blk, tpl.height, header, target.to_bytes(32, "big"), hdr.prev,
                  st.transactions_updated, time.time(), req.script, algo)
        self.jobs[job.job_id] = job
        while len(self.jobs) > 8:
            self.jobs.popitem(last=False)
        try:
            self.save_state()
        except OSError:
            pass
        return job

    def next_work(self, repartitioned: bool = False) -> Work:
        if self.stopping:
            return Work(flags=FLAG_STOP)
        with self.lock:
            req = self.request
            force = self.force_new or repartitioned
            self.force_new = False
        if req is None or req.done.is_set():
            return Work(flags=FLAG_IDLE)
        st = self.state
        tip = st.tip()
        cur = next(reversed(self.jobs.values())) if self.jobs else None
        stale = (cur is None or force or cur.prev != tip.hash or cur.script != req.script
                 or (st.transactions_updated != cur.tx_updated and time.time() - cur.created > self.refresh_s)
                 or (cur.algo in (ALGO_X16R, ALGO_X16RV2) and cur.tries >= 1 << 28))
        if not stale:
            return Work(cur.header, cur.boundary, cur.height, cur.job_id, 0, 0, cur.algo)
        job = self._new_job(req)
        return Work(job.header, job.boundary, job.height, job.job_id, 0, FLAG_CLEAN, job.algo)

    def _rank_stats(self, r: int) -> dict:
        r = self.rank_ids[r] if r < len(self.rank_ids) else r
        return self.per_rank.setdefault(r, {"shares": 0, "stale_shares": 0, "bad_shares": 0, "blocks": 0})

    def _check_share(self, job: Job, sh) -> bool:
        if job.algo == ALGO_KAWPOW:
            return sh.verify_full(job.height, job.header[:32], job.boundary)
        if job.algo == ALGO_EQUIHASH:
            from .search import equihash_block_hash

            p = _core.EquihashParams(200, 9)
            inp = job.header + sh.nonce256()
            ok = bool(_core.equihash_verify(p, inp, _core.equihash_unpack(p, sh.solution))[0])
            bh = equihash_block_hash(job.header, sh.nonce, sh.solution)
            return ok and bh == sh.block_hash and int.from_bytes(bh, "little") <= int.from_bytes(job.boundary, "big")
        return int.from_bytes(sh.block_hash, "little") <= int.from_bytes(job.boundary, "big")

    def _block_for(self, job: Job, sh):
        return solved_block(self.state.params, job.block, job.algo, sh)

    def on_results(self, records) -> None:
        records = [_as_record(r) for r in records]
        req = self.request
        for r, rec in enumerate(records):
            job = self.jobs.get(rec.job_id)
            if job is not None:
                job.tries += rec.hashes
        if req is None:
            return
        req.tries += sum(rec.hashes for rec in records)
        st = self.state
        for r, rec in enumerate(records):
            rs = self._rank_stats(r)
            for sh in rec.shares:
                if req.done.is_set():
                    break
                self.stats["shares"] += 1
                rs["shares"] += 1
                job = self.jobs.get(rec.job_id)
                if job is None or job.prev != st.tip().hash:
                    self.stats["stale_shares"] += 1
                    rs["stale_shares"] += 1
                    continue
                if not self._check_share(job, sh):
                    self.stats["bad_shares"] += 1
                    rs["bad_shares"] += 1
                    log.log_printf(f"miner: {ALGO_NAMES[job.algo]} share nonce {sh.nonce:#x} of job {rec.job_id} "
                                   f"(rank {r}) failed the host check; dropped")
                    continue
                blk = self._block_for(job, sh)
                res = st.process_new_block(blk)
                if not res.ok:
                    self.stats["rejected"] += 1
                    log.log_printf(f"miner: block of job {rec.job_id} rejected: {res.reject}")
                    if req.blocks is not None:  # generateBlocks: "ProcessNewBlock, block not accepted"
                        req.error = f"ProcessNewBlock, block not accepted: {res.reject}"
                        req.done.set()
                        break
                    continue
                bh = st.block_hash(blk.header)
                self.stats["blocks"] += 1
                rs["blocks"] += 1
                req.found.append(_core.u256_hex(bh))
                st._emit("block_found", bh)
                if self.on_block is not None:
                    self.on_block(blk)
                self.force_new = True
                if req.blocks is not None and len(req.found) >= req.blocks:
                    req.done.set()
                break  # one block per job: the next one builds on it
        if req.max_tries is not None and req.tries >= req.max_tries:
            req.done.set()


class BenchLeader:
    """A fixed synthetic job (bench.py): the same loop, no chain. Shares are kept for the host
    re-check after the timed region."""

    def __init__(self, work: Work, keep: int = 64):
        self.work = Work(work.header, work.boundary, work.height, work.job_id or 1, work.nonce_base, 0, work.algo)
        self.first = True
        self.keep = keep
        self.shares: list = []
        self.records = 0
        self.stopping = False

    def next_work(self, repartitioned: bool = False) -> Work:
        if self.stopping:
            return Work(flags=FLAG_STOP)
        if self.first or repartitioned:
            self.first = False
            w = self.work
            return Work(w.header, w.boundary, w.height, w.job_id, w.nonce_base, FLAG_CLEAN, w.algo)
        return self.work

    def on_results(self, records) -> None:
        for rec in (_as_record(r) for r in records):
            self.records += rec.has_result
            if len(self.shares) < self.keep:
                self.shares.extend(rec.shares[:self.keep - len(self.shares)])

    def shutdown(self) -> None:
        self.stopping = True


class MiningService:
    """The per-rank mining loop (see the module docstring). Rank 0 passes a leader."""

    def __init__(self, device, leader=None, *, window: int = 1 << 25, watchdog_s: float = 120.0,
                 collective_timeout_s: float = 60.0, grace_s: float | None = None, idle_sleep_s: float = 0.02,
                 record_windows: bool = False, max_failures: int = 3, rejoin=None, membership: int = 0):
        from ..parallel import world as W

        self.W = W
        self.dev = as_rank_device(device)
        self.leader = leader
        self.window = int(window)
        self.pipe = SearchPipeline(self.dev, watchdog_s)
        self.comm = Comm(collective_timeout_s)
        self.collective_timeout_s = float(collective_timeout_s)
        self.grace_s = float(grace_s) if grace_s is not None else 2 * self.collective_timeout_s + 1
        self.idle_sleep_s = float(idle_sleep_s)
        self.max_failures = int(max_failures)
        self.work = Work()
        self.cursor = 0
        self.rate = RateMeter()
        self.hashes_total = 0
        self.own_hashes = 0                           # this rank's own work
        self.first_result_at: float | None = None     # wall clock of this rank's first completed window
        self.rank_hashes: dict[int, int] = {}
        self.rank_info_raw: dict[int, dict] = {}
        self.kernel_windows = {"jit": 0, "generic": 0}  # GPU KawPow windows by kernel, all ranks (rank 0 only)
        self.rank_rates: dict[int, RateMeter] = {}
        self.steps = 0
        self.membership = int(membership)  # a rank that joined late starts at the membership it joined
        self.rejoin = rejoin               # rank 0 with -minerrejoin: the Rejoiner that brings lost ranks back
        self.reforms = 0
        self.reform_at = int(os.environ.get("NODEXA_MINER_REFORM_AT", "0"))  # test hook
        self.repartitioned = False
        self.windows: list[tuple[int, int, int]] | None = [] if record_windows else None
        self._light_thread: threading.Thread | None = None
        self._thread: threading.Thread | None = None
        self.error: BaseException | None = None
        self.last_step_ms = 0.0
        self.coll_ms = 0.0
        self.last_end_ms = 0.0  # device clock of the last window this rank took (SlotResult.end_ms)
        self.failures = 0          # consecutive failed windows on this rank
        self.total_failures = 0
        self.dev_alive = True
        self.last_error = ""
        self._tell_world_size()

    def _tell_world_size(self) -> None:
        """A leader that declares `world_size` learns the current one (at start, after a shrink): a
        pool's nonce prefix is split over the ranks by it (miner/stratum_client.StratumLeader)."""
        if self.leader is not None and hasattr(self.leader, "world_size"):
            self.leader.world_size = self.world_size
        if self.leader is not None and hasattr(self.leader, "rank_ids"):
            self.leader.rank_ids = self.member_ids

    @property
    def rank(self) -> int:
        return self.comm.w.rank

    @property
    def world_size(self) -> int:
        return self.comm.w.world_size

    @property
    def member_ids(self) -> tuple:
        """The id of every rank of the current world (its rank in the first world), by rank."""
        return self.comm.w.member_ids

    def hashrate(self) -> float:
        return self.rate.rate()

    # ---------------------------------------------------------------- one step
    def _next_epoch_vote(self) -> int:
        """1 when this rank has the next epoch's light cache (prebuild window only)."""
        w = self.work
        if w.idle or w.algo != ALGO_KAWPOW or w.height % _core.EPOCH_LENGTH < _core.EPOCH_LENGTH - EPOCH_PREBUILD_WINDOW:
            return 0
        nxt = w.epoch + 1
        if self.dev.epoch_ready(nxt):
            return 0
        t = self._light_thread
        if t is None:
            t = threading.Thread(target=_core.get_epoch_context, args=(nxt,), name=f"light-{nxt}", daemon=True)
            self._light_thread = t
            t.start()
        if t.is_alive():
            return 0
        return 1

    def _window_start(self, w: Work) -> int:
        if w.algo in (ALGO_X16R, ALGO_X16RV2):
            return ((self.rank & 0xF) << 28) | (self.cursor & 0x0FFFFFFF)
        return (w.nonce_base + (self.rank << w.rank_shift) + self.cursor) & 0xFFFFFFFFFFFFFFFF

    def _clip_window(self, w: Work, count: int) -> int:
        """`count` clipped to the end of this rank's range of a packet that names its rank_shift, in
        whole launch granules; 0 once the range is used up."""
        if not w.rank_bounded or w.algo != ALGO_KAWPOW:
            return count
        left = (1 << w.rank_shift) - self.cursor
        if count <= left:
            return count
        b = self.dev.block_for(w.height)
        return max(0, left) // b * b

    def _device_failure(self, err: Exception) -> None:
        self.failures += 1
        self.total_failures += 1
        self.last_error = f"{type(err).__name__}: {err}"
        log.log_printf(f"miner rank {self.rank}: window failed ({self.last_error}), {self.failures} in a row")
        if self.failures >= self.max_failures and self.dev_alive:
            self.dev_alive = False
            log.log_printf(f"miner rank {self.rank}: device evicted after {self.failures} failed windows")
            try:
                self.pipe.drain()
            except Exception:  # noqa: BLE001 — the device is being given up
                self.pipe.inflight = None
            if self.leader is None:
                raise DeviceEvicted(self.last_error)

    def step(self) -> bool:
        """One iteration of the loop on this rank; False once a stop packet has been processed."""
        t0 = time.perf_counter()
        w = self.work
        res = None
        exhausted = False
        try:
            count = 0
            if not w.idle and self.dev_alive:
                count = self._clip_window(w, self.dev.window_for(w, self.window))
                exhausted = count <= 0  # nothing of this job is left for this rank: no window, no wrap
            if count <= 0:
                res = self.pipe.drain() if self.pipe.inflight is not None else None
                if res is None:
                    time.sleep(self.idle_sleep_s)
            else:
                start = self._window_start(w)
                if self.windows is not None:
                    self.windows.append((w.job_id, start, count))
                self.cursor += count  # before the step: a window that fails was still searched once
                res = self.pipe.step(w, start, count)
            if res is not None:
                self.failures = 0
                self.last_end_ms = res.end_ms
                self.own_hashes += res.hashes
                if self.first_result_at is None:
                    self.first_result_at = time.time()
        except DeviceFault as e:
            self._device_failure(e)
            res = None
        vote = self._next_epoch_vote()
        dag = self._kawpow_dag()
        # resident or being built: what a peer needs to know to choose how it builds (search.dag_build_mode)
        rec = pack_record(res, coll_ms=self.coll_ms, failures=self.failures,
                          epochs=set(self.dev.resident_epochs()) | set(self.dev.pending_epochs()),
                          alive=self.dev_alive, device=int(getattr(self.dev, "device", -1)), vote=bool(vote),
                          exhausted=exhausted, dag_bad=dag.take_dag_bad() if dag is not None else False)
        tc = time.perf_counter()
        gathered = self.comm.all_gather(rec)
        coll = time.perf_counter() - tc
        hashes, votes = record_totals(gathered)
        self.hashes_total += hashes
        self.rate.add(hashes)
        view = self.dev.world_view
        if view is not None:
            view.update(record_epochs(gathered))
        if vote and votes == self.world_size:
            # every rank holds the light cache: all start the build on this step (collective, unless
            # a peer already holds that epoch: then the ranks that lack it build alone)
            self.dev.prebuild(w.epoch + 1)
            self._light_thread = None
            if view is not None:
                view.vote_passed(w.epoch + 1)
        payload = None
        if self.leader is not None:
            records = [unpack_record(r) for r in gathered]
            now = time.monotonic()
            ids = self.member_ids
            for i, rec_i in enumerate(records):
                i = ids[i]  # the counters follow the rank's id through a shrink and a re-join
                self.rank_hashes[i] = self.rank_hashes.get(i, 0) + rec_i.hashes
                self.rank_rates.setdefault(i, RateMeter()).add(rec_i.hashes, now)
                info = self.rank_info_raw.setdefault(i, {"aborted": 0, "windows": 0, "jit_windows": 0,
                                                         "generic_windows": 0, "dag_check_events": 0})
                info["dag_check_events"] += rec_i.dag_bad
                info.update(alive=rec_i.alive, failures=rec_i.failures, epochs=rec_i.epochs, device=rec_i.device,
                            coll_ms=rec_i.coll_ms)
                if rec_i.has_result:
                    info["windows"] += 1
                    info["aborted"] += rec_i.aborted
                    info.update(algo=rec_i.algo, device_ms=rec_i.device_ms)
                    if rec_i.kernel:
                        info["kernel"] = rec_i.kernel
                        info[rec_i.kernel + "_windows"] += 1
                        self.kernel_windows[rec_i.kernel] += 1
            self.leader.on_results(records)
            if self.world_size == 1 and not self.dev_alive and hasattr(self.leader, "fail"):
                self.leader.fail("no mining device left (all evicted): " + self.last_error)
            k = self._reform_due()
            if k is not None:
                payload = Work(nonce_base=k, flags=FLAG_IDLE | FLAG_REFORM).pack()
            else:
                payload = self.leader.next_work(self.repartitioned).pack()
                self.repartitioned = False
        tc = time.perf_counter()
        new = Work.unpack(self.comm.broadcast(payload, WORK_SIZE))
        self.coll_ms = (coll + time.perf_counter() - tc) * 1e3
        if new.job_id != w.job_id:
            self.cursor = 0
        if new.flags & FLAG_CLEAN or new.idle:
            self.dev.abort()  # the window queued for the old job stops on the device
        self.work = new
        self.steps += 1
        if new.flags & FLAG_REFORM:
            self._reform(new.nonce_base)
        self.last_step_ms = (time.perf_counter() - t0) * 1e3
        return not new.stop

    def _kawpow_dag(self):
        """This rank's KawPow device if it checks its DAGs (search.GpuSearchDevice with dag_check)."""
        kp = getattr(self.dev, "kawpow", None)
        return kp if getattr(kp, "dag_check", False) else None

    # ---------------------------------------------------------------- growing the world back
    def _reform_due(self) -> int | None:
        """Rank 0, once per step: the join attempt whose newcomer is ready (Rejoiner.poll), or the
        NODEXA_MINER_REFORM_AT test hook (the same members again, once). Returns the number of the
        store key that names the members, which goes out in a FLAG_REFORM packet."""
        if self.reform_at and self.steps + 1 == self.reform_at and self.W.store() is not None:
            k = max(self.membership, self.W.epoch()) + 1
            publish_members(self.W.store(), k, self.member_ids, k)
            return k
        if self.rejoin is not None and not getattr(self.leader, "stopping", False):
            return self.rejoin.poll(self)
        return None

    def _reform(self, k: int) -> None:
        """Every rank, on the FLAG_REFORM packet: drain, make the world again over the members that
        rank 0 published (parallel/world.reform) and start over as after a shrink: a new loop
        communicator, a reset cursor, and rank 0 issues a clean job, so the nonce partition re-derives
        from (rank, world_size). If the new world cannot be formed (a member died in between) the old
        members form the next membership instead; a newcomer left outside ends itself."""
        W = self.W
        info = json.loads(W.store().get(f"m{k}/members"))
        members, m = [int(x) for x in info["members"]], int(info["membership"])
        old = list(self.member_ids)
        try:
            self.pipe.drain()
        except DeviceHung:
            raise
        except Exception:  # noqa: BLE001 — the window of the old world is discarded
            self.pipe.inflight = None
        timeout = int(max(5.0, self.collective_timeout_s))
        try:
            W.reform(members, m, timeout_s=timeout)
        except Exception as e:  # noqa: BLE001 — a member was lost while the world was being made
            log.log_printf(f"miner rank id {old[self.rank] if self.rank < len(old) else '?'}: re-forming over "
                           f"{members} failed ({e}); the ranks {old} continue")
            m += 1
            W.reform(old, m, timeout_s=timeout)
            if self.rejoin is not None:
                self.rejoin.reform_failed()
        else:
            if self.rejoin is not None:
                self.rejoin.reformed(members)
        self.comm.rebind()
        self.membership = m
        self.reforms += 1
        if self.dev.world_view is not None:
            self.dev.world_view.reset()
        self._tell_world_size()
        self.work = Work()
        self.cursor = 0
        self.repartitioned = True
        log.log_printf(f"miner: membership {m}: rank {self.rank} of {self.world_size} (ids {list(self.member_ids)})")

    # ---------------------------------------------------------------- observability
    def rank_info(self) -> list[dict]:
        """getmininginfo.gpus[]: one entry per rank of the world (rank 0 only). With -minerrejoin a
        rank that is out keeps its entry (rank -1, its counters as they stood); `state` is mining /
        evicted / rejoining / refused, `lives` the processes started for it so far, `last_exit` the
        exit code of the last one that ended, `rejoin_in_s` the time until it may be spawned again."""
        out = []
        stats = getattr(self.leader, "per_rank", {}) if self.leader is not None else {}
        ids = list(self.member_ids)
        away = [g for g in (self.rejoin.known_ids() if self.rejoin is not None else []) if g not in ids]
        dag = self._kawpow_dag()
        local = dag.dag_counters() if dag is not None else {}  # the local device's own counters
        for r, gid in [(r, g) for r, g in enumerate(ids)] + [(-1, g) for g in away]:
            info = self.rank_info_raw.get(gid, {})
            rs = stats.get(gid, {})
            algo = info.get("algo", self.work.algo)
            shares, stale = rs.get("shares", 0), rs.get("stale_shares", 0)
            rate = self.rank_rates[gid].rate() if gid in self.rank_rates and r >= 0 else 0.0
            life = self.rejoin.describe(gid) if self.rejoin is not None else {}
            out.append({
                "rank": r,
                "id": gid,
                "state": life.get("state", "mining" if (info.get("alive", True) if gid else self.dev_alive)
                                  else "evicted"),
                "lives": life.get("lives", 1),
                "last_exit": life.get("last_exit"),
                "rejoin_in_s": life.get("rejoin_in_s"),
                "device": info.get("device", -1),
                "alive": (info.get("alive", True) if gid else self.dev_alive) and r >= 0,
                "algo": ALGO_NAMES[algo] if algo < len(ALGO_NAMES) else str(algo),
                ("solutionspersec" if algo == ALGO_EQUIHASH else "hashespersec"): round(rate, 1),
                "mhs": round(rate / 1e6, 3) if algo != ALGO_EQUIHASH else None,
                "hashes": int(self.rank_hashes.get(gid, 0)),
                "shares": shares,
                "stale_shares": stale,
                "stale_rate": round(stale / shares, 4) if shares else 0.0,
                "bad_shares": rs.get("bad_shares", 0),
                "blocks": rs.get("blocks", 0),
                "epochs_resident": info.get("epochs", []),
                "last_device_ms": round(info.get("device_ms", 0.0), 3),
                "last_step_ms": round(self.last_step_ms, 3),
                "collective_ms": round(info.get("coll_ms", 0.0), 3),
                "aborted_workgroups": info.get("aborted", 0),
                "windows": info.get("windows", 0),
                "kernel": info.get("kernel", ""),
                "generic_windows": info.get("generic_windows", 0),
                "jit_windows": info.get("jit_windows", 0),
                "failures": info.get("failures", 0),
                "dag_check_events": info.get("dag_check_events", 0),
            })
            if r == self.rank:
                out[-1].update({k: v for k, v in local.items() if k != "dag_check_events"})
        return out

    # ---------------------------------------------------------------- failures
    def recover(self, err: Exception) -> None:
        """Survivor side of a lost rank: membership by rendezvous-store registration, then a new
        group over the registered ranks. Raises if the leader (global rank 0) is among the lost."""
        import torch.distributed as dist

        W = self.W
        w = W.get()
        members = list(w.ranks or range(w.world_size))
        me = w.global_rank(w.rank)
        self.membership += 1
        store = dist.distributed_c10d._get_default_store()
        prefix = f"nodexa/miner/m{self.membership}/alive/"
        store.set(prefix + str(me), "1")
        log.log_printf(f"miner rank {me}: collective failed ({err}); membership round {self.membership}")
        deadline = time.monotonic() + self.grace_s
        alive = [me]
        while time.monotonic() < deadline:
            alive = [r for r in members if store.check([prefix + str(r)])]
            if len(alive) == len(members):
                break
            time.sleep(0.05)
        if members[0] not in alive:
            raise RuntimeError(f"miner leader (rank {members[0]}) is gone")
        try:
            self.pipe.drain()
        except DeviceHung:
            raise
        except Exception:  # noqa: BLE001 — the window of the broken step is discarded
            pass
        self.comm.abort()
        # the survivors arrive here up to one collective timeout apart (a rank next to the lost one
        # sees its socket close at once, the others wait their collective out), so the new group's
        # connect gets the grace period (gloo connects its full mesh under the group's timeout; every
        # collective on it stays bounded by Comm's own). RCCL connects lazily and keeps the timeout.
        conn = self.collective_timeout_s if w.backend == "nccl" else max(self.collective_timeout_s, self.grace_s)
        W.shrink(alive, timeout_s=int(max(1, conn)))
        self.comm.rebind()
        self._tell_world_size()
        self.work = Work()
        self.cursor = 0
        self.repartitioned = True
        log.log_printf(f"miner rank {me}: continuing as rank {self.rank} of {self.world_size} (ranks {alive})")

    def run(self, stop: threading.Event | None = None) -> None:
        """Loop until a stop packet (followers) or `stop` is set and the stop packet went out (leader)."""
        while True:
            if stop is not None and stop.is_set() and self.leader is not None:
                self.leader.shutdown()
            try:
                if not self.step():
                    break
            except CollectiveError as e:
                self.recover(e)
        try:
            self.pipe.drain()
        except Exception:  # noqa: BLE001
            pass

    def start(self) -> "MiningService":
        """Run the loop on a background thread (rank 0 inside the node)."""
        self._stop = threading.Event()

        def go():
            try:
                self.run(self._stop)
            except BaseException as e:  # noqa: BLE001 — surfaced through getmininginfo / logs
                self.error = e
                log.log_printf(f"miner loop stopped: {type(e).__name__}: {e}")
                if self.leader is not None and getattr(self.leader, "request", None) is not None:
                    self.leader.request.error = str(e)
                    self.leader.request.done.set()

        self._thread = threading.Thread(target=go, name="miner-service", daemon=True)
        self._thread.start()
        return self

    def stop(self, timeout: float = 30.0) -> None:
        if self._thread is None:
            return
        self._stop.set()
        self._thread.join(timeout)
        self._thread = None


class Rejoiner:
    """Rank 0's side of a lost rank's return (-minerrejoin), driven from the loop so that no
    collective has to fail first. `poll` runs once per step:

      * the supervisor reported that a member's process ended (75 hung, 76 evicted, a signal): the
        rank is `evicted`; the survivors shrink on their own (MiningService.recover);
      * once the world no longer holds the rank and RejoinPolicy says "spawn", the supervisor starts
        a new process for it with join_membership k; one attempt at a time. The newcomer prepares
        alone (imports, its device, the light cache of the epoch under "join/<k>/epoch"), sets
        "join/<k>/ready/<id>" and blocks on "m<k>/members";
      * when the ready key is there (a non-blocking check), rank 0 publishes the members and `poll`
        returns k: the next work packet carries FLAG_REFORM and every rank re-forms the world;
      * a newcomer whose exit is reported before it was ready cancels the attempt, which counts as
        a life and as a failed re-join; the survivors never see FLAG_REFORM for it.

    The leader, id 0, is never replaced: when its own device is evicted it keeps leading without
    searching, as without -minerrejoin."""

    def __init__(self, supervisor, policy, *, gpus: list[int], env: dict, argv: list | None = None):
        from ..utils.metrics import REGISTRY

        self.sup = supervisor
        self.policy = policy
        self.gpus = list(gpus)          # id -> device index
        self.env = dict(env)            # what every follower gets (follower_env, the ports)
        self.argv = argv                # test hook: another program in place of the follower
        self.ranks = {g: {"state": "mining", "lives": 1, "last_exit": None} for g in range(len(self.gpus))}
        self.attempt: dict | None = None
        self.last_k = 0
        self.counters = {"miner_rejoins_total": 0, "miner_rejoin_failed_total": 0, "miner_rejoin_refused_total": 0}
        self.metrics = REGISTRY
        self.last_event: dict = {}      # id -> wall clock of its last `exited` event (measurements)
        self.exit_log: list[dict] = []  # every `exited` event, in order
        self.lock = threading.Lock()

    def spawn_first(self) -> None:
        """The followers of the first world, life 0."""
        for g in range(1, len(self.gpus)):
            self.sup.spawn(gpu=self.gpus[g], rank=g, world_size=len(self.gpus), env=self.env)

    def known_ids(self) -> list[int]:
        return sorted(self.ranks)

    def describe(self, g: int) -> dict:
        with self.lock:
            d = dict(self.ranks.get(g, {}))
        if d.get("state") == "evicted":
            t = self.policy.rejoin_in(self.policy.clock(), g)
            d["rejoin_in_s"] = None if t is None else round(t, 3)
        return d

    def _count(self, name: str) -> None:
        self.counters[name] += 1
        self.metrics.inc(name, 1, worker="service")

    def _exited(self, ev: dict) -> None:
        g, code = int(ev["rank"]), int(ev["code"])
        self.exit_log.append(ev)
        st = self.ranks.get(g)
        if st is None or code == 0:
            return
        self.last_event[g] = time.time()
        self.policy.record_exit(g)
        with self.lock:
            st["last_exit"] = code
            st["state"] = "evicted"
        if self.attempt is not None and self.attempt["id"] == g:
            self.attempt = None
            self._count("miner_rejoin_failed_total")
            log.log_printf(f"miner: rank id {g} ended with {code} before it was ready; the re-join is cancelled")
        else:
            log.log_printf(f"miner: rank id {g} ended with {code} (life {ev.get('life')})")

    def poll(self, svc: "MiningService") -> int | None:
        for ev in self.sup.events():
            if ev.get("event") == "exited":
                self._exited(ev)
            elif ev.get("event") == "error":
                log.log_printf(f"miner supervisor: {ev.get('error')}")
                a = self.attempt
                if a is not None and not a.get("published"):
                    # the spawn was not carried out (the last process of that rank has not ended yet):
                    # the attempt is over, and the policy's delay applies before the next one
                    self.attempt = None
                    with self.lock:
                        self.ranks[a["id"]]["state"] = "evicted"
                        self.ranks[a["id"]]["lives"] -= 1
                    self.policy.record_exit(a["id"])
                    self._count("miner_rejoin_failed_total")
        store = svc.W.store()
        if store is None:
            return None
        members = list(svc.member_ids)
        if self.attempt is not None:
            a = self.attempt
            if a.get("published") or not store.check([f"join/{a['k']}/ready/{a['id']}"]):
                return None
            m = max(a["k"], svc.membership + 1)
            publish_members(store, a["k"], sorted(set(members) | {a["id"]}), m)
            a["published"] = True
            return a["k"]
        now = self.policy.clock()
        for g, st in sorted(self.ranks.items()):
            if g == 0 or st["state"] not in ("evicted", "refused") or g in members:
                continue  # (still a member: the survivors have not shrunk yet)
            what = self.policy.decide(now, g)
            if what == "refused":
                if st["state"] == "refused":
                    continue  # said once; it becomes eligible again when its exits leave the window
                with self.lock:
                    st["state"] = "refused"
                self._count("miner_rejoin_refused_total")
                log.log_printf(f"miner: rank id {g} (gpu {self.gpus[g]}) stays evicted: {self.policy.recent_exits(now, g)} "
                               f"exits within {self.policy.window_s:.0f} s (-minerrejoinmax={self.policy.max_exits})")
            elif what == "spawn":
                k = self.last_k = max(self.last_k, svc.membership, svc.W.epoch()) + 1  # never a key used before
                w = svc.work
                store.set(f"join/{k}/epoch", str(w.epoch if not w.idle and w.algo == ALGO_KAWPOW else -1))
                self.sup.spawn(gpu=self.gpus[g], rank=g, world_size=len(members) + 1, env=self.env,
                               join_membership=k, argv=self.argv)
                with self.lock:
                    st["state"] = "rejoining"
                    st["lives"] += 1
                self.attempt = {"id": g, "k": k}
                log.log_printf(f"miner: starting life {st['lives'] - 1} of rank id {g} (gpu {self.gpus[g]}), "
                               f"join membership {k}")
                break
        return None

    def reformed(self, members: list[int]) -> None:
        a, self.attempt = self.attempt, None
        if a is not None and a["id"] in members:
            with self.lock:
                self.ranks[a["id"]]["state"] = "mining"
            self._count("miner_rejoins_total")

    def reform_failed(self) -> None:
        """The world with the newcomer could not be formed; its exit event will follow and count
        against it (RejoinPolicy)."""
        a, self.attempt = self.attempt, None
        if a is not None:
            with self.lock:
                self.ranks[a["id"]]["state"] = "evicted"
            self._count("miner_rejoin_failed_total")

    def wait_followers(self, timeout: float = 30.0) -> None:
        """After the stop packet: until every follower has ended by itself (their exits are logged)."""
        deadline = time.monotonic() + timeout
        while time.monotonic() < deadline:
            for ev in self.sup.events():
                if ev.get("event") == "exited":
                    self.exit_log.append(ev)
            try:
                if not self.sup.status()["children"]:
                    break
            except Exception:  # noqa: BLE001 — the supervisor is gone, and its followers with it
                break
            time.sleep(0.05)
        for ev in self.sup.events():
            if ev.get("event") == "exited":
                self.exit_log.append(ev)

    def close(self) -> None:
        self.sup.stop()


def start_rejoin_world(gpus: list[int], port: int, *, cpu: bool, env: dict, policy, argv: list | None = None):
    """What rank 0 does in place of spawn_followers when lost ranks are to come back: start the
    supervisor (before this process touches a GPU), have it start ranks 1..n-1, and return the
    Rejoiner for MiningService(rejoin=...) and the port of the stand-alone rendezvous store for
    parallel/world.init(store_port=...). `port`: the env:// port the followers are told anyway."""
    import socket

    from . import supervisor as SV

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        store_port = sk.getsockname()[1]
    full = dict(env)
    full.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "NODEXA_MINER_CPU": "1" if cpu else "0",
                 "NODEXA_MINER_STORE_PORT": str(store_port), "PYTHONPATH": SV.follower_pythonpath()})
    rj = Rejoiner(SV.SupervisorClient(), policy, gpus=gpus, env=full, argv=argv)
    rj.spawn_first()
    return rj, store_port


class Miner:
    """The node's miner front-end (node.miner): generate / generatetoaddress / setgenerate /
    getmininginfo on top of the mining service's leader. Every proof of work and every device
    goes through the one loop; there is no second, thread-per-backend miner."""

    def __init__(self, state, service: MiningService):
        from ..utils.metrics import REGISTRY

        self.state = state
        self.service = service
        self.leader: ChainLeader = service.leader
        self.metrics = REGISTRY
        self._req: MiningRequest | None = None
        self.generating = False
        self._last_hashes = 0
        self._last_shares = 0
        self._last_kernel_windows = {"jit": 0, "generic": 0}
        self._last_dag = {"dag_scrubs": 0, "dag_bad_chunks": 0, "dag_repaired_items": 0}

    @classmethod
    def local(cls, state, *, window: int = 4096, fail_rate: float = 0.0, drop_rate: float = 0.0,
              max_failures: int = 3, watchdog_s: float = 120.0, state_path: str | None = None,
              target_bits: int = 0, start: bool = True) -> "Miner":
        """A single-rank miner on this host's CPU devices (CPU-only nodes, tests)."""
        from .search import CpuSearchDevice, FaultInjectingDevice, RankDevice

        dev = RankDevice(CpuSearchDevice(max_window=window))
        if fail_rate or drop_rate:
            dev = FaultInjectingDevice(dev, fail_rate, drop_rate, seed=0)
        leader = ChainLeader(state, state_path=state_path, target_bits=target_bits)
        svc = MiningService(dev, leader, window=window, watchdog_s=watchdog_s, max_failures=max_failures)
        return cls(state, svc.start() if start else svc)

    @property
    def hashrate(self) -> float:
        """getmininginfo.hashespersec: the rate summed over every rank's gathered record
        (src/miner.cpp:685-687)."""
        return self.service.hashrate()

    def workers(self) -> list[dict]:
        return [{"worker": g["rank"], "backend": f"{getattr(self.service.dev, 'name', 'dev')}-rank{g['rank']}",
                 "alive": g["alive"], "hashes": g["hashes"], "blocks": g["blocks"], "failures": g["failures"]}
                for g in self.service.rank_info()]

    def _export_metrics(self) -> None:
        h, s = self.service.hashes_total, self.leader.stats["shares"]
        if h > self._last_hashes:
            self.metrics.inc("miner_hashes_total", h - self._last_hashes, worker="service")
        if s > self._last_shares:
            self.metrics.inc("miner_shares_total", s - self._last_shares, worker="service")
        self._last_hashes, self._last_shares = h, s
        for kind, n in self.service.kernel_windows.items():
            if n > self._last_kernel_windows[kind]:
                self.metrics.inc(f"miner_kawpow_{kind}_windows_total", n - self._last_kernel_windows[kind], worker="service")
                self._last_kernel_windows[kind] = n
        dag = self.service._kawpow_dag()
        if dag is not None:
            now = dag.dag_counters()
            for key, last in self._last_dag.items():
                if now[key] > last:
                    self.metrics.inc(key + "_total", now[key] - last, worker="service")
                    self._last_dag[key] = now[key]

    def generate(self, script_pubkey: bytes, nblocks: int, max_tries: int = 1_000_000) -> list[str]:
        """generateBlocks: the new block hashes (display hex), mined by the service."""
        svc = self.service
        if svc.error is not None:
            raise RuntimeError(f"miner service stopped: {svc.error}")
        req = self.leader.mine(script_pubkey, blocks=nblocks, max_tries=max_tries)
        while not req.done.wait(0.2):
            if svc.error is not None:
                raise RuntimeError(f"miner service stopped: {svc.error}")
        self._export_metrics()
        for _ in req.found:
            self.metrics.inc("miner_blocks_total", 1, worker="service")
        if req.error is not None and not req.found:
            if req.error == "superseded":
                return []
            raise RuntimeError(req.error)
        return list(req.found)

    def set_generate(self, on: bool, script_pubkey: bytes | None = None) -> None:
        self.stop()
        if not on:
            return
        if script_pubkey is None:
            raise ValueError("setgenerate true needs -miningaddress")
        self._req = self.leader.mine(script_pubkey)  # until setgenerate false
        self.generating = True

    def stop(self) -> None:
        if self._req is not None:
            self.leader.stop_mining()
            for _ in self._req.found:
                self.metrics.inc("miner_blocks_total", 1, worker="service")
            self._req = None
        self._export_metrics()
        self.generating = False

    def close(self) -> None:
        """Node shutdown: stop mining and end the service loop (its stop packet ends every rank)."""
        self.stop()
        self.service.stop()


# -------------------------------------------------------------------- follower processes
def spawn_followers(gpus: list[int], port: int, cpu: bool = False, extra_env: dict | None = None) -> list:
    """Start ranks 1..n-1 of the miner world as child processes (before this process touches a GPU;
    they are started, never exec'd over a GPU process). Rank r drives gpus[r]."""
    import subprocess

    procs = []
    n = len(gpus)
    for r in range(1, n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_RANK": str(r), "MASTER_ADDR": "127.0.0.1",
                    "MASTER_PORT": str(port), "NODEXA_MINER_DEVICE": str(gpus[r]),
                    "NODEXA_MINER_CPU": "1" if cpu else "0"})
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, "-m", "nodexa_chain_core_amd.miner.service"], env=env))
    return procs


def follower_env(*, timeout: float, watchdog, max_failures: int, fail_rate: float, drop_rate: float,
                 jit_mode: str = "wait", window=None) -> dict[str, str]:
    """The node's miner flags as the environment of the follower ranks it spawns (follower_main
    reads them back): -minercollectivetimeout, -minerwatchdog, -minermaxfailures, -gpufailrate,
    -dropshare, -kawpowjit and, when set, -gpuintensity."""
    env = {"NODEXA_MINER_COLLECTIVE_TIMEOUT": str(timeout), "NODEXA_MINER_WATCHDOG": str(watchdog),
           "NODEXA_MINER_MAXFAILURES": str(max_failures), "NODEXA_MINER_FAILRATE": str(fail_rate),
           "NODEXA_MINER_DROPSHARE": str(drop_rate), "NODEXA_MINER_KAWPOWJIT": jit_mode}
    if window:
        env["NODEXA_MINER_WINDOW"] = str(window)
    return env


def follower_jit_mode() -> str:
    """-kawpowjit as the node handed it to this follower rank (validated: the node already did)."""
    from ..utils.config import KAWPOW_JIT_MODES

    mode = os.environ.get("NODEXA_MINER_KAWPOWJIT", "wait") or "wait"
    if mode not in KAWPOW_JIT_MODES:
        raise ValueError(f"NODEXA_MINER_KAWPOWJIT={mode}: expected one of {', '.join(KAWPOW_JIT_MODES)}")
    return mode


def injected_fail_rate(rate: float, rank_id: int) -> float:
    """-gpufailrate as it applies to this process. Two test hooks (environment only) narrow it:
    NODEXA_MINER_FAILRATE_RANK=<id>: only the rank with that id fails; NODEXA_MINER_FAILRATE_LIVES=<n>:
    only while NODEXA_MINER_LIFE < n, so a re-spawned rank comes back healthy. The faults are the
    software ones of search.FaultInjectingDevice."""
    only = os.environ.get("NODEXA_MINER_FAILRATE_RANK")
    if only not in (None, "") and int(only) != int(rank_id):
        return 0.0
    lives = os.environ.get("NODEXA_MINER_FAILRATE_LIVES")
    if lives not in (None, "") and int(os.environ.get("NODEXA_MINER_LIFE", "0")) >= int(lives):
        return 0.0
    return float(rate)


def make_rank_device(cpu: bool, device_index: int | None = None, collective_dag: bool = False, window: int = 4096,
                     fail_rate: float = 0.0, drop_rate: float = 0.0, seed: int = 0, eq_window: int = 1,
                     jit_mode: str = "wait", joined_late: bool = False):
    """This rank's RankDevice: GPU KawPow + GPU Equihash (built on first use) + GPU X16R, or the
    host equivalents; -gpufailrate / -dropshare wrap it. `joined_late`: the rank enters a running
    world, whose DAGs it builds alone (search.dag_build_mode)."""
    from .equihash_search import EquihashCpuDevice
    from .search import CpuSearchDevice, FaultInjectingDevice, RankDevice

    if cpu:
        dev = RankDevice(CpuSearchDevice(max_window=window), EquihashCpuDevice(eq_window))
    else:
        from .equihash_search import EquihashGpuDevice
        from .search import GpuSearchDevice, LegacyGpuDevice

        idx = int(device_index or 0)
        kawpow = GpuSearchDevice(idx, collective_dag=collective_dag, jit_mode=jit_mode)
        if joined_late:
            kawpow.world_view.joined_late = True
        dev = RankDevice(kawpow, equihash_factory=lambda: EquihashGpuDevice(idx), legacy=LegacyGpuDevice(idx))
    if fail_rate or drop_rate:
        dev = FaultInjectingDevice(dev, fail_rate, drop_rate, seed=seed)
    return dev


def join_world(k: int, my_id: int, store_port: int, *, cpu: bool, device_index: int | None):
    """A re-spawned rank before it has a world (join attempt `k`): open the device, build what needs
    no peer (the light cache of the epoch rank 0 named under "join/<k>/epoch"), set
    "join/<k>/ready/<id>" and block on "m<k>/members" under the rendezvous timeout. Returns
    (member ids, membership), or None when nobody named the members in time."""
    import datetime as dt

    from ..parallel import world as W

    if not cpu:
        import torch

        torch.cuda.set_device(int(device_index or 0))
        torch.cuda.current_stream().synchronize()  # the device is open before this rank says "ready"
    store = W.connect_store(store_port)
    try:
        epoch = int(store.get(f"join/{k}/epoch"))
    except Exception:  # noqa: BLE001 — nothing named: nothing to prepare
        epoch = -1
    if epoch >= 0:
        _core.get_epoch_context(epoch)
    store.set(f"join/{k}/ready/{my_id}", "1")
    try:
        store.wait([f"m{k}/members"], dt.timedelta(seconds=W.rendezvous_timeout()))
    except Exception as e:  # noqa: BLE001 — the store's timeout error
        log.log_printf(f"miner rank id {my_id}: not named a member of membership {k} in time ({e})")
        return None
    info = json.loads(store.get(f"m{k}/members"))
    return [int(x) for x in info["members"]], int(info["membership"])


def follower_main() -> int:
    """Entry point of ranks >= 1 (spawned by the node or launched by torchrun)."""
    from ..parallel import world as W

    cpu = os.environ.get("NODEXA_MINER_CPU", "0") == "1"
    dev_index = os.environ.get("NODEXA_MINER_DEVICE")
    timeout = float(os.environ.get("NODEXA_MINER_COLLECTIVE_TIMEOUT", "60"))
    watchdog = float(os.environ.get("NODEXA_MINER_WATCHDOG", "120"))
    window = int(os.environ.get("NODEXA_MINER_WINDOW", str(1 << 25)))
    store_port = os.environ.get("NODEXA_MINER_STORE_PORT")
    join = os.environ.get("NODEXA_MINER_JOIN_MEMBERSHIP")
    life = int(os.environ.get("NODEXA_MINER_LIFE", "0"))
    my_id = int(os.environ.get("RANK", "0"))
    kw = {"use_gpu": not cpu, "device_index": None if dev_index is None else int(dev_index),
          "timeout_s": max(int(timeout), W.rendezvous_timeout()), "elastic": True, "collective_timeout_s": timeout,
          "store_port": None if store_port is None else int(store_port)}
    membership = 0
    if join is not None:
        # a re-spawned rank: prepare alone, say so, and wait to be named a member of the next world
        if store_port is None:
            raise SystemExit("NODEXA_MINER_JOIN_MEMBERSHIP needs NODEXA_MINER_STORE_PORT")
        info = join_world(int(join), my_id, int(store_port), cpu=cpu, device_index=kw["device_index"])
        if info is None:
            return 4
        members, membership = info
        kw.update(rank=members.index(my_id), world_size=len(members), membership=membership, ids=members,
                  timeout_s=int(max(5.0, timeout)))
    W.init(**kw)
    w = W.get()
    dev = make_rank_device(cpu, w.device.index if not cpu else None, collective_dag=w.collective, window=window,
                           fail_rate=injected_fail_rate(float(os.environ.get("NODEXA_MINER_FAILRATE", "0") or 0), my_id),
                           drop_rate=float(os.environ.get("NODEXA_MINER_DROPSHARE", "0") or 0), seed=my_id,
                           jit_mode=follower_jit_mode(), joined_late=join is not None)
    hang = int(os.environ.get("NODEXA_MINER_HANG_AFTER", "0"))
    if hang > 0:  # fault injection for the failure-handling tests
        from .search import HangingDevice

        dev = HangingDevice(dev, hang)
    wlog = os.environ.get("NODEXA_MINER_WINDOWS_LOG")
    if wlog:
        # "{id}" in the path: one environment serves a whole supervised world; every life of a rank
        # writes a log of its own
        wlog = wlog.replace("{id}", str(my_id)) + (f".life{life}" if life else "")
    svc = MiningService(dev, None, window=window, watchdog_s=watchdog, collective_timeout_s=timeout,
                        record_windows=bool(wlog), max_failures=int(os.environ.get("NODEXA_MINER_MAXFAILURES", "3")),
                        membership=membership)

    def dump():
        if wlog:
            kd = getattr(svc.dev, "kawpow", None)
            with open(wlog, "w") as f:
                json.dump({"rank": svc.rank, "world_size": svc.world_size, "windows": svc.windows,
                           "steps": svc.steps, "hashes_total": svc.hashes_total,
                           "failures": svc.total_failures, "id": my_id, "life": life, "reforms": svc.reforms,
                           "membership": svc.membership, "own_hashes": svc.own_hashes,
                           "first_window_at": svc.first_result_at,
                           "dag_build_mode": {str(k): v for k, v in getattr(kd, "dag_build_mode", {}).items()},
                           "dag_build_s": {str(k): v for k, v in getattr(kd, "dag_build_s", {}).items()}}, f)

    try:
        svc.run()
    except DeviceHung as e:
        log.log_printf(f"miner rank {W.get().rank}: {e}; exiting so the survivors re-partition")
        dump()
        os._exit(EXIT_DEVICE_HUNG)
    except DeviceEvicted as e:
        log.log_printf(f"miner rank {W.get().rank}: device evicted ({e}); exiting so the survivors re-partition")
        dump()
        os._exit(EXIT_DEVICE_FAILED)
    except RuntimeError as e:
        log.log_printf(f"miner rank {W.get().rank}: {e}")
        dump()
        return 3
    dump()
    W.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(follower_main())
