"""Stratum server in the node: any KawPow miner mines to this node without RPC credentials and
without polling (wire format: miner/stratum.py).

Threads:
* the I/O thread owns every socket (one selector): accept, read lines, the cheap `mining.submit`
  checks, and writing. Other threads only append to a connection's bounded send buffer and wake
  the selector; a connection whose buffer is full (a peer that does not read) is closed, so no slow
  or dead peer can hold up the verifier or the other connections;
* the job thread waits for the job source to change and pushes `mining.notify` to everybody; with
  vardiff it also sends the current job again (clean_jobs false) to a connection that got no job
  for `RESEND_S` and whose target is due to change;
* the verifier thread does the full hashes. It drains whatever submits are queued at that moment
  into one batch (no added wait: batching comes from submits that arrive while a batch runs). A
  job whose epoch DAG is resident on the node's device (ops/verify.is_resident) goes through
  ops/verify.gpu_full_hash, anything else through the host's light-mode `_core.kawpow_hash`. The
  verifier itself never builds a DAG and never waits for one;
* with `gpu_verify` (-stratumgpuverify=1) and a device, one more thread (miner/stratum_epochs.py)
  builds the DAG of the current job's epoch when none is resident (a node that serves rigs without
  mining itself, or whose miner has not shared the new epoch yet), and the next epoch's from 120
  blocks before the boundary. While it builds, the epoch's shares go through `gpu_full_hash` in
  light mode as soon as the light cache is on the device, and through the host before that.
  Without the flag the only resident DAGs are the ones the in-process miner built.

`mining.submit` is checked in this order, answering at the first failure: subscribed (25) and
authorized (24); job known, built on the current tip and, with vardiff, sent to this connection
(21); header hash equals the job's (20); nonce carries the connection's extranonce (20); (job,
nonce) not seen before (22); `kawpow_hash_no_verify(height, header, mix, nonce)` at or below the
share target (23: the cheap check, no DAG access); the recomputed mix equals the submitted one
(otherwise 20 and the connection is closed: an honest miner cannot produce that). A share whose job
went stale while it waited for its full hash is answered 21 then. A share whose final hash also
meets the block target becomes a block through the job source.

The share target is the easier of the block target and 2^(256-bits) - 1. Without vardiff, bits is
-stratumsharebits for everybody. With `vardiff` (-stratumvardiff=<shares per minute>) every
connection has bits of its own, starting at -stratumsharebits; the rule is miner/stratum.py's
`vardiff_next_bits`. It runs only when a job is about to go to the connection and `RETARGET_S` have
passed since its last retarget (or its authorize), so a new target always travels as
`mining.set_target` right in front of a `mining.notify`, and a share is judged against the target
that went out with its job to that connection (the last `JOBS_KEPT` jobs are remembered per
connection; where the same job went out twice, the easier target judges and the work credited is
that of the hardest target sent that the hash meets). Every accepted share is recorded with its
work, 2^256 / (target + 1), and a connection's hashrate is the work of its window over the window.

`ban_s` (-stratumbantime=<seconds>): an address whose connections were closed for a wrong mix
`BAN_STRIKES` times within `BAN_WINDOW_S` is refused at accept for that long (`BanTable`).

Jobs come from a `JobSource`: the current job, and wait for change. The node's `ChainJobSource`
builds one template per job with BlockAssembler (all connections work on the same header hash in
disjoint nonce ranges: each has a 2-byte extranonce, unique among the live connections), issues a
clean job as soon as the tip changes (the `updated_block_tip` signal, no poll) and a non-clean one
when the pool of transactions moved and the job is older than the miner's template refresh time.
`StaticJobSource` takes injected jobs (tests, tools).
"""
from __future__ import annotations

import collections
import queue
import selectors
import socket
import threading
import time
from dataclasses import dataclass, field

from .. import core
from ..utils import log
from . import stratum as S

_core = core()

EXTRANONCE_BYTES = 2
SEND_BUFFER_MAX = 64 * 1024   # bytes queued for one connection before it is closed as too slow
JOBS_KEPT = 8
HASHRATE_WINDOW_S = 600.0
RETARGET_S = 30.0      # vardiff: the least time between two retargets of a connection
RESEND_S = 60.0        # vardiff: a connection without a job for this long gets the current one again when a retarget is due
BAN_STRIKES = 3        # -stratumbantime: wrong mixes from one address ...
BAN_WINDOW_S = 600.0   # ... within this time
BAN_TABLE_MAX = 1024   # addresses remembered, the oldest dropped


def share_work(target: int) -> int:
    """The expected hashes behind one share at `target`."""
    return (1 << 256) // (target + 1)


class BanTable:
    """Addresses that sent wrong mixes. `strike(addr, now)` records one and returns True when it
    is the `BAN_STRIKES`-th within `BAN_WINDOW_S`: the address is then banned for `ban_s`. One
    table, bounded at `BAN_TABLE_MAX` addresses (strikes and bans together), oldest dropped."""

    def __init__(self, ban_s: float):
        self.ban_s = float(ban_s)
        self.entries: collections.OrderedDict[str, list] = collections.OrderedDict()  # addr -> [strike times, banned until]
        self.lock = threading.Lock()

    def strike(self, addr: str, now: float) -> bool:
        with self.lock:
            ent = self.entries.pop(addr, None) or [[], 0.0]
            ent[0] = [t for t in ent[0] if now - t < BAN_WINDOW_S] + [now]
            banned = len(ent[0]) >= BAN_STRIKES
            if banned:
                ent[:] = [[], now + self.ban_s]
            self.entries[addr] = ent  # most recent last
            while len(self.entries) > BAN_TABLE_MAX:
                self.entries.popitem(last=False)
            return banned

    def banned_until(self, addr: str, now: float) -> float:
        """When the address's ban ends, or 0.0 when it has none."""
        with self.lock:
            ent = self.entries.get(addr)
            if ent is None or ent[1] <= now:
                if ent is not None and not ent[0] and ent[1]:
                    del self.entries[addr]  # an expired ban with no strike since
                return 0.0
            return ent[1]

    def __len__(self) -> int:
        return len(self.entries)


@dataclass
class ServerJob:
    job_id: str
    header_hash: bytes      # ProgPoW order
    height: int
    block_target: int
    bits: int = 0
    clean: bool = True
    tip: object = None      # what the job was built on: stale once the source's tip differs
    block: object = None    # the source's own payload (the template block)
    created: float = field(default_factory=time.time)
    seen: set = field(default_factory=set)  # nonces submitted for this job

    @property
    def seed_hash(self) -> bytes:
        return _core.epoch_seed(self.height // _core.EPOCH_LENGTH)


class JobSource:
    """Where the server's jobs come from: the current job, and wait for change."""

    algo = "kawpow"

    def current(self) -> ServerJob | None:
        raise NotImplementedError

    def wait_change(self, seq: int, timeout: float) -> int:
        """Block until the source's sequence number differs from `seq` (or `timeout`); returns it."""
        raise NotImplementedError

    def get(self, job_id: str) -> ServerJob | None:
        raise NotImplementedError

    def is_current_tip(self, job: ServerJob) -> bool:
        raise NotImplementedError

    def submit_block(self, job: ServerJob, nonce: int, mix_hash: bytes) -> tuple[bool, str]:
        raise NotImplementedError

    def close(self) -> None:
        pass


class StaticJobSource(JobSource):
    """Jobs pushed in by the caller. `on_block(job, nonce, mix)` is the block callback."""

    def __init__(self, on_block=None):
        self.cv = threading.Condition()
        self.seq = 0
        self.jobs: collections.OrderedDict[str, ServerJob] = collections.OrderedDict()
        self.tip = None
        self.on_block = on_block
        self.blocks: list[tuple[str, int, bytes]] = []

    def push(self, job: ServerJob) -> None:
        with self.cv:
            self.jobs[job.job_id] = job
            while len(self.jobs) > JOBS_KEPT:
                self.jobs.popitem(last=False)
            self.tip = job.tip
            self.seq += 1
            self.cv.notify_all()

    def current(self):
        with self.cv:
            return next(reversed(self.jobs.values())) if self.jobs else None

    def wait_change(self, seq, timeout):
        with self.cv:
            if self.seq == seq:
                self.cv.wait(timeout)
            return self.seq

    def get(self, job_id):
        with self.cv:
            return self.jobs.get(job_id)

    def is_current_tip(self, job):
        return job.tip == self.tip

    def submit_block(self, job, nonce, mix_hash):
        self.blocks.append((job.job_id, nonce, mix_hash))
        if self.on_block is not None:
            self.on_block(job, nonce, mix_hash)
        return True, "accepted"


class ChainJobSource(JobSource):
    """The node's jobs: BlockAssembler templates with the source's own ExtraNonce, a clean job on
    every tip change (signalled, never polled), a refresh when the transaction pool moved."""

    def __init__(self, state, script: bytes, refresh_s: float = 10.0):
        from ..chain.state import ValidationInterface
        from .assembler import ExtraNonce

        self.state = state
        self.script = script
        self.refresh_s = float(refresh_s)
        self.extranonce = ExtraNonce()
        self.cv = threading.Condition()
        self.seq = 0
        self.jobs: collections.OrderedDict[str, ServerJob] = collections.OrderedDict()
        self.job_n = 0
        self.tx_updated = -1
        self.algo = "kawpow"
        self.not_kawpow_logged = False
        self._tip_moved = threading.Event()
        self._stop = threading.Event()
        self._last_build = 0.0
        src = self

        class _Tip(ValidationInterface):
            def updated_block_tip(self, tip, fork, initial_download: bool) -> None:
                src._tip_moved.set()  # called under the chain lock: only a flag, the job thread builds

        self._listener = _Tip()
        state.register(self._listener)
        self._tip_moved.set()
        self._thread = threading.Thread(target=self._run, name="stratum-jobs", daemon=True)
        self._thread.start()

    def _run(self) -> None:
        while not self._stop.is_set():
            moved = self._tip_moved.wait(1.0)
            if self._stop.is_set():
                break
            self._tip_moved.clear()
            try:
                cur = self.current()
                # without a job (a template that failed, or a chain outside the KawPow era, which
                # begins by header time and so without any tip change) the template is tried again:
                # every tick after a failure, every refresh time outside the era
                retry = cur is None and time.time() - self._last_build >= (1.0 if self.algo == "kawpow" else self.refresh_s)
                if moved or retry:
                    self._last_build = time.time()
                    self._new_job(clean=True)
                elif cur is not None and self.state.transactions_updated != self.tx_updated \
                        and time.time() - cur.created > self.refresh_s:
                    self._new_job(clean=False)
            except Exception as e:  # noqa: BLE001 — a template that cannot be built now: the next signal retries
                log.log_printf(f"stratum: building a job failed: {type(e).__name__}: {e}")

    def _new_job(self, clean: bool) -> None:
        from ..chain.header import to_progpow
        from .assembler import BlockAssembler
        from .search import ALGO_KAWPOW, ALGO_NAMES
        from .service import algo_for_time

        st = self.state
        tx_updated = st.transactions_updated
        tpl = BlockAssembler(st).create_new_block(self.script)
        blk = tpl.block
        self.extranonce.increment(blk, tpl.height)
        hdr = blk.header
        algo = algo_for_time(st.params, hdr.time)
        with self.cv:
            self.algo = ALGO_NAMES[algo]
            self.tx_updated = tx_updated
            if algo != ALGO_KAWPOW:
                # not a KawPow block next: connections stay open, no job goes out
                if not self.not_kawpow_logged:
                    self.not_kawpow_logged = True
                    log.log_printf(f"stratum: the next block (height {tpl.height}) is a {self.algo} block, not KawPow; "
                                   "no job is served until the chain is in the KawPow era")
                if self.jobs:
                    self.jobs.clear()
                    self.seq += 1
                    self.cv.notify_all()
                return
            self.job_n += 1
            job = ServerJob("%x" % self.job_n, to_progpow(hdr.kawpow_header_hash()), tpl.height, int(tpl.target),
                            int(hdr.bits), clean, hdr.prev, blk)
            self.jobs[job.job_id] = job
            while len(self.jobs) > JOBS_KEPT:
                self.jobs.popitem(last=False)
            self.seq += 1
            self.cv.notify_all()

    def current(self):
        with self.cv:
            return next(reversed(self.jobs.values())) if self.jobs else None

    def wait_change(self, seq, timeout):
        with self.cv:
            if self.seq == seq:
                self.cv.wait(timeout)
            return self.seq

    def get(self, job_id):
        with self.cv:
            return self.jobs.get(job_id)

    def is_current_tip(self, job):
        return job.tip == self.state.tip().hash

    def submit_block(self, job, nonce, mix_hash):
        from ..ops.kawpow import Share
        from .search import ALGO_KAWPOW
        from .service import solved_block

        st = self.state
        blk = solved_block(st.params, job.block, ALGO_KAWPOW, Share(nonce, mix_hash, b""))
        res = st.process_new_block(blk)
        if not res.ok:
            return False, str(res.reject)
        st._emit("block_found", st.block_hash(blk.header))
        return True, _core.u256_hex(st.block_hash(blk.header))

    def close(self) -> None:
        self._stop.set()
        self._tip_moved.set()
        self._thread.join(10.0)
        self.state.unregister(self._listener)


class _Conn:
    def __init__(self, cid: int, sock, addr, extranonce: bytes, now: float | None = None, bits: int = 0):
        self.id = cid
        self.sock = sock
        self.addr = addr
        self.extranonce = extranonce
        self.buf = S.LineBuffer()
        self.out = bytearray()
        self.out_lock = threading.Lock()
        self.closed = False
        self.close_after_flush = False
        self.subscribed = False
        self.authorized = False
        self.agent = ""
        self.user = ""
        self.connected = time.time() if now is None else now
        self.accepted = 0
        self.rejected: dict[int, int] = {}
        self.last_share = 0.0
        self.accept_times: collections.deque = collections.deque()
        self.target_sent: int | None = None
        self.job_sent: ServerJob | None = None
        self.job_sent_at = 0.0
        # vardiff (unused without it): the connection's share bits, the shares accepted and the time since
        # its last retarget, and the targets that went out to it with each of its last JOBS_KEPT jobs
        self.bits = bits
        self.retargets = 0
        self.retarget_at = self.connected
        self.shares_since = 0
        self.job_targets: collections.OrderedDict[str, list[int]] = collections.OrderedDict()

    def info(self, now: float) -> dict:
        """`accept_times` holds (time, work of that share's target): the hashrate is the window's work."""
        while self.accept_times and now - self.accept_times[0][0] > HASHRATE_WINDOW_S:
            self.accept_times.popleft()
        span = max(1e-3, min(now - self.connected, HASHRATE_WINDOW_S))
        return {"id": self.id, "address": f"{self.addr[0]}:{self.addr[1]}", "agent": self.agent, "user": self.user,
                "extranonce": self.extranonce.hex(), "connected": round(now - self.connected, 3),
                "accepted": self.accepted, "rejected": {str(k): v for k, v in sorted(self.rejected.items())},
                "last_share": int(self.last_share),
                "hashrate": round(sum(w for _t, w in self.accept_times) / span, 3),
                "share_bits": self.bits, "retargets": self.retargets,
                "shares_per_minute": round(len(self.accept_times) * 60.0 / span, 3)}


class StratumServer:
    def __init__(self, source: JobSource, *, host: str = "127.0.0.1", port: int = 0, share_bits: int = 0,
                 password: str | None = None, max_connections: int = 64, device: int | None = None,
                 vardiff: int = 0, gpu_verify: bool = False, ban_s: float = 0.0, dag_check: bool = True,
                 epoch_owner=None, clock=time.time):
        """`vardiff`: wanted shares per minute and connection (0: one target for everybody).
        `gpu_verify`: keep DAGs for share checks on `device` (an `EpochOwner`; `epoch_owner` injects
        one). `ban_s`: seconds an address is refused after `BAN_STRIKES` wrong mixes (0: never).
        `clock`: the time source of everything the server times (tests inject one)."""
        self.source = source
        self.host, self.port = host, int(port)
        self.share_bits = int(share_bits)
        self.vardiff = max(0, int(vardiff))
        if self.vardiff and not 0 < self.share_bits <= S.VARDIFF_MAX_BITS:
            raise ValueError("vardiff needs share bits above 0: they are where every connection starts "
                             "and the easiest target it can get")
        self.clock = clock
        self.bans = BanTable(ban_s) if ban_s and ban_s > 0 else None
        self.share_target = S.share_target_for_bits(share_bits) if share_bits else 0  # 0: the block target
        self.password = password or None
        # every live connection needs a 2-byte extranonce of its own: below 2^16, so _accept always finds a free one
        self.max_connections = max(0, min(int(max_connections), (1 << 8 * EXTRANONCE_BYTES) - 1))
        self.device = device
        self.epochs = epoch_owner
        if self.epochs is None and gpu_verify and device is not None:
            from .stratum_epochs import EpochOwner, device_builder

            self.epochs = EpochOwner(device, device_builder(device, dag_check))
        self.conns: dict[int, _Conn] = {}
        self.lock = threading.Lock()       # conns, extranonces, counters
        self.stats = {"verify_batches_gpu": 0, "verify_batches_host": 0, "verified_gpu": 0, "verified_host": 0,
                      "accepted": 0, "rejected": 0, "refused_connections": 0, "jobs_sent": 0, "slow_closed": 0,
                      "blocks_rejected": 0}
        if self.epochs is not None:
            self.stats["verified_gpu_light"] = 0
        self.blocks_found = 0
        self.recent: collections.deque = collections.deque(maxlen=8)  # the last closed connections, as they ended
        self.verify_q: queue.Queue = queue.Queue()
        self._next_id = 1
        self._next_extranonce = 1
        self._stop = threading.Event()
        self._sel = selectors.DefaultSelector()
        self._wake_r, self._wake_w = socket.socketpair()
        self._wake_r.setblocking(False)
        self._wake_w.setblocking(False)
        self._listen: socket.socket | None = None
        self._threads: list[threading.Thread] = []

    # ------------------------------------------------------------------ lifecycle
    def start(self) -> "StratumServer":
        ls = socket.socket(socket.AF_INET6 if ":" in self.host else socket.AF_INET, socket.SOCK_STREAM)
        ls.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        ls.bind((self.host, self.port))
        ls.listen(64)
        ls.setblocking(False)
        self._listen = ls
        self.port = ls.getsockname()[1]
        self._sel.register(ls, selectors.EVENT_READ, "listen")
        self._sel.register(self._wake_r, selectors.EVENT_READ, "wake")
        for name, fn in (("stratum-io", self._io_loop), ("stratum-notify", self._job_loop),
                         ("stratum-verify", self._verify_loop)):
            t = threading.Thread(target=fn, name=name, daemon=True)
            t.start()
            self._threads.append(t)
        log.log_printf(f"Stratum listening on {self.host}:{self.port}")
        return self

    def stop(self, timeout: float = 10.0) -> None:
        if self._stop.is_set():
            return
        self._stop.set()
        self.verify_q.put(None)
        self._wake()
        for t in self._threads:
            t.join(timeout)
        self._threads = []
        if self.epochs is not None:
            self.epochs.stop()
        for c in list(self.conns.values()):
            self._close(c)
        if self._listen is not None:
            try:
                self._sel.unregister(self._listen)
            except (KeyError, ValueError):
                pass
            self._listen.close()
            self._listen = None
        self._sel.close()
        self._wake_r.close()
        self._wake_w.close()

    def _count(self, key: str, n: int = 1) -> None:
        with self.lock:
            self.stats[key] += n

    def _wake(self) -> None:
        try:
            self._wake_w.send(b"\0")
        except (BlockingIOError, OSError):
            pass

    # ------------------------------------------------------------------ sending (any thread)
    def _send(self, c: _Conn, data: bytes, then_close: bool = False) -> None:
        with c.out_lock:
            if c.closed:
                return
            if len(c.out) + len(data) > SEND_BUFFER_MAX:
                c.close_after_flush = True
                c.out.clear()  # a peer that does not read: nothing more for it, the I/O thread closes it
                self._count("slow_closed", 1)
            else:
                c.out += data
                c.close_after_flush |= then_close
        self._wake()

    def effective_target(self, job: ServerJob) -> int:
        """The easier of the share target and the block target."""
        return max(self.share_target, job.block_target)

    def _next_bits(self, c: _Conn, now: float) -> int | None:
        """The connection's bits after a retarget now, or None when none is due yet."""
        if now - c.retarget_at < RETARGET_S:
            return None
        return S.vardiff_next_bits(c.bits, c.shares_since, int((now - c.retarget_at) * 1000), self.vardiff,
                                   self.share_bits)

    def _vardiff_target(self, c: _Conn, job: ServerJob, now: float) -> int:
        """Vardiff's part of `_send_job`: retarget if due, and remember the target with the job."""
        with self.lock:
            bits = self._next_bits(c, now)
            if bits is not None:
                c.retarget_at, c.shares_since = now, 0
                if bits != c.bits:
                    c.bits = bits
                    c.retargets += 1
            target = max(S.share_target_for_bits(c.bits), job.block_target)
            sent = c.job_targets.pop(job.job_id, [])
            c.job_targets[job.job_id] = sent if target in sent else sent + [target]
            while len(c.job_targets) > JOBS_KEPT:
                c.job_targets.popitem(last=False)
        return target

    def _send_job(self, c: _Conn, job: ServerJob, clean: bool | None = None) -> None:
        if self.vardiff:
            c.job_sent_at = now = self.clock()
            target = self._vardiff_target(c, job, now)
        else:
            target = self.effective_target(job)
        wire = S.Job(job.job_id, job.header_hash, job.seed_hash, target, job.clean if clean is None else clean,
                     job.height, job.bits)
        data = b""
        c.job_sent = job
        if c.target_sent != target:
            c.target_sent = target
            data = S.set_target(target)
        self._send(c, data + S.notify(wire))
        self._count("jobs_sent", 1)

    # ------------------------------------------------------------------ the job thread
    def _job_loop(self) -> None:
        seq = -1
        last = None
        while not self._stop.is_set():
            seq = self.source.wait_change(seq, 0.5)
            job = self.source.current()
            if job is not None and job is last and self.vardiff:
                self._resend_due(job)
            if job is None or job is last:
                last = job
                continue
            last = job
            if self.epochs is not None:
                self.epochs.note_job(job.height)
            with self.lock:
                conns = [c for c in self.conns.values() if c.subscribed and c.authorized]
            for c in conns:
                if c.job_sent is not job:  # it authorized after the change and got this job then
                    self._send_job(c, job)

    def _resend_due(self, job: ServerJob) -> None:
        """A connection that got no job for RESEND_S and whose bits a retarget would change now gets
        the current job again, not clean: the only way a target reaches a connection is with a job."""
        now = self.clock()
        with self.lock:
            due = [c for c in self.conns.values() if c.subscribed and c.authorized and c.job_sent is not None
                   and now - c.job_sent_at >= RESEND_S and self._next_bits(c, now) not in (None, c.bits)]
        for c in due:
            self._send_job(c, job, clean=False)

    # ------------------------------------------------------------------ the I/O thread
    def _io_loop(self) -> None:
        while not self._stop.is_set():
            for key, ev in self._sel.select(0.5):
                if key.data == "wake":
                    try:
                        self._wake_r.recv(4096)
                    except (BlockingIOError, OSError):
                        pass
                elif key.data == "listen":
                    self._accept()
                else:
                    c = key.data
                    if ev & selectors.EVENT_READ:
                        self._read(c)
                    if ev & selectors.EVENT_WRITE and not c.closed:
                        self._flush(c)
            for c in list(self.conns.values()):  # what other threads queued
                if c.out or c.close_after_flush:
                    self._flush(c)

    def _accept(self) -> None:
        try:
            sock, addr = self._listen.accept()
        except OSError:
            return
        with self.lock:
            if len(self.conns) >= self.max_connections:
                self.stats["refused_connections"] += 1
                sock.close()
                return
            until = self.bans.banned_until(addr[0], self.clock()) if self.bans is not None else 0.0
            if until:
                self.stats["refused_connections"] += 1
                self.recent.append({"address": f"{addr[0]}:{addr[1]}", "refused": "banned for wrong mixes",
                                    "banned_until": int(until), "closed": int(self.clock())})
                sock.close()
                return
            used = {c.extranonce for c in self.conns.values()}
            while True:  # unique among the live connections
                x = (self._next_extranonce & 0xFFFF).to_bytes(EXTRANONCE_BYTES, "big")
                self._next_extranonce += 1
                if x not in used:
                    break
            c = _Conn(self._next_id, sock, addr, x, self.clock(), self.share_bits)
            self._next_id += 1
            self.conns[c.id] = c
        sock.setblocking(False)
        try:
            sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
        except OSError:
            pass
        self._sel.register(sock, selectors.EVENT_READ, c)

    def _close(self, c: _Conn) -> None:
        with c.out_lock:
            if c.closed:
                return
            c.closed = True
        with self.lock:
            self.conns.pop(c.id, None)
            if c.subscribed:
                self.recent.append(dict(c.info(self.clock()), closed=int(self.clock())))
        try:
            self._sel.unregister(c.sock)
        except (KeyError, ValueError, OSError):
            pass
        try:
            c.sock.close()
        except OSError:
            pass

    def _flush(self, c: _Conn) -> None:
        with c.out_lock:
            if c.closed:
                return
            try:
                while c.out:
                    n = c.sock.send(c.out)
                    del c.out[:n]
            except (BlockingIOError, InterruptedError):
                pass
            except OSError:
                c.out.clear()
                c.close_after_flush = True
            pending, close = bool(c.out), c.close_after_flush and not c.out
        if close:
            self._close(c)
            return
        try:
            self._sel.modify(c.sock, selectors.EVENT_READ | (selectors.EVENT_WRITE if pending else 0), c)
        except (KeyError, ValueError, OSError):
            pass

    def _read(self, c: _Conn) -> None:
        try:
            data = c.sock.recv(65536)
        except (BlockingIOError, InterruptedError):
            return
        except OSError:
            data = b""
        if not data:
            self._close(c)
            return
        try:
            for line in c.buf.feed(data):
                self._on_message(c, S.decode(line))
                if c.closed or c.close_after_flush:
                    break
        except S.StratumError as e:
            if e.fatal:  # over-long line, or not a JSON object
                self._close(c)

    def _reject(self, c: _Conn, msg_id, code: int, message: str | None = None, close: bool = False) -> None:
        with self.lock:
            c.rejected[code] = c.rejected.get(code, 0) + 1
            self.stats["rejected"] += 1
        self._send(c, S.error_response(msg_id, code, message), then_close=close)

    def _on_message(self, c: _Conn, m: S.Message) -> None:
        if m.is_response:
            return
        try:
            if m.method == "mining.subscribe":
                c.subscribed = True
                c.agent = str(m.params[0])[:64] if m.params else ""
                self._send(c, S.response(m.id, S.subscribe_result(None, c.extranonce)))
            elif m.method == "mining.authorize":
                if not c.subscribed:
                    self._send(c, S.error_response(m.id, S.ERR_NOT_SUBSCRIBED))
                    return
                user = m.params[0] if len(m.params) > 0 else ""
                pw = m.params[1] if len(m.params) > 1 else ""
                if not isinstance(user, str) or (self.password is not None and pw != self.password):
                    self._send(c, S.error_response(m.id, S.ERR_UNAUTHORIZED))
                    return
                c.authorized, c.user = True, user[:64]
                c.retarget_at = self.clock()
                self._send(c, S.response(m.id, True))
                job = self.source.current()
                if job is not None:
                    self._send_job(c, job, clean=True)
            elif m.method == "mining.submit":
                self._on_submit(c, m)
            else:
                self._send(c, S.error_response(m.id, S.ERR_OTHER, f"unknown method {m.method[:40]}"))
        except S.StratumError as e:
            if e.fatal:
                raise
            self._reject(c, m.id, e.code, str(e))

    def _on_submit(self, c: _Conn, m: S.Message) -> None:
        if not c.subscribed:
            return self._reject(c, m.id, S.ERR_NOT_SUBSCRIBED)
        if not c.authorized:
            return self._reject(c, m.id, S.ERR_UNAUTHORIZED)
        sub = S.Submit.from_params(m.params)  # StratumError -> 20
        job = self.source.get(sub.job_id)
        if job is None or not self.source.is_current_tip(job):
            return self._reject(c, m.id, S.ERR_STALE)
        sent = None
        if self.vardiff:
            with self.lock:
                sent = list(c.job_targets.get(sub.job_id, ()))
            if not sent:  # a job this connection was never sent (or one it got too long ago)
                return self._reject(c, m.id, S.ERR_STALE)
        if sub.header_hash != job.header_hash:
            return self._reject(c, m.id, S.ERR_OTHER, "wrong header hash for the job")
        if not S.nonce_in_extranonce(sub.nonce, c.extranonce):
            return self._reject(c, m.id, S.ERR_OTHER, "nonce outside the extranonce")
        if sub.nonce in job.seen:
            return self._reject(c, m.id, S.ERR_DUPLICATE)
        fin = _core.kawpow_hash_no_verify(job.height, job.header_hash, sub.mix_hash, sub.nonce)
        value = int.from_bytes(fin, "big")
        # the hardest target that went out with this job to this connection and that the hash meets
        met = [t for t in (sent or (self.effective_target(job),)) if value <= t]
        if not met:
            return self._reject(c, m.id, S.ERR_HIGH_HASH)
        job.seen.add(sub.nonce)
        self.verify_q.put((c, m.id, job, sub, fin, share_work(min(met))))

    # ------------------------------------------------------------------ the verifier thread
    def _resident(self, epoch: int) -> bool:
        if self.device is None:
            return False
        from ..ops import verify as V

        return V.is_resident(self.device, epoch)

    def _verify_loop(self) -> None:
        while True:
            item = self.verify_q.get()
            if item is None or self._stop.is_set():
                return
            batch = [item]
            while True:  # whatever is queued right now; no wait for more
                try:
                    nxt = self.verify_q.get_nowait()
                except queue.Empty:
                    break
                if nxt is None:
                    return
                batch.append(nxt)
            try:
                self._verify_batch(batch)
            except Exception as e:  # noqa: BLE001 — the submits of a failed batch are answered, not left waiting
                log.log_printf(f"stratum: share verification failed: {type(e).__name__}: {e}")
                for c, msg_id, *_ in batch:
                    self._reject(c, msg_id, S.ERR_OTHER, "verification failed")

    def _verify_batch(self, batch: list) -> None:
        resident = {e: self._resident(e) for e in {b[2].height // _core.EPOCH_LENGTH for b in batch}}
        gpu = [b for b in batch if resident[b[2].height // _core.EPOCH_LENGTH]]
        host = [b for b in batch if not resident[b[2].height // _core.EPOCH_LENGTH]]
        results: dict[int, tuple[bytes, bytes]] = {}
        if host and self.epochs is not None:
            # an epoch whose DAG is still being built: the light-mode kernel, once its light cache is on the device
            lit = {e for e, r in resident.items() if not r and self.epochs.mode(e) == "light"}
            light = [b for b in host if b[2].height // _core.EPOCH_LENGTH in lit]
            if light:
                from ..ops import verify as V

                host = [b for b in host if b[2].height // _core.EPOCH_LENGTH not in lit]
                out = V.gpu_full_hash([b[2].height for b in light], [b[2].header_hash for b in light],
                                      [b[3].nonce for b in light], device=self.device, mode="light")
                for b, r in zip(light, out):
                    results[id(b)] = r
                self._count("verified_gpu_light", len(light))
        if gpu:
            from ..ops import verify as V

            out = V.gpu_full_hash([b[2].height for b in gpu], [b[2].header_hash for b in gpu],
                                  [b[3].nonce for b in gpu], device=self.device, mode="auto")
            for b, r in zip(gpu, out):
                results[id(b)] = r
            self._count("verify_batches_gpu", 1)
            self._count("verified_gpu", len(gpu))
        if host:
            for b in host:
                ctx = _core.get_epoch_context(b[2].height // _core.EPOCH_LENGTH)
                results[id(b)] = _core.kawpow_hash(ctx, b[2].height, b[2].header_hash, b[3].nonce)
            self._count("verify_batches_host", 1)
            self._count("verified_host", len(host))
        now = self.clock()
        for b in batch:
            c, msg_id, job, sub, fin, work = b
            full_fin, full_mix = results[id(b)]
            if bytes(full_mix) != sub.mix_hash or bytes(full_fin) != fin:
                log.log_printf(f"stratum: connection {c.id} ({c.addr[0]}) sent a wrong mix for nonce {sub.nonce:016x}; closed")
                # counted before the peer can see the close: its next connection already meets the ban
                banned = self.bans is not None and self.bans.strike(c.addr[0], now)
                self._reject(c, msg_id, S.ERR_OTHER, "wrong mix", close=True)
                if banned:
                    log.log_printf(f"stratum: {c.addr[0]} sent {BAN_STRIKES} wrong mixes within {int(BAN_WINDOW_S)} s; "
                                   f"refused for {int(self.bans.ban_s)} s")
                continue
            if not self.source.is_current_tip(job):  # the tip moved while the share waited for its hash
                self._reject(c, msg_id, S.ERR_STALE)
                continue
            with self.lock:
                c.accepted += 1
                c.last_share = now
                c.accept_times.append((now, work))
                c.shares_since += 1
                self.stats["accepted"] += 1
            if int.from_bytes(fin, "big") <= job.block_target and self.source.is_current_tip(job):
                try:
                    ok, info = self.source.submit_block(job, sub.nonce, sub.mix_hash)
                except Exception as e:  # noqa: BLE001
                    ok, info = False, f"{type(e).__name__}: {e}"
                if ok:
                    self.blocks_found += 1
                else:
                    self._count("blocks_rejected", 1)
                log.log_printf(f"stratum: share of connection {c.id} (job {job.job_id}, nonce {sub.nonce:016x}) meets "
                               f"the block target: {'block ' + info if ok else 'rejected: ' + info}")
            self._send(c, S.response(msg_id, True))

    # ------------------------------------------------------------------ getstratuminfo
    def info(self) -> dict:
        job = self.source.current()
        now = self.clock()
        algo = getattr(self.source, "algo", "kawpow")
        target = self.effective_target(job) if job is not None else self.share_target
        with self.lock:
            conns = [c.info(now) for c in self.conns.values()]
            recent = list(self.recent)
            stats = dict(self.stats)
        stats["vardiff"] = self.vardiff
        if self.epochs is not None:
            stats.update(self.epochs.info())
        out = {"enabled": True, "port": self.port, "serving": job is not None, "algo": algo,
               "height": job.height if job is not None else None,
               "job": {"id": job.job_id, "header_hash": job.header_hash.hex(), "age": round(now - job.created, 3)}
               if job is not None else None,
               "share_target": S.target_hex(target) if target else None,
               "blocks_found": self.blocks_found, **stats, "connections": conns, "recent_connections": recent}
        if job is None and algo != "kawpow":
            out["note"] = f"the next block is a {algo} block, not KawPow: connections stay open, no job is served"
        return out
