"""Stratum pool client: this engine mining on a KawPow pool (wire format: miner/stratum.py).

Two threads meet in memory only. The connection thread (`StratumConnection`) owns the socket:
connect, `mining.subscribe`, `mining.authorize`, then it reads notifications and sends the shares
the loop queued; it reconnects with capped exponential back-off, trying the `-stratum=host:port`
entries in order. The mining loop's thread (miner/service.MiningService with a `StratumLeader`)
never touches the socket: `next_work` reads the newest job from memory (idle while disconnected or
before the first job) and `on_results` puts every share of a live job, after a full host re-hash,
on a queue. So a pool that stalls cannot stall the device, and a `mining.notify` with `clean_jobs`
reaches the device-side stale-work abort on the loop's next step without any poll.

Nonce ranges: the pool's extranonce bytes are the top bytes of every nonce; the free low bits are
split over the ranks of the mining loop by `rank_shift` (miner/search.Work).
"""
from __future__ import annotations

import queue
import selectors
import socket
import threading
import time

from .. import core
from ..utils import log
from . import stratum as S

_core = core()

AGENT = "nodexa-miner/1.0"


def parse_endpoint(s: str) -> tuple[str, int]:
    s = s.split("://", 1)[-1]
    host, _, port = s.rpartition(":")
    if not host or not port.isdigit():
        raise ValueError(f"-stratum={s}: expected host:port")
    return host, int(port)


def new_stats() -> dict:
    return {"windows": 0, "hashes": 0, "jobs": 0, "submitted": 0, "accepted": 0, "rejected": 0, "rejected_stale": 0, "lost": 0,
            "bad_shares": 0, "above_target": 0, "stale_shares": 0, "shares_dropped": 0, "refused_jobs": 0, "exhausted": 0,
            "connects": 0, "disconnects": 0}


class StratumConnection:
    """The connection thread and what it shares with the loop: the session (a number that changes
    with every connection), its extranonce, the newest job and the share queue."""

    def __init__(self, endpoints, user: str = "", password: str = "x", *, agent: str = AGENT, timeout: float = 30.0,
                 backoff: tuple[float, float] = (0.5, 30.0), stats: dict | None = None):
        self.endpoints = [parse_endpoint(e) if isinstance(e, str) else (e[0], int(e[1])) for e in endpoints]
        if not self.endpoints:
            raise ValueError("no stratum endpoint")
        self.user, self.password, self.agent = user, password, agent
        self.timeout = float(timeout)
        self.backoff = backoff
        self.stats = stats if stats is not None else new_stats()
        self.lock = threading.Lock()
        self.stats_lock = threading.Lock()
        self.session = 0             # 0: not connected (subscribed and authorized) now
        self.sessions = 0
        self.extranonce = b""
        self.job: S.Job | None = None
        self.job_seq = 0             # +1 per accepted mining.notify
        self.live_seq = 0            # shares of jobs older than this are stale (a clean job arrived)
        self.target: int | None = None
        self.shares: queue.Queue = queue.Queue()
        self.sent: list[S.Submit] = []  # what went out (tests, the last few hundred)
        self._pending: dict[int, tuple[float, S.Submit]] = {}
        self._next_id = 1
        self._refused_seeds: set[bytes] = set()
        self._stop = threading.Event()
        self._wake_r, self._wake_w = socket.socketpair()
        self._wake_r.setblocking(False)
        self._wake_w.setblocking(False)
        self._thread: threading.Thread | None = None
        self.peer: tuple[str, int] | None = None

    # ------------------------------------------------------------------ the loop thread's side
    def count(self, key: str, n: int = 1) -> None:
        """Add to a counter: the loop's thread and the connection's both count (stale_shares)."""
        with self.stats_lock:
            self.stats[key] += n

    def snapshot(self):
        """(session, extranonce, job, job_seq, live_seq) — memory only."""
        with self.lock:
            return self.session, self.extranonce, self.job, self.job_seq, self.live_seq

    def queue_share(self, session: int, seq: int, sub: S.Submit) -> None:
        self.shares.put((session, seq, sub))
        try:
            self._wake_w.send(b"\0")
        except (BlockingIOError, OSError):
            pass  # the wake pipe is full: the thread is about to look anyway

    # ------------------------------------------------------------------ lifecycle
    def start(self) -> "StratumConnection":
        self._thread = threading.Thread(target=self._run, name="stratum-client", daemon=True)
        self._thread.start()
        return self

    def stop(self, timeout: float = 5.0) -> None:
        self._stop.set()
        try:
            self._wake_w.send(b"\0")
        except (BlockingIOError, OSError):
            pass
        if self._thread is not None:
            self._thread.join(timeout)
            self._thread = None

    # ------------------------------------------------------------------ the connection thread
    def _run(self) -> None:
        delay = self.backoff[0]
        k = 0
        while not self._stop.is_set():
            host, port = self.endpoints[k % len(self.endpoints)]
            k += 1
            t0 = time.monotonic()
            try:
                self._session(host, port)
            except (OSError, S.StratumError) as e:
                log.log_printf(f"stratum: {host}:{port}: {e}")
            with self.lock:
                was, self.session, self.job = self.session, 0, None
            if was:
                self.count("disconnects", 1)
            if not self._stop.is_set():  # answers that cannot arrive any more
                self.count("lost", len(self._pending))
            self._pending.clear()
            if self._stop.is_set():
                break
            if was and time.monotonic() - t0 > self.backoff[1]:
                delay = self.backoff[0]  # a session that lasted: start the back-off over
            self._stop.wait(delay)
            delay = min(self.backoff[1], delay * 2)

    def _call(self, sock, buf: S.LineBuffer, line_for, what: str) -> S.Message:
        """Send one request and read until its response (matched by id); notifications that come
        in between are handled."""
        msg_id = self._next_id
        self._next_id += 1
        sock.sendall(line_for(msg_id))
        deadline = time.monotonic() + self.timeout
        while True:
            left = deadline - time.monotonic()
            if left <= 0:
                raise OSError(f"{what}: no response in {self.timeout:.0f}s")
            sock.settimeout(left)
            data = sock.recv(65536)
            if not data:
                raise OSError(f"{what}: connection closed")
            got = None
            for line in buf.feed(data):  # every line of this read: a job may follow the response at once
                m = S.decode(line)
                if m.is_response and m.id == msg_id:
                    got = m
                else:
                    self._handle(m)
            if got is not None:
                return got

    def _session(self, host: str, port: int) -> None:
        sock = socket.create_connection((host, port), timeout=self.timeout)
        sel = selectors.DefaultSelector()
        try:
            sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            buf = S.LineBuffer()
            self.target = None
            m = self._call(sock, buf, lambda i: S.subscribe(i, self.agent), "mining.subscribe")
            if m.error:
                raise OSError(f"mining.subscribe refused: {m.error}")
            _sid, extranonce = S.parse_subscribe_result(m.result)
            with self.lock:
                self.extranonce = extranonce
            m = self._call(sock, buf, lambda i: S.authorize(i, self.user, self.password), "mining.authorize")
            if m.error or m.result is not True:
                raise OSError(f"mining.authorize refused: {m.error}")
            while not self.shares.empty():  # found under an earlier extranonce: never sent under this one
                try:
                    self.shares.get_nowait()
                    self.count("stale_shares", 1)
                except queue.Empty:
                    break
            with self.lock:
                self.sessions += 1
                self.session = self.sessions
            self.count("connects", 1)
            self.peer = (host, port)
            log.log_printf(f"stratum: connected to {host}:{port}, extranonce {extranonce.hex() or '(none)'}")
            sock.settimeout(self.timeout)  # sends block at most this long; the loop never waits for them
            sel.register(sock, selectors.EVENT_READ, "sock")
            sel.register(self._wake_r, selectors.EVENT_READ, "wake")
            while not self._stop.is_set():
                for key, _ev in sel.select(min(1.0, self.timeout / 4)):
                    if key.data == "wake":
                        try:
                            self._wake_r.recv(4096)
                        except (BlockingIOError, OSError):
                            pass
                        continue
                    data = sock.recv(65536)
                    if not data:
                        raise OSError("connection closed by the pool")
                    for line in buf.feed(data):
                        self._handle(S.decode(line))
                self._send_shares(sock)
                now = time.monotonic()
                for i in [i for i, (t, _s) in self._pending.items() if now - t > self.timeout]:
                    self._pending.pop(i)
                    self.count("lost", 1)
        finally:
            sel.close()
            try:
                sock.close()
            except OSError:
                pass

    def _send_shares(self, sock) -> None:
        while True:
            try:
                session, seq, sub = self.shares.get_nowait()
            except queue.Empty:
                return
            with self.lock:
                live = session == self.session and seq >= self.live_seq
            if not live:  # another connection's extranonce, or a clean job arrived since it was found
                self.count("stale_shares", 1)
                continue
            msg_id = self._next_id
            self._next_id += 1
            self._pending[msg_id] = (time.monotonic(), sub)
            self.count("submitted", 1)
            self.sent.append(sub)
            del self.sent[:-256]
            sock.sendall(S.submit(msg_id, sub))

    def _handle(self, m: S.Message) -> None:
        if m.is_response:
            ent = self._pending.pop(m.id, None) if isinstance(m.id, int) else None
            if ent is None:
                return
            ok = m.result is True and not m.error
            self.count("accepted" if ok else "rejected", 1)
            if not ok and m.error_code in (S.ERR_STALE, S.ERR_DUPLICATE):
                self.count("rejected_stale", 1)  # the job changed while the share travelled: routine
            log.log_printf(f"stratum: share nonce {ent[1].nonce:016x} of job {ent[1].job_id} -> "
                           f"{'accepted' if ok else m.error}")
            return
        try:
            if m.method == "mining.set_target":
                self.target = S.parse_set_target(m.params)
            elif m.method == "mining.notify":
                self._on_job(S.Job.from_params(m.params))
            # anything else: an unknown notification, ignored
        except S.StratumError as e:
            log.log_printf(f"stratum: bad {m.method}: {e}")

    def _on_job(self, job: S.Job) -> None:
        want = _core.epoch_seed(job.height // _core.EPOCH_LENGTH)
        if job.seed_hash != want:
            self.count("refused_jobs", 1)
            if job.seed_hash not in self._refused_seeds:  # mining it would use the wrong DAG
                self._refused_seeds.add(job.seed_hash)
                log.log_printf(f"stratum: job {job.job_id} at height {job.height} refused: its seed hash "
                               f"{job.seed_hash.hex()} is not this engine's seed of epoch "
                               f"{job.height // _core.EPOCH_LENGTH} ({want.hex()})")
            return
        self.target = job.target  # a target in mining.notify replaces the last mining.set_target
        with self.lock:
            self.job_seq += 1
            if job.clean:
                self.live_seq = self.job_seq
            self.job = job
        self.count("jobs", 1)


class StratumLeader:
    """Rank 0 of a pool miner's mining loop, with the leader interface of RemoteLeader. It never
    does I/O: work comes from the connection's memory and shares go onto its queue."""

    def __init__(self, conn: StratumConnection):
        self.conn = conn
        self.stats = conn.stats
        self.world_size = 1  # declared: the mining service keeps it current (also after a shrink)
        self.stopping = False
        self.job_id = 0      # the work packet's job id: +1 whenever (session, header hash, ranks) changes
        self._key = None
        self._seq_seen = 0
        self._live: dict[int, tuple[int, int, bytes, S.Job]] = {}  # job id -> (session, seq, extranonce, job)
        self._exhausted: set[tuple[int, int]] = set()

    def next_work(self, repartitioned: bool = False):
        from .search import FLAG_CLEAN, FLAG_IDLE, FLAG_STOP, Work, rank_shift_flags

        if self.stopping:
            return Work(flags=FLAG_STOP)
        session, extranonce, job, seq, live_seq = self.conn.snapshot()
        if not session or job is None:
            self._key = None
            self._live.clear()
            return Work(flags=FLAG_IDLE)
        base, free = S.extranonce_range(extranonce)
        try:
            shift = S.rank_shift_for(free, self.world_size)
        except S.StratumError as e:
            log.log_printf(f"stratum: {e}; idle")
            return Work(flags=FLAG_IDLE)
        key = (session, job.header_hash, job.height, self.world_size)
        flags = 0
        if key != self._key or repartitioned:
            self._key = key
            self.job_id += 1
            flags = FLAG_CLEAN
        if seq != self._seq_seen:
            self._seq_seen = seq
            if job.clean:
                flags = FLAG_CLEAN
        # shares of older jobs stay welcome only while every newer job came with clean_jobs false
        for jid in [j for j, (s, q, _x, _job) in self._live.items() if s != session or q < live_seq]:
            del self._live[jid]
        self._live[self.job_id] = (session, seq, extranonce, job)
        while len(self._live) > 8:
            del self._live[min(self._live)]
        return job.work(self.job_id, base, flags | rank_shift_flags(shift))

    def on_results(self, records) -> None:
        from .service import _as_record

        for r, rec in enumerate(records):
            rec = _as_record(rec)
            self.conn.count("hashes", rec.hashes)
            self.conn.count("windows", rec.hashes > 0)
            self.conn.count("shares_dropped", getattr(rec, "dropped", 0))
            if getattr(rec, "exhausted", False) and (r, self.job_id) not in self._exhausted:
                self._exhausted = {x for x in self._exhausted if x[1] == self.job_id} | {(r, self.job_id)}
                self.conn.count("exhausted", 1)
                log.log_printf(f"stratum: rank {r} has searched its whole nonce range of job {self.job_id}; "
                               "it waits for the next job")
            if not rec.shares:
                continue
            ent = self._live.get(rec.job_id)
            if ent is None:
                self.conn.count("stale_shares", len(rec.shares))
                continue
            session, seq, extranonce, job = ent
            for sh in rec.shares:
                if not S.nonce_in_extranonce(sh.nonce, extranonce) or not sh.verify_full(job.height, job.header_hash):
                    self.conn.count("bad_shares", 1)
                    log.log_printf(f"stratum: share nonce {sh.nonce:016x} failed the full re-hash; dropped")
                    continue
                if int.from_bytes(sh.final_hash, "big") > job.target:
                    # found under an easier target of the same header, which the pool has tightened
                    # since the window was queued: an honest share that is worth nothing now
                    self.conn.count("above_target", 1)
                    continue
                self.conn.queue_share(session, seq, S.Submit(self.conn.user, job.job_id, sh.nonce, job.header_hash,
                                                             bytes(sh.mix_hash)))

    def shutdown(self) -> None:
        self.stopping = True


class StratumMiner:
    """The pool miner: the node's own mining loop (pipelined windows, device-side stale-work abort,
    full share re-hash) with a StratumLeader in place of the chain."""

    def __init__(self, endpoints, backend, *, user: str = "", password: str = "x", window: int = 1 << 22,
                 timeout: float = 30.0, backoff: tuple[float, float] = (0.5, 30.0)):
        from .remote import _device_for
        from .service import MiningService

        self.conn = StratumConnection(endpoints, user, password, timeout=timeout, backoff=backoff)
        self.leader = StratumLeader(self.conn)
        self.dev = _device_for(backend)
        if getattr(self.dev, "name", "") == "cpu" and hasattr(self.dev, "max_window"):
            self.dev.max_window = min(self.dev.max_window, int(window))
        self.service = MiningService(self.dev, self.leader, window=int(window))
        self.stats = self.conn.stats
        self._stop = threading.Event()

    def stop(self) -> None:
        self._stop.set()

    def run(self, max_shares: int | None = None, max_seconds: float | None = None) -> dict:
        """Mine until `max_shares` shares were accepted (-blocks), `max_seconds` passed or stop()."""
        t0 = time.time()
        self.conn.start()
        try:
            while not self._stop.is_set():
                if max_shares is not None and self.stats["accepted"] >= max_shares:
                    break
                if max_seconds is not None and time.time() - t0 > max_seconds:
                    break
                self.service.step()
        finally:
            try:
                self.service.pipe.drain()
            except Exception:  # noqa: BLE001
                pass
            self.conn.stop()
        out = dict(self.stats)
        out["seconds"] = round(time.time() - t0, 3)
        out["kernel"] = getattr(getattr(self.dev, "kawpow", self.dev), "kernel_kind", "")
        return out
