"""Stratum for KawPow on the host: the codec (miner/stratum.py), both ends against hand-written
transcripts (tests/golden/stratum/) and against each other, the nonce ranges under a pool's
extranonce in the mining loop, the server's share checks, the client against a scripted fake pool,
and the node serving a miner process end to end.

Light-mode KawPow on the host costs several milliseconds per hash, so the shares these tests
submit were found once with the host golden model (`kawpow_search_light`, share target 2^-8) and
are recorded in tests/golden/stratum/shares.json; every run re-hashes them (`shares` fixture) and
the server verifies each with the full hash. For the same reason the nonce-range tests, which count
65,536 nonces through `CpuSearchDevice`, replace the native search call under it with one that
hashes nothing: the windows, their clipping and the exhaustion are the mining loop's work, which
runs unchanged."""
import ast
import json
import os
import socket
import subprocess
import sys
import threading
import time

import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stratum")
H = bytes([0x11]) * 32
HEIGHT = 1
SHARE_TARGET = (1 << 248) - 1   # 2^-8
BLOCK_TARGET = (1 << 216) - 1   # 2^-40
KAWPOW_REGTEST = "-kawpowactivationtime=1524179367"


def _wait(cond, timeout=20.0, what="condition"):
    end = time.monotonic() + timeout
    while not cond():
        if time.monotonic() > end:
            raise AssertionError(f"timed out waiting for {what}")
        time.sleep(0.005)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _transcript(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return [json.loads(line) for line in f if line.strip()]


@pytest.fixture(scope="module")
def shares(core, ctx0):
    """The recorded shares, re-hashed: {"shares": [Share x3], "high": Share above the target}."""
    from nodexa_chain_core_amd.ops.kawpow import Share

    with open(os.path.join(GOLDEN, "shares.json")) as f:
        g = json.load(f)
    assert bytes.fromhex(g["header_hash"]) == H and g["height"] == HEIGHT
    out = {"shares": [], "high": None}
    for ent in g["shares"] + [g["high"]]:
        nonce = int(ent["nonce"], 16)
        fin, mix = core.kawpow_hash(ctx0, HEIGHT, H, nonce)
        assert (fin.hex(), mix.hex()) == (ent["final"], ent["mix"])
        assert nonce >> 48 == 1
        out["shares"].append(Share(nonce, mix, fin))
    out["high"] = out["shares"].pop()
    assert all(int.from_bytes(s.final_hash, "big") <= SHARE_TARGET for s in out["shares"])
    assert int.from_bytes(out["high"].final_hash, "big") > SHARE_TARGET
    return out


class Peer:
    """A raw line-oriented end of a Stratum connection."""

    def __init__(self, sock):
        self.s = sock
        self.s.settimeout(20)
        self.f = sock.makefile("rb")
        self.notes = []

    @classmethod
    def connect(cls, port):
        return cls(socket.create_connection(("127.0.0.1", port), timeout=20))

    def send(self, obj):
        self.s.sendall((json.dumps(obj) + "\n").encode())

    def recv(self):
        line = self.f.readline()
        return json.loads(line) if line else None

    def call(self, msg_id, method, params):
        self.send({"id": msg_id, "method": method, "params": params})
        while True:
            m = self.recv()
            if m is None or m.get("id") == msg_id:
                return m
            self.notes.append(m)

    def login(self, password="x"):
        assert self.call(1, "mining.subscribe", ["test/1.0"])["error"] is None
        assert self.call(2, "mining.authorize", ["w", password])["result"] is True

    def submit(self, msg_id, job_id, share, header=H, mix=None, prefix="0x"):
        return self.call(msg_id, "mining.submit", ["w", job_id, prefix + "%016x" % share.nonce, prefix + header.hex(),
                                                   prefix + (mix or share.mix_hash).hex()])

    def close(self):
        for fn in (lambda: self.s.shutdown(socket.SHUT_RDWR), self.f.close, self.s.close):
            try:
                fn()
            except OSError:
                pass


# ---------------------------------------------------------------------- 1. codec
def test_codec_round_trips():
    from nodexa_chain_core_amd.miner import stratum as S

    job = S.Job("a1", H, bytes(32), SHARE_TARGET, True, 7501, 0x1B00FFFF)
    m = S.decode(S.notify(job))
    assert m.id is None and m.method == "mining.notify" and S.Job.from_params(m.params) == job
    assert m.params[3] == "00" + "ff" * 31 and m.params[6] == "1b00ffff"
    sub = S.Submit("w", "a1", 0x0001_0000_0000_00AC, H, bytes(range(32)))
    m = S.decode(S.submit(9, sub))
    assert m.id == 9 and m.method == "mining.submit" and S.Submit.from_params(m.params) == sub
    assert all(p.startswith("0x") for p in m.params[2:])  # sent with the prefix
    bare = [m.params[0], m.params[1]] + [p[2:] for p in m.params[2:]]
    assert S.Submit.from_params(bare) == sub  # accepted without it
    assert S.decode(S.subscribe(1, "agent/1")).params == ["agent/1"]
    assert S.decode(S.authorize(2, "u", "p")).params == ["u", "p"]
    assert S.parse_set_target(S.decode(S.set_target(SHARE_TARGET)).params) == SHARE_TARGET
    r = S.decode(S.response(3, S.subscribe_result(None, b"\x00\x01")))
    assert r.is_response and r.id == 3 and S.parse_subscribe_result(r.result) == (None, b"\x00\x01")
    e = S.decode(S.error_response(4, S.ERR_DUPLICATE))
    assert e.is_response and e.error_code == 22 and e.error == [22, "duplicate share", None] and e.result is None
    assert S.decode(S.request(5, "x.y", [])).method == "x.y"


def test_codec_refuses_bad_fields():
    from nodexa_chain_core_amd.miner import stratum as S

    good = ["w", "j", "0x" + "0" * 16, "0x" + "11" * 32, "0x" + "22" * 32]
    for i, bad in ((2, "0x" + "0" * 15), (2, "0" * 17), (3, "11" * 31), (4, "0x" + "22" * 33), (4, "zz" * 32), (2, 5)):
        p = list(good)
        p[i] = bad
        with pytest.raises(S.StratumError) as ei:
            S.Submit.from_params(p)
        assert ei.value.code == 20 and not ei.value.fatal
    with pytest.raises(S.StratumError):
        S.Submit.from_params(good[:4])
    with pytest.raises(S.StratumError):
        S.Job.from_params(["j", "11" * 32, "00" * 32, "ff" * 31, True, 1, "1d00ffff"])  # short target
    with pytest.raises(S.StratumError):
        S.Job.from_params(["j", "11" * 32, "00" * 32, "ff" * 32, True, 1, "1d00ff"])   # short bits
    for x in ("", "00", "0001", "00" * 6):
        assert S.parse_extranonce(x) == bytes.fromhex(x)
    for x in ("0", "000", "00" * 7, "0g"):  # odd length, longer than 12 digits, not hex
        with pytest.raises(S.StratumError):
            S.parse_extranonce(x)
    assert S.extranonce_range(b"") == (0, 64)
    assert S.extranonce_range(b"\x00\x01") == (1 << 48, 48)
    assert S.extranonce_range(bytes.fromhex("aabbccddeeff")) == (0xAABBCCDDEEFF << 16, 16)
    assert S.nonce_in_extranonce((1 << 48) + 5, b"\x00\x01") and not S.nonce_in_extranonce((2 << 48) + 5, b"\x00\x01")
    assert [S.rank_shift_for(16, w) for w in (1, 2, 3, 4, 8)] == [16, 15, 14, 14, 13]


def test_codec_refuses_bad_lines():
    from nodexa_chain_core_amd.miner import stratum as S

    for line in (b"[1,2]", b'"x"', b"17", b"{not json", b"\xff\xfe"):
        with pytest.raises(S.StratumError) as ei:
            S.decode(line)
        assert ei.value.fatal
    long = b'{"id":1,"method":"m","params":["' + b"a" * (16 * 1024) + b'"]}'
    with pytest.raises(S.StratumError) as ei:
        S.decode(long)
    assert ei.value.fatal
    buf = S.LineBuffer()
    assert buf.feed(b'{"id":1}\n{"id"') == [b'{"id":1}'] and buf.feed(b":2}\n") == [b'{"id":2}']
    with pytest.raises(S.StratumError) as ei:
        buf.feed(b"a" * (16 * 1024 + 1))  # no newline in sight
    assert ei.value.fatal
    with pytest.raises(S.StratumError):
        S.LineBuffer().feed(long + b"\n")


# ---------------------------------------------------------------------- server fixtures
def _server_job(job_id="j1", header=H, tip="tipA", clean=True, block_target=BLOCK_TARGET):
    from nodexa_chain_core_amd.miner.stratum_server import ServerJob

    return ServerJob(job_id, header, HEIGHT, block_target, 0x1D00FFFF, clean, tip)


@pytest.fixture()
def server(core):
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    made = []

    def make(**kw):
        src = StaticJobSource()
        srv = StratumServer(src, share_bits=8, **kw).start()
        made.append(srv)
        return srv, src

    yield make
    for srv in made:
        srv.stop()


# ---------------------------------------------------------------------- 2. transcripts
def test_server_transcript(server, shares):
    srv, src = server()
    src.push(_server_job())
    p = Peer.connect(srv.port)
    try:
        for i, ent in enumerate(_transcript("server_transcript.jsonl")):
            if ent["dir"] == "c2s":
                p.send(ent["msg"])
            else:
                assert p.recv() == ent["msg"], f"line {i + 1}"
    finally:
        p.close()
    assert srv.stats["verified_host"] == 2 and srv.stats["verified_gpu"] == 0


class FakePool:
    """A scripted pool: `handler(index, peer)` runs on a thread of its own for every connection."""

    def __init__(self, handler):
        self.handler = handler
        self.ls = socket.socket()
        self.ls.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self.ls.bind(("127.0.0.1", 0))
        self.ls.listen(8)
        self.port = self.ls.getsockname()[1]
        self.peers = []
        self.errors = []
        self.t = threading.Thread(target=self._accept, daemon=True)
        self.t.start()

    def _accept(self):
        while True:
            try:
                s, _ = self.ls.accept()
            except OSError:
                return
            p = Peer(s)
            self.peers.append(p)
            threading.Thread(target=self._serve, args=(len(self.peers) - 1, p), daemon=True).start()

    def _serve(self, i, p):
        try:
            self.handler(i, p)
        except (OSError, ValueError):
            pass
        except AssertionError as e:
            self.errors.append(f"connection {i}: {e}")

    def close(self):
        self.ls.close()
        for p in self.peers:
            p.close()


def _handshake(p, extranonce):
    m = p.recv()
    assert m["method"] == "mining.subscribe", m
    p.send({"id": m["id"], "result": [None, extranonce], "error": None})
    m = p.recv()
    assert m["method"] == "mining.authorize", m
    p.send({"id": m["id"], "result": True, "error": None})


def _notify(job_id="j1", header=H, clean=True, seed=bytes(32), target=SHARE_TARGET):
    return {"id": None, "method": "mining.notify",
            "params": [job_id, header.hex(), seed.hex(), "%064x" % target, clean, HEIGHT, "1d00ffff"]}


def _client(port, **kw):
    from nodexa_chain_core_amd.miner.stratum_client import StratumConnection, StratumLeader

    conn = StratumConnection([("127.0.0.1", port)], kw.pop("user", "w"), kw.pop("password", "x"), backoff=(0.02, 0.1),
                             **kw).start()
    return conn, StratumLeader(conn)


def _work(leader, what="a job"):
    """The leader's next non-idle work packet."""
    box = []

    def ready():
        w = leader.next_work()
        if not w.idle:
            box.append(w)
        return bool(box)

    _wait(ready, what=what)
    return box[0]


def test_client_transcript(core, shares):
    from nodexa_chain_core_amd.miner.search import FLAG_CLEAN

    script = _transcript("client_transcript.jsonl")
    done = threading.Event()

    def handler(i, p):
        for n, ent in enumerate(script):
            if ent["dir"] == "s2c":
                p.send(ent["msg"])
            else:
                got = p.recv()
                assert got == ent["msg"], f"line {n + 1}: {got}"
        done.set()

    pool = FakePool(handler)
    conn, leader = _client(pool.port, user="worker.1", password="secret")
    try:
        w = _work(leader)
        assert w.header_hash == H and w.height == HEIGHT and w.flags & FLAG_CLEAN
        assert w.target() == SHARE_TARGET  # the notify's target replaced mining.set_target's
        assert (w.nonce_base, w.rank_shift) == (1 << 48, 48)
        leader.on_results([(w.job_id, 4096, shares["shares"][:2])])
        assert done.wait(20), pool.errors
        _wait(lambda: conn.stats["accepted"] + conn.stats["rejected"] == 2, what="both answers")
        assert not pool.errors, pool.errors
        assert (conn.stats["accepted"], conn.stats["rejected"], conn.stats["submitted"]) == (1, 1, 2)
    finally:
        conn.stop()
        pool.close()


# ---------------------------------------------------------------------- 3. nonce ranges
class _FakeConn:
    """The memory side of a StratumConnection, no thread and no socket."""

    def __init__(self, extranonce: bytes):
        from nodexa_chain_core_amd.miner import stratum as S
        from nodexa_chain_core_amd.miner.stratum_client import new_stats

        self.S = S
        self.stats = new_stats()
        self.user = "w"
        self.extranonce = extranonce
        self.seq = 0
        self.job = None
        self.queued = []

    def new_job(self, header: bytes, clean=True, target=0):
        self.seq += 1
        self.job = self.S.Job("j%d" % self.seq, header, bytes(32), target, clean, HEIGHT, 0)  # target 0: no share ever

    def count(self, key, n=1):
        self.stats[key] += n

    def snapshot(self):
        return 1, self.extranonce, self.job, self.seq, self.seq

    def queue_share(self, *a):
        self.queued.append(a)


def _no_hash_search(monkeypatch_setattr):
    """Replace the native light search under CpuSearchDevice with one that hashes nothing (see the
    module docstring)."""
    from nodexa_chain_core_amd.miner import search

    class _Core:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            return getattr(self._real, name)

        @staticmethod
        def kawpow_search_light(ctx, height, hh, boundary, start, count):
            return False, 0, b"", b""

    monkeypatch_setattr(search, "_core", _Core(search._core))


def _range_run(rank_world=(0, 1)):
    """Drive the loop over a 6-byte extranonce; returns what the range assertions need."""
    from nodexa_chain_core_amd.miner.search import CpuSearchDevice
    from nodexa_chain_core_amd.miner.service import MiningService
    from nodexa_chain_core_amd.miner.stratum_client import StratumLeader

    rank, world = rank_world
    conn = _FakeConn(bytes.fromhex("aabbccddeeff"))
    leader = StratumLeader(conn) if rank == 0 else None
    svc = MiningService(CpuSearchDevice(max_window=4096), leader, window=4096, record_windows=True, idle_sleep_s=0.0)
    conn.new_job(H)
    per_rank = 65536 // world
    steps = per_rank // 4096 + 2  # the idle first step, the windows, the drain of the last one
    for _ in range(steps):
        svc.step()
    first = {"windows": list(svc.windows), "hashes": svc.hashes_total}
    for _ in range(3):
        svc.step()
    later = {"windows": list(svc.windows), "hashes": svc.hashes_total}
    conn.new_job(bytes([0x22]) * 32)
    for _ in range(4):
        svc.step()
    resumed = {"windows": list(svc.windows), "hashes": svc.hashes_total}
    stats = dict(conn.stats)
    if leader is not None:
        leader.shutdown()
    while svc.step():
        pass
    return first, later, resumed, stats, (leader.world_size if leader else None)


def test_nonce_range_one_rank(core, monkeypatch):
    _no_hash_search(monkeypatch.setattr)
    first, later, resumed, stats, ws = _range_run()
    base = 0xAABBCCDDEEFF << 16
    assert ws == 1
    wins = first["windows"]
    assert len(wins) == 16 and first["hashes"] == 65536  # after 16 windows the rank is exhausted
    assert [s for _j, s, _c in wins] == [base + i * 4096 for i in range(16)] and all(c == 4096 for _j, _s, c in wins)
    assert all(base <= s and s + c <= base + 65536 for _j, s, c in wins)  # inside the prefix, none twice (distinct starts)
    assert later == first and stats["exhausted"] == 1  # zero hashes, no further window, until a new job
    new = resumed["windows"][16:]
    assert new and new[0][1] == base and new[0][0] != wins[0][0] and resumed["hashes"] > 65536
    assert stats["shares_dropped"] == 0


def _range_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        from nodexa_chain_core_amd.parallel import world as W

        W.init(use_gpu=False)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_stratum as T

        T._no_hash_search(setattr)
        first, later, resumed, stats, ws = T._range_run((rank, world))
        W.shutdown()
        q.put((rank, (first, later, resumed, stats, ws)))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc()))


@pytest.mark.timeout(300)
def test_nonce_range_two_ranks_gloo(core):
    """A gloo world of 2 under the same 16 free bits: rank_shift 15, disjoint halves."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_range_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=280) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert all(not isinstance(v, str) for v in results.values()), results
    base = 0xAABBCCDDEEFF << 16
    for r in (0, 1):
        first, later, _resumed, _stats, _ws = results[r]
        lo = base + (r << 15)
        assert [s for _j, s, _c in first["windows"]] == [lo + i * 4096 for i in range(8)], r
        assert later["windows"] == first["windows"]
    first0, later0, resumed0, stats0, ws0 = results[0]
    assert ws0 == 2 and first0["hashes"] == later0["hashes"] == 65536  # both halves, summed on every rank
    assert stats0["exhausted"] == 2 and resumed0["hashes"] > 65536


def test_clipped_windows_through_the_real_host_search(core):
    """The same clipping with CpuSearchDevice hashing for real: an empty extranonce and a rank_shift
    of 4 leave 16 nonces, which windows of 6 cover as 6 + 6 + 4; then the rank is exhausted."""
    from nodexa_chain_core_amd.miner.search import FLAG_CLEAN, CpuSearchDevice, Work, rank_shift_flags
    from nodexa_chain_core_amd.miner.service import BenchLeader, MiningService

    w = Work(H, bytes(32), HEIGHT, 5, 0x7700, FLAG_CLEAN | rank_shift_flags(4))  # boundary 0: every nonce is hashed
    assert w.rank_shift == 4 and w.rank_bounded and Work.unpack(w.pack()).rank_shift == 4 and len(w.pack()) == 144
    leader = BenchLeader(w)
    leader.work = Work(w.header, w.boundary, w.height, w.job_id, w.nonce_base, rank_shift_flags(4))  # keep the shift
    svc = MiningService(CpuSearchDevice(max_window=6), leader, window=6, record_windows=True, idle_sleep_s=0.0)
    for _ in range(8):
        svc.step()
    assert svc.windows == [(5, 0x7700, 6), (5, 0x7706, 6), (5, 0x770C, 4)] and svc.hashes_total == 16


def test_leader_with_an_empty_extranonce(core):
    """The wire format allows an extranonce of no bytes: 64 free bits, carried as the largest
    rank_shift a packet holds."""
    from nodexa_chain_core_amd.miner.search import Work
    from nodexa_chain_core_amd.miner.stratum_client import StratumLeader

    for world, shift in ((1, 63), (2, 63), (4, 62)):
        conn = _FakeConn(b"")
        conn.new_job(H)
        leader = StratumLeader(conn)
        leader.world_size = world
        w = Work.unpack(leader.next_work().pack())
        assert not w.idle and (w.nonce_base, w.rank_shift) == (0, shift) and w.rank_bounded
        assert ((world - 1) << shift) + (1 << shift) <= 1 << 64  # the last rank's range ends inside 64 bits


def test_share_above_a_tightened_target_is_not_a_bad_share(core, shares):
    """The pool re-sends the header with a harder target while a window is in flight: its honest
    share is worth nothing now, but it did not fail the re-hash."""
    from nodexa_chain_core_amd.miner.stratum_client import StratumLeader

    conn = _FakeConn(b"\x00\x01")
    leader = StratumLeader(conn)
    conn.new_job(H, target=SHARE_TARGET)
    w1 = leader.next_work()
    conn.new_job(H, clean=False, target=BLOCK_TARGET)
    w2 = leader.next_work()
    assert w2.job_id == w1.job_id and w2.target() == BLOCK_TARGET
    leader.on_results([(w1.job_id, 4096, shares["shares"][:2])])
    assert (conn.stats["above_target"], conn.stats["bad_shares"], conn.queued) == (2, 0, [])


def test_rank_shift_zero_is_the_old_partition(core, monkeypatch):
    """A packet without a rank_shift (every existing leader's) starts its windows where the
    partition formula always put them, and is never clipped."""
    from nodexa_chain_core_amd.miner.search import CpuSearchDevice, Work
    from nodexa_chain_core_amd.miner.service import BenchLeader, MiningService

    _no_hash_search(monkeypatch.setattr)
    nonce_base = 0x5EED_0000_0000_0000
    w = Work(H, bytes(32), HEIGHT, 3, nonce_base, 0)
    assert w.rank_shift == 56 and not w.rank_bounded and Work.unpack(w.pack()) == w and len(w.pack()) == 144
    svc = MiningService(CpuSearchDevice(max_window=4096), BenchLeader(w), window=4096, record_windows=True)
    for _ in range(6):
        svc.step()
    rank, cursor = 0, 0
    for _job, start, count in svc.windows:
        assert start == (nonce_base + (rank << 56) + cursor) & 0xFFFFFFFFFFFFFFFF
        cursor += count
    assert len(svc.windows) == 5
    for rank in (1, 5):  # the formula itself, for other ranks of a world
        svc.comm.w = type("W", (), {"rank": rank, "world_size": 8})()
        svc.cursor = 12288
        assert svc._window_start(w) == nonce_base + (rank << 56) + 12288
        assert svc._clip_window(w, 4096) == 4096


def test_dropped_shares_are_counted(core):
    """What the device ring (SlotResult.dropped) and the record's 16-share cap lose reaches the
    leader's `shares_dropped`; a record within both limits is packed as it always was."""
    from nodexa_chain_core_amd.miner.search import SlotResult
    from nodexa_chain_core_amd.miner.service import pack_record, unpack_record
    from nodexa_chain_core_amd.miner.stratum_client import StratumLeader
    from nodexa_chain_core_amd.ops.kawpow import Share

    twenty = [Share(i, bytes([i]) * 32, bytes([i + 1]) * 32) for i in range(20)]
    rec = unpack_record(pack_record(SlotResult(7, 0, 4096, 4096, twenty, dropped=5)))
    assert len(rec.shares) == 16 and rec.dropped == 9 and not rec.exhausted
    few = unpack_record(pack_record(SlotResult(7, 0, 4096, 4096, twenty[:3]), exhausted=True))
    assert len(few.shares) == 3 and few.dropped == 0 and few.exhausted and few.has_result
    assert pack_record(SlotResult(7, 0, 4096, 4096, twenty[:3]))[16:20] == (3).to_bytes(4, "little")
    conn = _FakeConn(b"\x00\x01")
    leader = StratumLeader(conn)
    rec.shares = []
    leader.on_results([rec])
    assert conn.stats["shares_dropped"] == 9


# ---------------------------------------------------------------------- 4. server share handling
def test_server_share_checks(server, shares):
    """Block target 2^-40, share target 2^-8. No 2^-40 share can be found on the host, so the case
    of a share that meets the block target injects a second job whose block target is the hash of
    one of the recorded shares: that share meets it, the next one does not."""
    found = []
    srv, src = server()
    src.on_block = lambda job, nonce, mix: found.append((job.job_id, nonce, mix))
    src.push(_server_job("j1"))
    good, second, third = shares["shares"]
    p = Peer.connect(srv.port)
    try:
        assert p.submit(1, "j1", good)["error"][0] == 25                     # not subscribed
        assert p.call(2, "mining.subscribe", ["t/1"])["result"] == [None, "0001"]
        assert p.submit(3, "j1", good)["error"][0] == 24                     # not authorized
        assert p.call(4, "mining.authorize", ["w", "x"])["result"] is True
        assert p.submit(5, "nope", good)["error"][0] == 21                   # job not found
        assert p.submit(6, "j1", good, header=bytes(32))["error"][0] == 20   # wrong header hash for the job
        assert p.call(7, "mining.submit", ["w", "j1", "0x12", "0x" + H.hex(), "0x" + good.mix_hash.hex()])["error"][0] == 20
        other = type(good)(good.nonce + (1 << 48), good.mix_hash, good.final_hash)
        assert p.submit(8, "j1", other)["error"][0] == 20                    # nonce outside the extranonce
        assert p.call(9, "mining.frobnicate", [])["error"][0] == 20          # unknown method
        before = dict(srv.stats)
        assert before["verified_host"] == 0
        assert p.submit(10, "j1", shares["high"])["error"][0] == 23          # above the share target
        assert p.submit(11, "j1", good) == {"id": 11, "result": True, "error": None}
        assert p.submit(12, "j1", good, prefix="")["error"][0] == 22         # duplicate
        # the share above the target never reached the full-hash verifier: one share, one batch
        assert (srv.stats["verified_host"], srv.stats["verify_batches_host"], srv.stats["verified_gpu"]) == (1, 1, 0)
        assert not found  # 2^-8 shares do not meet the 2^-40 block target
        info = srv.info()
        c = info["connections"][0]
        assert info["serving"] and info["job"]["id"] == "j1" and info["share_target"] == "00" + "ff" * 31
        assert c["accepted"] == 1 and c["rejected"] == {"20": 3, "21": 1, "22": 1, "23": 1, "24": 1, "25": 1}
        assert c["extranonce"] == "0001" and c["agent"] == "t/1" and c["hashrate"] > 0
        # a job on a new tip: the old job is stale, and a share that meets its block target is a block
        src.push(_server_job("j2", tip="tipB", block_target=int.from_bytes(second.final_hash, "big")))
        assert p.submit(13, "j1", second)["error"][0] == 21                  # built on the old tip
        assert p.submit(14, "j2", third)["result"] is True and not found     # above j2's block target
        assert p.submit(15, "j2", second)["result"] is True
        assert found == [("j2", second.nonce, second.mix_hash)] and srv.blocks_found == 1
        assert [n["params"][0] for n in p.notes if n["method"] == "mining.notify"] == ["j1", "j2"]
    finally:
        p.close()


def test_server_wrong_mix_closes(server, shares, core):
    srv, src = server()
    src.push(_server_job("j1"))
    good = shares["shares"][0]
    p, q = Peer.connect(srv.port), Peer.connect(srv.port)
    try:
        p.login()
        q.login()
        nonce = (1 << 48) + 7
        k = 0
        while True:  # a mix that passes the cheap check for this nonce and is not the real one
            mix = core.sha256d(b"forged mix %d" % k)
            k += 1
            if int.from_bytes(core.kawpow_hash_no_verify(HEIGHT, H, mix, nonce), "big") <= SHARE_TARGET:
                break
        r = p.submit(3, "j1", type(good)(nonce, mix, b""))
        assert r["error"][0] == 20 and "mix" in r["error"][1]
        assert p.recv() is None  # closed
        assert srv.stats["verified_host"] == 1
        _wait(lambda: len(srv.info()["connections"]) == 1, what="the connection to go")
        assert q.call(4, "mining.subscribe", ["again"])["error"] is None  # the other connection is served as before
        assert q.submit(5, "j1", good)["error"][0] == 20  # (its own extranonce is 0002)
    finally:
        p.close()
        q.close()


def test_server_password_limits_and_bad_lines(server):
    srv, src = server(password="pw", max_connections=2)
    a = Peer.connect(srv.port)
    try:
        assert a.call(1, "mining.authorize", ["w", "pw"])["error"][0] == 25
        a.call(2, "mining.subscribe", ["t"])
        assert a.call(3, "mining.authorize", ["w", "wrong"])["error"][0] == 24
        assert a.call(4, "mining.authorize", ["w", "pw"])["result"] is True
        b = Peer.connect(srv.port)
        assert b.call(1, "mining.subscribe", ["t"])["result"] == [None, "0002"]  # unique among the live connections
        c = Peer.connect(srv.port)  # the third of two: refused
        assert c.recv() is None
        b.s.sendall(b"[1, 2, 3]\n")  # not a JSON object
        assert b.recv() is None
        _wait(lambda: len(srv.info()["connections"]) == 1, what="the slot to free")
        d = Peer.connect(srv.port)
        d.s.sendall(b'{"id":1,"method":"mining.subscribe","params":["' + b"a" * 17000)  # an over-long line
        assert d.recv() is None
        assert srv.stats["refused_connections"] == 1
        # no job yet: connections stay open and get the job when it comes
        src.push(_server_job("j9"))
        _wait(lambda: a.call(9, "mining.subscribe", ["t"]) and any(n["method"] == "mining.notify" for n in a.notes),
              what="the pushed job")
    finally:
        a.close()


def test_server_slow_peer_is_closed(server):
    """A peer that never reads fills its own send buffer and is closed; the others are served."""
    srv, src = server()
    src.push(_server_job("j0"))
    slow = socket.create_connection(("127.0.0.1", srv.port))
    slow.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 4096)
    slow.sendall(b'{"id":1,"method":"mining.subscribe","params":["slow"]}\n'
                 b'{"id":2,"method":"mining.authorize","params":["w","x"]}\n')
    fast = Peer.connect(srv.port)
    try:
        fast.login()
        _wait(lambda: len(srv.info()["connections"]) == 2 and all(c["user"] for c in srv.info()["connections"]),
              what="both logins")
        conn = next(c for c in srv.conns.values() if c.agent == "slow")
        junk = b'{"id":null,"method":"client.show_message","params":["' + b"x" * 8000 + b'"]}\n'
        for _ in range(4096):  # far more than the socket buffers and the 64 KiB queue hold
            srv._send(conn, junk)
            if srv.stats["slow_closed"]:
                break
        assert srv.stats["slow_closed"] == 1
        _wait(lambda: len(srv.info()["connections"]) == 1, what="the slow connection to be closed")
        assert fast.call(5, "mining.subscribe", ["still here"])["error"] is None
    finally:
        slow.close()
        fast.close()


# ---------------------------------------------------------------------- 5. client against a fake pool
def test_client_submits_all_shares_and_drops_stale(core, shares):
    from nodexa_chain_core_amd.miner.search import FLAG_CLEAN

    got = []

    def handler(i, p):
        _handshake(p, "0001")
        p.send(_notify("j1"))
        while True:
            m = p.recv()
            if m is None:
                return
            got.append(m)
            p.send({"id": m["id"], "result": True, "error": None})

    pool = FakePool(handler)
    conn, leader = _client(pool.port)
    three = shares["shares"]
    try:
        w1 = _work(leader)
        assert w1.flags & FLAG_CLEAN and not leader.next_work().flags & FLAG_CLEAN
        leader.on_results([(w1.job_id, 4096, three)])  # one record, three shares: all go out
        _wait(lambda: conn.stats["accepted"] == 3, what="3 accepted shares")
        assert [m["params"] for m in got] == [["w", "j1", "0x%016x" % s.nonce, "0x" + H.hex(), "0x" + s.mix_hash.hex()]
                                              for s in three]
        # a share that fails the full re-hash is dropped here, not sent
        leader.on_results([(w1.job_id, 0, [type(three[0])(three[0].nonce, three[1].mix_hash, three[0].final_hash)])])
        assert conn.stats["bad_shares"] == 1
        # a newer job that came with clean_jobs false: shares of the old one are still welcome
        pool.peers[0].send(_notify("j2", header=bytes([0x22]) * 32, clean=False))
        _wait(lambda: conn.stats["jobs"] == 2, what="job 2")
        w2 = leader.next_work()
        assert w2.job_id != w1.job_id and w2.flags & FLAG_CLEAN and w2.header_hash == bytes([0x22]) * 32
        leader.on_results([(w1.job_id, 0, three[:1])])
        _wait(lambda: conn.stats["accepted"] == 4, what="the old job's share")
        assert got[-1]["params"][1] == "j1"
        # a clean job: whatever the old jobs still find is dropped
        pool.peers[0].send(_notify("j3", header=bytes([0x33]) * 32, clean=True))
        _wait(lambda: conn.stats["jobs"] == 3, what="job 3")
        w3 = leader.next_work()
        assert w3.flags & FLAG_CLEAN and w3.job_id not in (w1.job_id, w2.job_id)
        leader.on_results([(w1.job_id, 0, three[:2]), (w2.job_id, 0, three[2:])])
        assert conn.stats["stale_shares"] == 3 and conn.shares.empty() and conn.stats["submitted"] == 4
        # the same header under a new pool job id keeps the loop's job (and its cursor)
        pool.peers[0].send(_notify("j4", header=bytes([0x33]) * 32, clean=False, target=BLOCK_TARGET))
        _wait(lambda: conn.stats["jobs"] == 4, what="job 4")
        w4 = leader.next_work()
        assert w4.job_id == w3.job_id and not w4.flags & FLAG_CLEAN and w4.target() == BLOCK_TARGET
        assert len(got) == 4 and not pool.errors
    finally:
        conn.stop()
        pool.close()


def test_client_refuses_wrong_seed(core):
    def handler(i, p):
        _handshake(p, "0001")
        p.send(_notify("j1", seed=bytes([0xAB]) * 32))
        p.send(_notify("j2", seed=bytes([0xAB]) * 32))
        p.recv()

    pool = FakePool(handler)
    conn, leader = _client(pool.port)
    try:
        _wait(lambda: conn.stats["refused_jobs"] == 2, what="the refusals")
        assert leader.next_work().idle and conn.stats["jobs"] == 0 and len(conn._refused_seeds) == 1
    finally:
        conn.stop()
        pool.close()


def test_client_reconnects_with_a_new_extranonce(core, shares):
    close_first = threading.Event()
    got = {0: [], 1: []}

    def handler(i, p):
        _handshake(p, "0001" if i == 0 else "0002")
        p.send(_notify("j1"))
        if i == 0:
            close_first.wait(30)
            p.close()
            return
        while True:
            m = p.recv()
            if m is None:
                return
            got[i].append(m)

    pool = FakePool(handler)
    conn, leader = _client(pool.port)
    try:
        w1 = _work(leader)
        assert w1.nonce_base == 1 << 48
        close_first.set()
        _wait(lambda: conn.snapshot()[0] == 2, what="the reconnect")
        assert conn.stats["connects"] == 2 and conn.stats["disconnects"] == 1 and conn.snapshot()[1] == b"\x00\x02"
        # found under the old extranonce, handed over after the reconnect: never sent under the new one
        leader.on_results([(w1.job_id, 4096, shares["shares"][:1])])
        _wait(lambda: conn.stats["stale_shares"] == 1 and conn.shares.empty(), what="the drop")
        w2 = _work(leader)
        assert w2.nonce_base == 2 << 48 and w2.job_id != w1.job_id and w2.flags & 4
        leader.on_results([(w1.job_id, 4096, shares["shares"][:1])])
        assert conn.stats["stale_shares"] == 2 and conn.stats["submitted"] == 0
        assert got[1] == [] and len(pool.peers) == 2 and not pool.errors
    finally:
        conn.stop()
        pool.close()


def test_client_loop_never_waits_for_the_socket(core, shares):
    """A pool that stops reading: the connection thread blocks in its send, the loop's calls return."""
    from nodexa_chain_core_amd.miner import stratum as S

    release = threading.Event()

    def handler(i, p):
        _handshake(p, "0001")
        p.send(_notify("j1"))
        release.wait(60)  # never reads again

    pool = FakePool(handler)
    conn, leader = _client(pool.port, timeout=30.0)
    try:
        w = _work(leader)
        session, _x, _job, seq, _live = conn.snapshot()
        junk = S.Submit("w", "j1", 1 << 48, H, bytes(32))
        for _ in range(150_000):  # ~30 MB of submits: more than any loopback socket buffers
            conn.shares.put((session, seq, junk))
        conn.queue_share(session, seq, junk)
        last = [-1]

        def stuck():
            n, last[0] = last[0], conn.stats["submitted"]
            time.sleep(0.05)
            return n == last[0] and n > 0

        _wait(stuck, timeout=30, what="the connection thread to block in send")
        assert not conn.shares.empty()
        t0 = time.perf_counter()
        leader.on_results([(w.job_id, 4096, shares["shares"])])  # three full re-hashes, no I/O
        w2 = leader.next_work()
        dt = time.perf_counter() - t0
        assert dt < 1.0 and w2.job_id == w.job_id, dt
        assert not conn.shares.empty()  # still blocked
    finally:
        release.set()
        pool.close()
        conn.stop()


# ---------------------------------------------------------------------- 6. node end to end
def _rpc(port):
    from nodexa_chain_core_amd.rpc.client import RPCClient

    return RPCClient("127.0.0.1", port, "u", "p", timeout=30)


def _start_node(tmp_path, core, extra):
    addr = core.base58check_encode(bytes([42]) + bytes(range(20)))
    rpc_port, stratum_port = _free_port(), _free_port()
    env = dict(os.environ, PYTHONPATH=ROOT)
    node = subprocess.Popen([sys.executable, "-m", "nodexa_chain_core_amd.node", "-regtest", f"-datadir={tmp_path}",
                             f"-rpcport={rpc_port}", "-rpcuser=u", "-rpcpassword=p", f"-miningaddress={addr}",
                             "-listen=0", "-printtoconsole=0", f"-stratumport={stratum_port}", *extra], env=env)
    c = _rpc(rpc_port)

    def up():
        try:
            return c.getblockcount() == 0
        except (OSError, RuntimeError):
            assert node.poll() is None, "nodexad exited"
            return False

    _wait(up, timeout=120, what="the node's RPC")
    return node, c, stratum_port


def _stop_node(node, c):
    try:
        c.stop()
    except (OSError, RuntimeError):
        node.terminate()
    try:
        node.wait(timeout=60)
    except subprocess.TimeoutExpired:
        node.kill()


@pytest.mark.timeout(300)
def test_node_serves_a_miner_process(core, tmp_path):
    node, c, stratum_port = _start_node(tmp_path, core, [KAWPOW_REGTEST])
    trap = socket.socket()  # where the miner's RPC flags point: nothing may ever connect
    trap.bind(("127.0.0.1", 0))
    trap.listen(4)
    trap.setblocking(False)
    try:
        info = c.getstratuminfo()
        assert info["enabled"] and info["port"] == stratum_port and info["serving"] and info["algo"] == "kawpow"
        assert info["height"] == 1 and info["connections"] == [] and "getstratuminfo" in c.help()
        miner = subprocess.run([sys.executable, "-m", "nodexa_chain_core_amd.miner.remote", "-regtest", "-cpu",
                                "-minerwindow=64", f"-stratum=127.0.0.1:{stratum_port}", "-stratumuser=rig1", "-blocks=2",
                                f"-rpcport={trap.getsockname()[1]}", "-printtoconsole=0"],
                               env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
        assert miner.returncode == 0, miner.stdout + miner.stderr
        stats = ast.literal_eval(miner.stdout.strip().splitlines()[-1])
        assert stats["accepted"] >= 2 and stats["bad_shares"] == 0 and stats["lost"] == 0 and stats["jobs"] >= 2, stats
        with pytest.raises(BlockingIOError):
            trap.accept()  # no RPC connection at all: the jobs were pushed
        assert c.getblockcount() >= 2
        # the job of the next block is out although nobody asked for it
        _wait(lambda: c.getstratuminfo()["height"] == c.getblockcount() + 1, what="the pushed job")
        info = c.getstratuminfo()
        assert info["blocks_found"] >= 2 and info["accepted"] >= 2 and info["verified_host"] >= 2
        assert info["jobs_sent"] >= 3 and info["job"]["header_hash"] and info["verified_gpu"] == 0
        rig = [x for x in info["connections"] + info["recent_connections"] if x["user"] == "rig1"]
        assert len(rig) == 1 and rig[0]["accepted"] >= 2 and rig[0]["hashrate"] > 0 and rig[0]["last_share"] > 0, rig
        assert rig[0]["agent"].startswith("nodexa-miner") and len(rig[0]["extranonce"]) == 4
    finally:
        trap.close()
        _stop_node(node, c)


@pytest.mark.timeout(300)
def test_node_outside_the_kawpow_era_serves_nothing(core, tmp_path):
    node, c, stratum_port = _start_node(tmp_path, core, [])  # the regtest default: X16RV2
    p = Peer.connect(stratum_port)
    try:
        p.login()
        info = c.getstratuminfo()
        assert info["enabled"] and info["serving"] is False and info["algo"] == "x16rv2" and "note" in info
        assert len(info["connections"]) == 1  # the connection stays open
        assert p.call(3, "mining.subscribe", ["t"])["error"] is None
        assert not [n for n in p.notes if n.get("method") == "mining.notify"] and info["jobs_sent"] == 0
    finally:
        p.close()
        _stop_node(node, c)


def test_node_flag_errors(core, tmp_path):
    from nodexa_chain_core_amd.miner import remote
    from nodexa_chain_core_amd.node import Node
    from nodexa_chain_core_amd.utils.config import ArgsManager

    args = ArgsManager()
    args.parse_parameters(["-regtest", f"-datadir={tmp_path}", "-stratumport=0"])
    with pytest.raises(SystemExit, match="-miningaddress"):
        Node(args)
    with pytest.raises(SystemExit, match="-minerrank"):
        remote.main(["-cpu", "-stratum=127.0.0.1:1", "-minerrank=1"])
