"""The Stratum server's per-connection vardiff, its ban table and the owner of its share-check
DAGs, on the host: the rule as a table, the server against raw sockets with a `StaticJobSource`
and an injected clock, the pool client following retargets, and `EpochOwner` with a fake builder
and a fake registry.

Shares: tests/golden/stratum/vardiff_shares.json lists every nonce of two small ranges (prefixes
0001 and 0002, header 0x11..11, height 1) whose KawPow hash has two or more leading zero bits, with
that number ("bits"). The server hashes every one it is sent in full, so a wrong record cannot pass.
tests/golden/stratum/server_session_v0.jsonl is a session with the server as it was before vardiff
existed, the server's lines kept byte for byte."""
import json
import os
import socket
import threading

import pytest

from test_stratum import BLOCK_TARGET, GOLDEN, H, HEIGHT, Peer, _client, _wait, _work

LO = 2          # -stratumsharebits of these servers
PER_MINUTE = 1  # -stratumvardiff


class Clock:
    def __init__(self, t=1_000_000.0):
        self.t = t

    def __call__(self):
        return self.t


class Sh:
    def __init__(self, ent):
        self.nonce = int(ent["nonce"], 16)
        self.mix_hash = bytes.fromhex(ent["mix"])
        self.final_hash = bytes.fromhex(ent["final"])
        self.bits = ent["bits"]


@pytest.fixture(scope="module")
def easy():
    """{"0001": [Sh...], "0002": [...]}: the recorded shares, by nonce prefix."""
    with open(os.path.join(GOLDEN, "vardiff_shares.json")) as f:
        g = json.load(f)
    assert bytes.fromhex(g["header_hash"]) == H and g["height"] == HEIGHT
    out = {k: [Sh(e) for e in v] for k, v in g["shares"].items()}
    for v in out.values():
        assert all(256 - int.from_bytes(s.final_hash, "big").bit_length() == s.bits >= LO for s in v)
    return out


def _target(bits):
    return (1 << (256 - bits)) - 1


def _job(job_id, clean=True, tip="tipA", height=HEIGHT, block_target=BLOCK_TARGET):
    from nodexa_chain_core_amd.miner.stratum_server import ServerJob

    return ServerJob(job_id, H, height, block_target, 0x1D00FFFF, clean, tip)


@pytest.fixture()
def server(core):
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    made = []

    def make(**kw):
        src = StaticJobSource()
        kw.setdefault("share_bits", LO)
        srv = StratumServer(src, **kw).start()
        made.append(srv)
        return srv, src

    yield make
    for srv in made:
        srv.stop()


def _next_note(p):
    """The next notification, from those `call` put aside or from the socket."""
    return p.notes.pop(0) if p.notes else p.recv()


# ---------------------------------------------------------------------- 1. the rule
def test_vardiff_rule_table():
    from nodexa_chain_core_amd.miner.stratum import vardiff_next_bits as nb

    m = 60000
    # (bits, shares, elapsed_ms, per_minute, lo, hi) -> bits; at 6 per minute one minute wants 6 shares
    table = [
        ((10, 12, m, 6, 8, 255), 11),        # ratio exactly 2: one bit harder
        ((10, 12, m + 1, 6, 8, 255), 10),    # one unit below 2 (E grew by 6): unchanged
        ((10, 12, m - 1, 6, 8, 255), 11),    # one unit above 2
        ((10, 11, m, 6, 8, 255), 10),
        ((10, 24, m, 6, 8, 255), 12),        # ratio 4
        ((10, 24, m + 1, 6, 8, 255), 11),    # just below 4
        ((10, 3, m, 6, 8, 255), 9),          # ratio exactly 1/2: one bit easier
        ((10, 3, m - 1, 6, 8, 255), 10),     # one unit above 1/2: unchanged
        ((10, 3, m + 1, 6, 8, 255), 9),      # one unit below 1/2
        ((10, 4, m, 6, 8, 255), 10),
        ((10, 6, m, 6, 8, 255), 10),         # on the wanted rate
        ((20, 96, m, 6, 8, 255), 24),        # ratio 16: 4 bits
        ((20, 96, m + 1, 6, 8, 255), 23),    # just below 16
        ((20, 192, m, 6, 8, 255), 24),       # ratio 32: capped at 4
        ((20, 10 ** 9, m, 6, 8, 255), 24),
        ((20, 1, 10 * m, 6, 8, 255), 16),    # ratio 1/60: capped at 4
        ((20, 1, 2 * m, 6, 8, 255), 17),     # ratio 1/12: floor(log2 12) = 3
        ((20, 0, m, 6, 8, 255), 16),         # no share at all counts as the full 4
        ((20, 0, 1, 6, 8, 255), 16),
        ((9, 0, m, 6, 8, 255), 8),           # the lower clamp: -stratumsharebits
        ((8, 0, m, 6, 8, 255), 8),
        ((8, 3, m, 6, 8, 255), 8),
        ((253, 192, m, 6, 8, 255), 255),     # the upper clamp
        ((255, 12, m, 6, 8, 255), 255),
        ((30, 192, m, 6, 8, 32), 32),
        ((10, 12, 0, 6, 8, 255), 10),        # no time passed: nothing was measured
        ((10, 0, 0, 6, 8, 255), 10),
        # elapsed_ms beyond 2^53, where a float rounds: with 60000 per minute S >= 2E is shares >= 2 * elapsed_ms
        ((10, 2 ** 54 + 2, 2 ** 53 + 1, 60000, 8, 255), 11),
        ((10, 2 ** 54 + 1, 2 ** 53 + 1, 60000, 8, 255), 10),  # float(2^53 + 1) == 2^53 would say "twice": it is not
        ((10, 2 ** 52, 2 ** 53 + 1, 60000, 8, 255), 9),       # 2 * shares = elapsed_ms - 1: half, and a unit to spare
        ((10, 2 ** 52 + 1, 2 ** 53 + 1, 60000, 8, 255), 10),  # 2 * shares = elapsed_ms + 1: not half
    ]
    for args, want in table:
        assert nb(*args) == want, (args, nb(*args), want)
    assert float(2 ** 53 + 1) == float(2 ** 53)  # why that row needs integers
    with pytest.raises(ValueError):
        nb(10, -1, m, 6, 8, 255)


# ---------------------------------------------------------------------- 2. the server, raw sockets
def test_vardiff_server_session(server, easy):
    from nodexa_chain_core_amd.miner.stratum_server import share_work

    clk = Clock()
    t0 = clk.t
    srv, src = server(vardiff=PER_MINUTE, clock=clk)
    src.push(_job("j1"))
    p = Peer.connect(srv.port)
    q = None
    mine = easy["0001"]
    try:
        p.login()
        a, b = _next_note(p), _next_note(p)
        assert (a["method"], a["params"]) == ("mining.set_target", ["%064x" % _target(LO)])
        assert b["method"] == "mining.notify" and b["params"][0] == "j1" and b["params"][3] == "%064x" % _target(LO)
        # 4 shares in 30 s where 1 a minute is wanted: 8 times the rate
        burst = mine[:4]
        for i, s in enumerate(burst):
            clk.t = t0 + 5 * (i + 1)
            assert p.submit(10 + i, "j1", s)["result"] is True
        clk.t = t0 + 30
        assert p.call(20, "mining.subscribe", ["again"])["error"] is None
        assert p.notes == []  # no target and no job came by themselves, although a retarget is due
        assert srv.info()["connections"][0]["share_bits"] == LO
        # the next job brings the harder target: set_target immediately in front of its notify
        src.push(_job("j2", clean=False))
        a, b = _next_note(p), _next_note(p)
        hard = LO + 3  # S / E = 4 * 60000 / (1 * 30000) = 8
        assert a == {"id": None, "method": "mining.set_target", "params": ["%064x" % _target(hard)]}
        assert b["method"] == "mining.notify" and b["params"][0] == "j2" and b["params"][3] == "%064x" % _target(hard)
        assert b["params"][4] is False
        # a share of the previous job is judged at the previous target; the same share of the new job is too high
        weak = next(s for s in mine[4:] if s.bits < hard)
        strong = next(s for s in mine[4:] if s.bits >= hard)
        assert p.submit(30, "j1", weak)["result"] is True
        assert p.submit(31, "j2", weak)["error"][0] == 23
        assert p.submit(32, "j2", strong)["result"] is True
        assert p.submit(33, "j0", strong)["error"][0] == 21  # a job this connection was never sent
        # a second connection starts at the easiest target while the first holds the harder one
        q = Peer.connect(srv.port)
        q.login()
        a, b = _next_note(q), _next_note(q)
        assert (a["method"], a["params"]) == ("mining.set_target", ["%064x" % _target(LO)])
        assert b["method"] == "mining.notify" and b["params"][0] == "j2" and b["params"][3] == "%064x" % _target(LO)
        qs = easy["0002"][0]
        assert qs.bits < hard and q.submit(3, "j2", qs)["result"] is True  # too high for p, good for q
        assert q.submit(4, "j1", qs)["error"][0] == 21                      # j1 never went to q
        info = srv.info()
        by_id = {c["id"]: c for c in info["connections"]}
        assert info["vardiff"] == PER_MINUTE
        assert (by_id[1]["share_bits"], by_id[1]["retargets"]) == (hard, 1)
        assert (by_id[2]["share_bits"], by_id[2]["retargets"]) == (LO, 0)
        # hashrate: the summed work of the window, each share at the target it was judged by
        work = 5 * share_work(_target(LO)) + share_work(_target(hard))
        assert by_id[1]["accepted"] == 6 and by_id[1]["hashrate"] == round(work / 30.0, 3)
        assert by_id[1]["shares_per_minute"] == 12.0
        assert by_id[2]["hashrate"] == round(share_work(_target(LO)) / 1e-3, 3)  # connected for no time at all
        # silence: 2 shares since the retarget, and 1000 s want 16.7: E / S = 8.3, three bits easier. No job went
        # out for 60 s, so the current one comes again, not clean, with that target
        clk.t = t0 + 30 + 1000
        a, b = _next_note(p), _next_note(p)  # the job thread looks every half second
        easier = hard - 3
        assert a == {"id": None, "method": "mining.set_target", "params": ["%064x" % _target(easier)]}
        assert b["method"] == "mining.notify" and b["params"][0] == "j2" and b["params"][4] is False
        assert b["params"][3] == "%064x" % _target(easier)
        # j2 went to p twice: the easier target judges its shares from now on
        assert p.submit(40, "j2", weak)["result"] is True
        info = srv.info()
        by_id = {c["id"]: c for c in info["connections"]}
        assert (by_id[1]["share_bits"], by_id[1]["retargets"]) == (easier, 2)
        assert by_id[2]["retargets"] == 0 and q.notes == []  # q, at the easiest target already, got nothing
        assert info["accepted"] == 8 and info["verified_host"] == 8
    finally:
        p.close()
        if q is not None:
            q.close()


def test_flag_off_session_is_byte_identical(server):
    """Every line the server sends in the recorded session, byte for byte, with no new flag set."""
    from nodexa_chain_core_amd.miner.stratum_server import ServerJob

    with open(os.path.join(GOLDEN, "server_session_v0.jsonl")) as f:
        script = [json.loads(line) for line in f if line.strip()]
    srv, src = server(share_bits=8)
    s = socket.create_connection(("127.0.0.1", srv.port), timeout=20)
    f = s.makefile("rb")
    try:
        for n, ent in enumerate(script):
            if ent["dir"] == "push":
                j = ent["job"]
                src.push(ServerJob(j["job_id"], bytes.fromhex(j["header_hash"]), j["height"], int(j["block_target"], 16),
                                   int(j["bits"], 16), j["clean"], j["tip"]))
            elif ent["dir"] == "c2s":
                s.sendall(ent["raw"].encode())
            else:
                assert f.readline() == ent["raw"].encode(), f"line {n + 1}"
    finally:
        s.close()
    assert sum(e["dir"] == "s2c" for e in script) == 16
    info = srv.info()
    assert info["vardiff"] == 0 and info["verified_host"] == 4 and "dag_builds" not in info


def test_vardiff_needs_share_bits(core, tmp_path):
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer
    from nodexa_chain_core_amd.node import Node
    from nodexa_chain_core_amd.utils.config import ArgsManager

    with pytest.raises(ValueError, match="share bits"):
        StratumServer(StaticJobSource(), share_bits=0, vardiff=6)
    addr = core.base58check_encode(bytes([42]) + bytes(range(20)))
    for flags, what in ((["-stratumvardiff=6"], "-stratumsharebits"), (["-stratumvardiff=-1"], "-stratumvardiff"),
                        (["-stratumgpuverify=2"], "-stratumgpuverify"), (["-stratumbantime=-5"], "-stratumbantime")):
        args = ArgsManager()
        args.parse_parameters(["-regtest", f"-datadir={tmp_path}", "-stratumport=0", f"-miningaddress={addr}"] + flags)
        node = Node.__new__(Node)  # the flag checks come before anything of the node is used
        node.gpus, node.mining_script, node.miner = [], b"\x51", None
        with pytest.raises(SystemExit, match=what):
            node._start_stratum(args)


# ---------------------------------------------------------------------- 3. the client follows
def test_client_follows_two_retargets(core):
    """The pool client on a host device against the vardiff server: a harder target, then an easier
    one, each arriving with a job; every share the client submits is accepted."""
    from nodexa_chain_core_amd.miner.search import CpuSearchDevice
    from nodexa_chain_core_amd.miner.service import MiningService
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    clk = Clock()
    src = StaticJobSource()
    srv = StratumServer(src, share_bits=LO, vardiff=4, clock=clk).start()
    src.push(_job("j1"))
    conn, leader = _client(srv.port)
    svc = MiningService(CpuSearchDevice(max_window=16), leader, window=16, idle_sleep_s=0.0)

    def mine_until(n, what):
        def step():
            svc.step()
            return conn.stats["accepted"] >= n
        _wait(step, timeout=60, what=what)
        _wait(lambda: conn.shares.empty() and conn.stats["accepted"] + conn.stats["rejected"] == conn.stats["submitted"],
              what="every answer")

    def bits():
        c = srv.info()["connections"][0]
        return c["share_bits"], c["retargets"]

    try:
        assert _work(leader).target() == _target(LO)
        mine_until(8, "8 shares at the first target")
        n1 = conn.stats["accepted"]
        assert bits() == (LO, 0)
        # n1 >= 8 shares in 30 s where 2 are wanted: at least 2 bits harder, with the next job
        clk.t += 30
        src.push(_job("j2", clean=False))
        _wait(lambda: conn.stats["jobs"] == 2, what="job 2")
        b1, r1 = bits()
        assert r1 == 1 and LO + 2 <= b1 <= LO + 4
        _wait(lambda: leader.next_work().target() == _target(b1), what="the harder target at the loop")
        mine_until(n1 + 1, "a share at the harder target")
        # 5 minutes want 20 shares; the few there were make it easier again
        assert conn.stats["accepted"] - n1 <= 10
        clk.t += 300
        src.push(_job("j3", clean=False))
        _wait(lambda: conn.stats["jobs"] == 3, what="job 3")
        b2, r2 = bits()
        assert r2 == 2 and LO <= b2 < b1
        _wait(lambda: leader.next_work().target() == _target(b2), what="the easier target at the loop")
        n2 = conn.stats["accepted"]
        mine_until(n2 + 2, "shares at the easier target")
        st = dict(conn.stats)
        assert st["rejected"] == 0 and st["bad_shares"] == 0 and st["lost"] == 0 and st["accepted"] == st["submitted"], st
        assert srv.stats["rejected"] == 0 and srv.stats["accepted"] == st["accepted"]
    finally:
        conn.stop()
        srv.stop()
        leader.shutdown()
        while svc.step():
            pass


# ---------------------------------------------------------------------- 4. the ban table
def test_ban_table_rule():
    from nodexa_chain_core_amd.miner.stratum_server import BAN_TABLE_MAX, BanTable

    t = BanTable(100.0)
    assert not t.strike("a", 0) and not t.strike("a", 10) and t.banned_until("a", 11) == 0.0
    assert t.strike("a", 599)                      # the third inside 10 minutes
    assert t.banned_until("a", 600) == 699 and t.banned_until("a", 698.9) == 699
    assert t.banned_until("a", 699) == 0.0 and len(t) == 0   # expired, and forgotten
    # two strikes, and a third only after the window has passed the first two: no ban
    assert not t.strike("b", 0) and not t.strike("b", 1) and not t.strike("b", 601.5)
    assert t.banned_until("b", 602) == 0.0
    assert not t.strike("b", 700) and t.strike("b", 1201)  # 601.5, 700, 1201 are within 600 s
    assert t.banned_until("b", 1202) == 1301
    # bounded: the oldest addresses go, bans included
    for i in range(BAN_TABLE_MAX + 10):
        t.strike("x%d" % i, 1300)
    assert len(t) == BAN_TABLE_MAX and t.banned_until("b", 1300.5) == 0.0
    assert not t.strike("x0", 1300) and not t.strike("x0", 1300)  # x0 was dropped: these are its 1st and 2nd again


def _forged(core, nonce, target, k0):
    k = k0
    while True:  # a mix that passes the cheap check for this nonce and is not the real one
        mix = core.sha256d(b"forged mix %d" % k)
        k += 1
        if int.from_bytes(core.kawpow_hash_no_verify(HEIGHT, H, mix, nonce), "big") <= target:
            return mix


def test_ban_at_accept(server, core):
    clk = Clock()
    srv, src = server(ban_s=120, clock=clk)
    src.push(_job("j1"))
    for i in range(3):
        p = Peer.connect(srv.port)
        try:
            p.login()
            assert srv.info()["connections"][0]["extranonce"] == "%04x" % (i + 1)
            nonce = ((i + 1) << 48) + 99
            r = p.submit(3, "j1", type("F", (), {"nonce": nonce, "mix_hash": _forged(core, nonce, _target(LO), i * 1000)}))
            assert r["error"][0] == 20 and "mix" in r["error"][1] and p.recv() is None
        finally:
            p.close()
        _wait(lambda: not srv.info()["connections"], what="the close")
        clk.t += 60
    assert srv.stats["refused_connections"] == 0
    p = Peer.connect(srv.port)
    try:
        assert p.recv() is None  # refused at accept
    finally:
        p.close()
    info = srv.info()
    last = info["recent_connections"][-1]
    assert info["refused_connections"] == 1 and last["refused"] and last["address"].startswith("127.0.0.1:")
    assert last["banned_until"] == int(clk.t - 60 + 120)
    clk.t += 61  # the ban has run out
    p = Peer.connect(srv.port)
    try:
        p.login()
        assert srv.info()["connections"][0]["extranonce"] == "0004" and srv.stats["refused_connections"] == 1
    finally:
        p.close()


# ---------------------------------------------------------------------- 5. the epoch owner
class FakeRegistry:
    def __init__(self):
        self.d = {}
        self.lock = threading.Lock()

    def is_resident(self, device, epoch):
        with self.lock:
            return (device, epoch) in self.d

    def register(self, device, epoch, e):
        with self.lock:
            self.d.setdefault((device, epoch), e)
            return self.d[(device, epoch)] is e

    def drop(self, device, epoch, e):
        with self.lock:
            if self.d.get((device, epoch)) is e:
                del self.d[(device, epoch)]
                return True
            return False

    def resident(self, device):
        with self.lock:
            return [e for d, e in self.d if d == device]


class FakeBuilder:
    def __init__(self, fail=()):
        self.gate = threading.Event()
        self.started = []
        self.lights = []
        self.running = 0
        self.max_running = 0
        self.fail = set(fail)
        self.lock = threading.Lock()

    def light(self, epoch):
        self.lights.append(epoch)

    def build(self, epoch):
        with self.lock:
            self.started.append(epoch)
            self.running += 1
            self.max_running = max(self.max_running, self.running)
        try:
            assert self.gate.wait(20)
            if epoch in self.fail:
                raise RuntimeError("no memory for epoch %d" % epoch)
            return ("dag", epoch)
        finally:
            with self.lock:
                self.running -= 1


def _owner(fail=(), foreign=None):
    from nodexa_chain_core_amd.miner.stratum_epochs import EpochOwner

    reg, b = FakeRegistry(), FakeBuilder(fail)
    return EpochOwner(0, b, registry=reg, foreign_pending=foreign), reg, b


def test_owner_builds_one_at_a_time(core):
    E = core.EPOCH_LENGTH
    own, reg, b = _owner()
    try:
        own.note_job(3 * E - 1)  # epoch 2, one block before the boundary: 2 and 3 are wanted
        _wait(lambda: b.started == [2], what="the first build")
        assert own.mode(2) == "light" and own.mode(3) == "host" and not own.ready(2) and not own.idle()
        for _ in range(5):  # asking again starts nothing
            own.note_job(3 * E - 1)
        assert b.started == [2] and b.running == 1
        b.gate.set()
        _wait(own.idle, what="both builds")
        assert b.started == [2, 3] and b.max_running == 1 and b.lights == [2, 3]
        assert own.mode(2) == own.mode(3) == "dag" and own.own_epochs() == [2, 3]
        info = own.info()
        assert info["dag_builds"] == 2 and info["dag_build_failures"] == 0 and info["epochs_resident"] == [2, 3]
        assert info["dag_last_build_ms"] >= 0
    finally:
        b.gate.set()
        own.stop()


def test_owner_lookahead_edge(core):
    E = core.EPOCH_LENGTH
    own, reg, b = _owner()
    b.gate.set()
    try:
        own.note_job(E - 121)
        _wait(own.idle, what="the build")
        assert b.started == [0]
        own.note_job(E - 120)
        _wait(lambda: own.idle() and own.ready(1), what="the next epoch")
        assert b.started == [0, 1]
    finally:
        own.stop()


def test_owner_leaves_foreign_epochs_alone(core):
    E = core.EPOCH_LENGTH
    pending = {6}
    own, reg, b = _owner(foreign=lambda e: e in pending)
    b.gate.set()
    try:
        miner4, miner5 = ("miner", 4), ("miner", 5)
        reg.register(0, 4, miner4)   # the "miner" shared epochs 4 and 5, and is prebuilding 6
        reg.register(0, 5, miner5)
        own.note_job(5 * E - 1)      # 4 and 5 wanted: both resident
        own.note_job(6 * E - 1)      # 5 resident, 6 being prebuilt elsewhere
        assert own.idle() and b.started == [] and own.mode(4) == "dag" and own.mode(6) == "host"
        # eviction: the owner builds 7, 8, 9 in turn and keeps its last two; the miner's stay
        for e in (7, 8, 9):
            own.note_job(e * E)
            _wait(lambda: own.idle() and own.ready(e), what=f"epoch {e}")
        assert b.started == [7, 8, 9] and own.own_epochs() == [8, 9]
        assert sorted(reg.resident(0)) == [4, 5, 8, 9] and reg.d[(0, 4)] is miner4 and reg.d[(0, 5)] is miner5
        # the miner's DAG took an epoch's place while the owner built it: not the owner's to drop
        own.failed.clear()
        reg.d[(0, 10)] = ("miner", 10)
        own.wanted.append(10)
        pending.clear()
        own._build(10)
        assert own.own_epochs() == [8, 9] and reg.d[(0, 10)] == ("miner", 10)
    finally:
        own.stop()


def test_owner_failing_builder(core, server, easy, monkeypatch):
    from nodexa_chain_core_amd.miner import stratum_epochs

    logged = []
    monkeypatch.setattr(stratum_epochs.log, "log_printf", logged.append)
    own, reg, b = _owner(fail={0})
    b.gate.set()
    srv, src = server(device=0, epoch_owner=own)
    src.push(_job("j1"))
    p = Peer.connect(srv.port)
    try:
        _wait(lambda: b.started == [0] and own.idle(), what="the failed build")
        for _ in range(3):
            own.note_job(5)
        assert own.idle() and b.started == [0]  # not tried again
        assert own.mode(0) == "host" and own.info()["dag_build_failures"] == 1 and own.info()["dag_builds"] == 0
        p.login()
        assert p.submit(3, "j1", easy["0001"][0])["result"] is True  # the host path works
        info = srv.info()
        assert info["verified_host"] == 1 and info["verified_gpu"] == 0 and info["verified_gpu_light"] == 0
        assert info["dag_build_failures"] == 1 and info["epochs_resident"] == []
    finally:
        p.close()
    srv.stop()
    assert len([m for m in logged if "building the epoch 0 DAG" in m and "no memory for epoch 0" in m]) == 1
