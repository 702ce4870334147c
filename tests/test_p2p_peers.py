"""Connection slots, inbound eviction, keep-alive / inactivity timeouts and the outbound eviction
rules (net/peerman.py, ConnectionManager.maintain). Protocol timeouts are crossed on a mock clock;
the only real waits are bounded polls for socket events."""
import struct
import threading

from nodexa_chain_core_amd.net import protocol as P
from p2p_script import MockClock, ScriptedPeer, ScriptedServer, node_peer, wait
from test_p2p import _node

# ------------------------------------------------------------------ 1. the selection, pure
def select_node_to_evict(candidates):
    from nodexa_chain_core_amd.net import peerman

    return peerman.select_node_to_evict(candidates)


# ids 1-4:   the four highest keyed net groups                    -> protected by rule 1
# ids 5-12:  the eight lowest minimum pings                       -> protected by rule 2
# ids 13-16: the only ones with a transaction, the newest four    -> protected by rule 3
# ids 17-20: the only ones with a block, the newest four          -> protected by rule 4
# ids 21...: the rest, connected at 1000 + id (21 is the oldest); their net groups vary per case.
# ids 1-20 connected later than all of them, so rule 5 (age) could never be what saves those.


def _candidates(rest_groups):
    from nodexa_chain_core_amd.net.peerman import EvictionCandidate as C

    out = []
    for i in range(1, 5):
        out.append(C(i, 2000 + i, 5.0, 0, 0, True, True, False, 9000 + i))
    for i in range(5, 13):
        out.append(C(i, 2000 + i, 0.001 * i, 0, 0, True, True, False, 1))
    for i in range(13, 17):
        out.append(C(i, 2000 + i, 2.0, 0, 100 + i, True, True, False, 2))
    for i in range(17, 21):
        out.append(C(i, 2000 + i, 2.0, 100 + i, 0, True, True, False, 3))
    for k, g in enumerate(rest_groups):
        out.append(C(21 + k, 1021 + k, 2.0, 0, 0, True, True, False, g))
    return out


def test_eviction_protects_up_to_twenty():
    full = _candidates([1, 1, 1, 1])
    for n in (0, 1, 4, 5, 12, 13, 16, 20):
        assert select_node_to_evict(full[:n]) is None, n
    # the 21st has no protection left: 4 + 8 + 4 + 4 are taken, and half of one is none
    assert select_node_to_evict(full[:21]) == 21


def test_eviction_youngest_of_largest_group():
    # 24 candidates: rules 1-4 leave 21-24, rule 5 protects the older two (21, 22); 23 and 24
    # share a net group, and 24 is its youngest
    assert select_node_to_evict(_candidates([1, 2, 7, 7])) == 24
    # the order of the records must not matter
    assert select_node_to_evict(list(reversed(_candidates([1, 2, 7, 7])))) == 24
    # 28 candidates: rules 1-4 leave 21-28, rule 5 protects 21-24; of 25-28 three are in group 7
    # and the youngest of all (28) is alone in group 8: the largest group loses its youngest, 27
    assert select_node_to_evict(_candidates([1, 1, 1, 1, 7, 7, 7, 8])) == 27
    # ... wherever the lone one stands
    assert select_node_to_evict(_candidates([1, 1, 1, 1, 8, 7, 7, 7])) == 28


def test_eviction_tie_between_equal_groups():
    # 25, 28 in group 7 and 26, 27 in group 8: equal sizes, group 7 has the younger newest member
    assert select_node_to_evict(_candidates([1, 1, 1, 1, 7, 8, 8, 7])) == 28
    # 25, 26 in group 7 and 27, 28 in group 8: now group 8 has it
    assert select_node_to_evict(_candidates([1, 1, 1, 1, 7, 7, 8, 8])) == 28
    # seven left after rules 1-4 (21-27): rule 5 protects the older three, leaving 24 in group 1,
    # 25 and 27 in group 8 and 26 in group 7: 27 is the youngest of the larger group
    assert select_node_to_evict(_candidates([1, 1, 1, 1, 8, 7, 8])) == 27
    # again seven: 24, 25 in group 7 and 26, 27 in group 8 tie, and group 8 has the younger newest
    assert select_node_to_evict(_candidates([1, 1, 1, 7, 7, 8, 8])) == 27


# ------------------------------------------------------------------ 9. -maxconnections
def test_connection_slots_arithmetic():
    from nodexa_chain_core_amd.net.peerman import connection_slots

    assert connection_slots(20, 8) == (8, 11)
    assert connection_slots(4, 8) == (4, 0)
    assert connection_slots(125, 8) == (8, 116)
    assert connection_slots(0, 8) == (0, 0)


def test_maxconnections_flag(core, tmp_path):
    for name, extra, want in (("m20", ["-maxconnections=20"], (8, 11)), ("m4", ["-maxconnections=4"], (4, 0)),
                              ("dflt", [], (8, 116))):
        n = _node(core, tmp_path, name, ["-listen", "-port=0", *extra])
        try:
            assert (n.connman.max_outbound, n.connman.max_inbound) == want
        finally:
            n.stop()
    # -connect still means no automatic outbound connections
    n = _node(core, tmp_path, "conn", ["-listen", "-port=0", "-connect=127.0.0.1:1"])
    try:
        assert n.connman.connect_only
        assert not any(t.name == "p2p-opencon" for t in threading.enumerate())
    finally:
        n.stop()


# ------------------------------------------------------------------ 2. the inbound limit, live
def _inbound(node):
    return [p for p in list(node.connman.peers) if p.inbound and not p.closed.is_set()]


def test_inbound_limit_refuses_when_all_protected(core, tmp_path):
    a = _node(core, tmp_path, "a", ["-listen", "-port=0", "-maxconnections=12"])
    peers = []
    try:
        assert a.connman.max_inbound == 3
        magic = bytes(a.params.message_start)
        peers = [ScriptedPeer.dial(a.connman.port, magic) for _ in range(3)]
        assert wait(lambda: a.peer_count() == 3)
        # three candidates, all within the four that the net-group rule protects: nobody can go
        fourth = ScriptedPeer.dial(a.connman.port, magic, handshake=False)
        peers.append(fourth)
        assert fourth.closed.wait(10), "the fourth connection was not closed by the node"
        assert not any(p.closed.is_set() for p in peers[:3])
        assert a.peer_count() == 3 and len(_inbound(a)) == 3
    finally:
        for p in peers:
            p.close()
        a.stop()


def test_inbound_limit_evicts_one_and_spares_whitelisted(core, tmp_path):
    a = _node(core, tmp_path, "a", ["-listen", "-port=0", "-maxconnections=33"])
    peers = []
    try:
        assert a.connman.max_inbound == 24
        magic = bytes(a.params.message_start)
        for _ in range(24):
            peers.append(ScriptedPeer.dial(a.connman.port, magic))
        assert wait(lambda: a.peer_count() == 24)
        # the two youngest are whitelisted (as a -whitebind socket marks its peers): with one net
        # group among all of them, youth is what the last rule picks by, so these would be first
        white = peers[-2:]
        for w in white:
            node_peer(a, w).whitebind = True
        newcomer = ScriptedPeer.dial(a.connman.port, magic)
        assert wait(lambda: sum(p.closed.is_set() for p in peers) == 1 and a.peer_count() == 24)
        assert not newcomer.closed.is_set()
        assert not any(w.closed.is_set() for w in white)
        assert len(_inbound(a)) == 24
        peers.append(newcomer)
    finally:
        for p in peers:
            p.close()
        a.stop()


# ------------------------------------------------------------------ 3. timeouts, mock clock
def _clocked_node(core, tmp_path, name="a", extra=()):
    n = _node(core, tmp_path, name, ["-listen", "-port=0", *extra])
    clock = MockClock()
    n.connman.set_clock(clock)
    return n, clock


def test_silent_socket_dropped_after_a_minute(core, tmp_path):
    a, clock = _clocked_node(core, tmp_path)
    try:
        s = ScriptedPeer.dial(a.connman.port, bytes(a.params.message_start), handshake=False)  # never says version
        assert wait(lambda: len(a.connman.peers) == 1)
        np = a.connman.peers[0]
        clock.advance(60)
        a.connman.maintain()
        assert not np.closed.is_set()
        clock.advance(1)
        a.connman.maintain()
        assert np.closed.is_set() and s.closed.wait(10)
        assert wait(lambda: len(a.connman.peers) == 0)
    finally:
        a.stop()


def test_unanswered_ping_times_out_at_1200(core, tmp_path):
    a, clock = _clocked_node(core, tmp_path)
    try:
        s = ScriptedPeer.dial(a.connman.port, bytes(a.params.message_start), answer_pings=False)
        assert wait(lambda: a.peer_count() == 1)
        np = node_peer(a, s)
        a.connman.maintain()  # the first pass after the handshake sends the first ping
        assert wait(lambda: s.count("ping") == 1)
        (nonce,) = struct.unpack("<Q", s.payloads("ping")[0])
        assert nonce != 0 and nonce == np.ping_nonce
        clock.advance(1199)
        a.connman.maintain()
        assert not np.closed.is_set()
        assert s.count("ping") == 1  # one ping at a time
        info = a.table.execute("getpeerinfo", [])[0]
        assert info["pingwait"] == 1199 and "pingtime" not in info and "minping" not in info
        clock.advance(1)
        a.connman.maintain()
        assert np.closed.is_set() and s.closed.wait(10)
    finally:
        a.stop()


def test_pong_records_pingtime(core, tmp_path):
    a, clock = _clocked_node(core, tmp_path)
    try:
        s = ScriptedPeer.dial(a.connman.port, bytes(a.params.message_start))
        assert wait(lambda: a.peer_count() == 1)
        np = node_peer(a, s)
        a.connman.maintain()
        assert wait(lambda: np.ping_time is not None)
        info = a.table.execute("getpeerinfo", [])[0]
        assert info["pingtime"] == 0 and info["minping"] == 0 and "pingwait" not in info
        assert info["synced_headers"] == -1 and info["synced_blocks"] == -1 and info["inflight"] == []
        # the next ping goes out 120 s after the last one began, and not before
        clock.advance(120)
        a.connman.maintain()
        assert np.ping_nonce == 0 and s.count("ping") == 1
        clock.advance(1)
        a.connman.maintain()
        assert wait(lambda: s.count("ping") == 2)
    finally:
        a.stop()


def test_bad_pongs_are_ignored_without_ban_score(core, tmp_path):
    a, clock = _clocked_node(core, tmp_path)
    try:
        s = ScriptedPeer.dial(a.connman.port, bytes(a.params.message_start), answer_pings=False)
        assert wait(lambda: a.peer_count() == 1)
        np = node_peer(a, s)
        a.connman.maintain()
        assert wait(lambda: s.count("ping") == 1)
        (nonce,) = struct.unpack("<Q", s.payloads("ping")[0])
        for k, bad in enumerate((struct.pack("<Q", nonce ^ 1), struct.pack("<Q", 0), b"\x01\x02\x03")):
            s.send("pong", bad)
            s.send("ping", struct.pack("<Q", 77 + k))  # the node's pong to this one shows it has read the bad one
            assert wait(lambda: s.count("pong") == k + 1)
            info = a.table.execute("getpeerinfo", [])[0]
            assert "pingwait" in info and "pingtime" not in info and info["banscore"] == 0
            assert np.ping_nonce == nonce and not np.closed.is_set()
        s.send("pong", struct.pack("<Q", nonce))  # the right one still ends it
        assert wait(lambda: np.ping_nonce == 0 and np.ping_time is not None)
    finally:
        a.stop()


def test_ping_rpc_reaches_every_peer(core, tmp_path):
    a, clock = _clocked_node(core, tmp_path)
    try:
        magic = bytes(a.params.message_start)
        peers = [ScriptedPeer.dial(a.connman.port, magic) for _ in range(3)]
        assert wait(lambda: a.peer_count() == 3)
        a.connman.maintain()
        assert wait(lambda: all(p.ping_time is not None and p.ping_nonce == 0 for p in a.connman.peers))
        assert [s.count("ping") for s in peers] == [1, 1, 1]
        a.table.execute("ping", [])  # no time has passed: only the RPC can be why these go out
        assert wait(lambda: [s.count("ping") for s in peers] == [2, 2, 2])
    finally:
        a.stop()


# ------------------------------------------------------------------ 8. outbound management, mock clock
def _announce(node, s, clock):
    """The scripted peer announces a block (an inv of the genesis hash, a header the node knows)."""
    pid = node_peer(node, s).id
    s.send("inv", P.inv_payload([(P.MSG_BLOCK, node.state.chain.genesis().hash)]))
    assert wait(lambda: node.connman.fetcher.last_block_announcement(pid) == clock.t)


def test_extra_outbound_peer_evicted(core, tmp_path):
    b, clock = _clocked_node(core, tmp_path, "b")
    servers = []
    try:
        cm = b.connman
        cm.max_outbound = 2
        b.miner.generate(b.mining_script, 1)  # above genesis, so announcing genesis earns no protection
        magic = bytes(b.params.message_start)
        servers = [ScriptedServer(magic) for _ in range(3)]
        t0 = clock.t
        cm.maintain()  # the 45 s rhythm starts here
        s1 = (cm.connect("127.0.0.1", servers[0].port), servers[0].accept())[1]
        s2 = (cm.connect("127.0.0.1", servers[1].port), servers[1].accept())[1]
        assert wait(lambda: b.peer_count() == 2)
        clock.t = t0 + 5
        _announce(b, s1, clock)
        clock.t = t0 + 10
        _announce(b, s2, clock)
        clock.t = t0 + 20
        s3 = (cm.connect("127.0.0.1", servers[2].port), servers[2].accept())[1]
        assert wait(lambda: b.peer_count() == 3)
        clock.t = t0 + 44
        cm.maintain()
        assert b.peer_count() == 3  # not yet time for the check
        clock.t = t0 + 45
        cm.maintain()
        # the check ran and chose s3 (it never announced a block), which is only 25 s old: kept
        assert b.peer_count() == 3 and not any(p.closed.is_set() for p in cm.peers)
        clock.t = t0 + 50
        _announce(b, s3, clock)
        clock.t = t0 + 60
        _announce(b, s1, clock)
        clock.t = t0 + 90
        cm.maintain()
        # now s2's announcement (t0 + 10) is the oldest, and s2 is old enough
        assert s2.closed.wait(10)
        assert wait(lambda: b.peer_count() == 2)
        assert not s1.closed.is_set() and not s3.closed.is_set()
        clock.t = t0 + 135
        cm.maintain()
        assert b.peer_count() == 2  # at the target: nobody else goes
    finally:
        for s in servers:
            s.close()
        b.stop()


def test_stale_tip_allows_one_extra_outbound(core, tmp_path):
    b, clock = _clocked_node(core, tmp_path, "b")
    try:
        cm = b.connman
        cm.maintain()
        assert not cm.try_new_outbound
        clock.advance(3 * b.params.pow_target_spacing)
        cm.maintain()
        assert not cm.try_new_outbound  # the stale check itself comes round every ten minutes
        clock.advance(601)
        cm.maintain()
        assert cm.try_new_outbound
        b.miner.generate(b.mining_script, 1)
        clock.advance(601)
        cm.maintain()
        assert not cm.try_new_outbound
    finally:
        b.stop()


def test_outbound_peer_behind_our_tip_is_dropped(core, tmp_path):
    b, clock = _clocked_node(core, tmp_path, "b")
    srv = None
    try:
        cm = b.connman
        b.miner.generate(b.mining_script, 1)  # our tip has more work than anything the peer shows
        srv = ScriptedServer(bytes(b.params.message_start))
        cm.connect("127.0.0.1", srv.port)
        s = srv.accept()
        assert wait(lambda: b.peer_count() == 1 and s.count("getheaders") == 1)
        np = node_peer(b, s)
        t0 = clock.t
        cm.maintain()  # behind our tip, noticed: 20 minutes from here

        def step(to):
            clock.t = to
            cm.maintain()
            assert wait(lambda: np.ping_nonce == 0 or np.closed.is_set())  # its pong is in: it is not silent

        for k in range(1, 13):
            step(t0 + 100 * k)
        assert s.count("getheaders") == 1 and not np.closed.is_set()  # exactly 20 min: not yet
        step(t0 + 1201)
        assert wait(lambda: s.count("getheaders") == 2) and not np.closed.is_set()
        step(t0 + 1201 + 120)
        assert s.count("getheaders") == 2 and not np.closed.is_set()  # one reminder only, 2 min not over
        step(t0 + 1201 + 121)
        assert np.closed.is_set() and s.closed.wait(10)
    finally:
        if srv is not None:
            srv.close()
        b.stop()


def test_addnode_flag_peer_is_manual(core, tmp_path):
    """-addnode peers are dialled from the address manager; like the RPC's they are manual
    connections, which the extra-outbound and chain-sync rules pass by."""
    srv = ScriptedServer(bytes(core.make_chain_params("regtest").message_start))
    b = None
    try:
        b = _node(core, tmp_path, "b", ["-listen", "-port=0", f"-addnode=127.0.0.1:{srv.port}"])
        s = srv.accept()
        assert wait(lambda: b.peer_count() == 1)
        np = node_peer(b, s)
        assert np.manual and not np.inbound
    finally:
        srv.close()
        if b is not None:
            b.stop()
