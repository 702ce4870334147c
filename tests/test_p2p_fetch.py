"""Tracked block download (net/blockfetch.py): the per-peer and window limits, one holder per
block, the stall and timeout penalties, and out-of-order arrival, against scripted peers that
serve a 24-block regtest chain mined once on a real node."""
import threading

import pytest

from p2p_script import ChainData, MockClock, ScriptedPeer, node_peer, wait
from test_p2p import _node

N_BLOCKS = 24


@pytest.fixture(scope="module")
def chain_a(core, tmp_path_factory):
    """Node A with the 24-block chain, and that chain's headers and raw blocks. Read-only."""
    a = _node(core, tmp_path_factory.mktemp("fetch_a"), "a", ["-listen", "-port=0"])
    try:
        a.miner.generate(a.mining_script, N_BLOCKS)
        assert a.state.height() == N_BLOCKS
        yield a, ChainData(core, a)
    finally:
        a.stop()


def _node_b(core, tmp_path, per_peer=None, window=None, clock=None):
    b = _node(core, tmp_path, "b", ["-listen", "-port=0"])
    if per_peer is not None:
        b.connman.max_blocks_in_transit_per_peer = per_peer
    if window is not None:
        b.connman.block_download_window = window
    if clock is not None:
        b.connman.set_clock(clock)
    return b


def _serves_headers(data):
    return lambda peer: peer.send("headers", data.headers_payload())


class Ledger:
    """What the scripted peers see of B's requests, checked as they arrive."""

    def __init__(self, data, per_peer, window):
        self.data, self.per_peer, self.window = data, per_peer, window
        self.lock = threading.Lock()
        self.outstanding = {}   # hash -> the scripted peer it was asked of and has not yet sent it
        self.sent = set()       # heights sent to B
        self.errors = []
        self.most = 0           # the most requests one peer ever had outstanding

    def linked(self):
        h = 0
        while h + 1 in self.sent:
            h += 1
        return h

    def requested(self, peer, hashes):
        with self.lock:
            for h in hashes:
                height = self.data.height[h]
                if h in self.outstanding:
                    self.errors.append(f"block {height} asked of two peers at once")
                if height in self.sent:
                    self.errors.append(f"block {height} asked for again after it was sent")
                # B's last common block with anybody is at most the last block up to which all were
                # sent to it, so nothing may be asked for beyond that plus the window
                if height > self.linked() + self.window:
                    self.errors.append(f"block {height} asked for with only 1..{self.linked()} sent")
                self.outstanding[h] = peer
            mine = sum(1 for p in self.outstanding.values() if p is peer)
            self.most = max(self.most, mine)
            if mine > self.per_peer:
                self.errors.append(f"{mine} requests outstanding at one peer")

    def sending(self, h):
        with self.lock:
            self.outstanding.pop(h, None)
            self.sent.add(self.data.height[h])


def test_fetch_limits(core, tmp_path, chain_a):
    a, data = chain_a
    b = _node_b(core, tmp_path, per_peer=4, window=8)
    peers = []
    try:
        ledger = Ledger(data, per_peer=4, window=8)

        def serve(peer, hashes):
            ledger.requested(peer, hashes)
            for h in reversed(hashes):  # newest first, so that B holds blocks it cannot connect yet
                ledger.sending(h)
                peer.send("block", data.raw[h])

        magic = bytes(b.params.message_start)
        peers = [ScriptedPeer.dial(b.connman.port, magic, on_getheaders=_serves_headers(data), on_getdata=serve)
                 for _ in range(2)]
        assert wait(lambda: b.state.height() == N_BLOCKS), (b.state.height(), ledger.errors)
        assert ledger.errors == []
        assert ledger.most == 4  # the limit was reached, and never passed
        assert len(ledger.sent) == N_BLOCKS and b.state.tip().hash == a.state.tip().hash
        assert wait(lambda: b.connman.fetcher.blocks_in_flight() == 0)  # the last record goes once it is stored
    finally:
        for p in peers:
            p.close()
        b.stop()


def test_withholding_peer_is_dropped_as_staller(core, tmp_path, chain_a):
    a, data = chain_a
    clock = MockClock()
    b = _node_b(core, tmp_path, per_peer=4, window=8, clock=clock)
    w = None
    try:
        cm = b.connman
        asked = []
        w = ScriptedPeer.dial(cm.port, bytes(b.params.message_start), on_getheaders=_serves_headers(data),
                              on_getdata=lambda peer, hashes: asked.extend(hashes))  # and never a block
        assert wait(lambda: len(asked) == 4)
        nw = node_peer(b, w)
        info = [i for i in b.table.execute("getpeerinfo", []) if i["id"] == nw.id][0]
        assert info["inflight"] == [1, 2, 3, 4] and info["synced_headers"] == N_BLOCKS and info["synced_blocks"] == 0
        # A serves 5-8; then the window (8 above the common block 0) is used up, blocks 1-4 held by W
        # are all that is in the way: W is the staller
        cm.connect("127.0.0.1", a.connman.port)
        ws = cm.fetcher.peers[nw.id]
        assert wait(lambda: ws.stalling_since != 0)
        assert ws.stalling_since == clock.t
        # (W is named as soon as A's free slot finds nothing but W's blocks in the way, which may be
        # while A's own four are still arriving)
        assert wait(lambda: all(data.hashes[k] in b.state.block_pos for k in range(4, 8))
                    and cm.fetcher.blocks_in_flight() == 4)  # A's are in; W's four are all that is out
        assert b.state.height() == 0
        clock.advance(2)
        cm.maintain()
        assert not nw.closed.is_set()  # two seconds, not yet more
        clock.advance(1)
        cm.maintain()
        assert nw.closed.is_set() and w.closed.wait(10)
        # W's blocks are free again and asked of A, and the sync completes
        assert wait(lambda: b.state.height() == N_BLOCKS), b.state.height()
        assert b.state.tip().hash == a.state.tip().hash
        assert len(asked) == 4  # W was never asked for more than its first four
    finally:
        if w is not None:
            w.close()
        b.stop()


def test_withholding_only_peer_times_out(core, tmp_path, chain_a):
    a, data = chain_a
    clock = MockClock()
    b = _node_b(core, tmp_path, clock=clock)
    w = None
    try:
        cm = b.connman
        asked = []
        w = ScriptedPeer.dial(cm.port, bytes(b.params.message_start), on_getheaders=_serves_headers(data),
                              on_getdata=lambda peer, hashes: asked.extend(hashes))
        assert wait(lambda: len(asked) == 16)  # the default limit per peer
        nw = node_peer(b, w)
        spacing = b.params.pow_target_spacing
        # alone, so no other peer with blocks in flight stretches the limit: one target spacing
        clock.advance(spacing)
        cm.maintain()
        assert not nw.closed.is_set()
        clock.advance(1)
        cm.maintain()
        assert nw.closed.is_set() and w.closed.wait(10)
        assert wait(lambda: cm.fetcher.blocks_in_flight() == 0)
        assert len(asked) == 16
    finally:
        if w is not None:
            w.close()
        b.stop()


def test_out_of_order_delivery(core, tmp_path, chain_a):
    a, data = chain_a
    b = _node_b(core, tmp_path, per_peer=8, window=8)
    s = None
    try:
        held, sent, order = [], set(), []

        def serve(peer, hashes):
            held.extend(hashes)
            if len(held) < min(8, N_BLOCKS - len(sent)):
                return  # wait until B has asked for the whole window
            for h in sorted(held, key=lambda x: -data.height[x]):
                sent.add(h)
                order.append(data.height[h])
                peer.send("block", data.raw[h])
            held.clear()

        s = ScriptedPeer.dial(b.connman.port, bytes(b.params.message_start), on_getheaders=_serves_headers(data),
                              on_getdata=serve)
        assert wait(lambda: b.state.height() == N_BLOCKS), (b.state.height(), order)
        assert order == [8, 7, 6, 5, 4, 3, 2, 1, 16, 15, 14, 13, 12, 11, 10, 9, 24, 23, 22, 21, 20, 19, 18, 17]
        b.state.check_block_index()
        assert b.state.tip().hash == a.state.tip().hash
        assert all(h in b.state.block_pos for h in data.hashes)
    finally:
        if s is not None:
            s.close()
        b.stop()


def test_mutated_block_under_a_real_header_does_not_stop_the_sync(core, tmp_path, chain_a):
    """Anybody can wrap a real header around other transactions. Such a block is refused before it
    is stored; the real block with that header stays wanted and is fetched from an honest peer."""
    a, data = chain_a
    b = _node(core, tmp_path, "b", ["-listen", "-port=0", "-whitelist=127.0.0.1"])  # one address for all: no ban
    m = h = None
    try:
        cm = b.connman
        magic = bytes(b.params.message_start)
        m = ScriptedPeer.dial(cm.port, magic, on_getheaders=_serves_headers(data))  # headers, never a block
        assert wait(lambda: b.state.chain.height() == N_BLOCKS)
        nm = node_peer(b, m)
        for k in (0, 4, N_BLOCKS - 1):  # the next block wanted, one further on, and the best header's
            blk = core.Block.deserialize(data.raw[data.hashes[k]], data.act)
            blk.vtx = list(blk.vtx) * 2  # the header's merkle root no longer fits
            m.send("block", blk.serialize(data.act))
        assert wait(lambda: nm.misbehavior >= 300), nm.misbehavior  # all three were read and refused
        assert b.state.height() == 0 and not any(x in b.state.block_pos for x in data.hashes)
        assert not cm.fetcher.rejected
        m.close()
        assert wait(lambda: b.peer_count() == 0)
        h = ScriptedPeer.dial(cm.port, magic, on_getheaders=_serves_headers(data),
                              on_getdata=lambda peer, hashes: [peer.send("block", data.raw[x]) for x in hashes])
        assert wait(lambda: b.state.height() == N_BLOCKS), b.state.height()
        assert b.state.tip().hash == a.state.tip().hash
    finally:
        for p in (m, h):
            if p is not None:
                p.close()
        b.stop()


def test_rejected_set_is_bounded(core, tmp_path, chain_a):
    from nodexa_chain_core_amd.net.blockfetch import MAX_REJECTED, BlockFetcher

    a, _ = chain_a
    f = BlockFetcher(a.state)
    for k in range(MAX_REJECTED + 10):
        f.mark_rejected(k.to_bytes(32, "little"))
    assert len(f.rejected) == MAX_REJECTED
    assert (0).to_bytes(32, "little") not in f.rejected  # the oldest went
    assert (MAX_REJECTED + 9).to_bytes(32, "little") in f.rejected
