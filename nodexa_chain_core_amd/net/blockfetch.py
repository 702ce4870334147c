"""Tracked block download: which block is asked of which peer, and who is holding the sync up.

Parity: FindNextBlocksToDownload / MarkBlockAsInFlight / MarkBlockAsReceived /
UpdateBlockAvailability (src/net_processing.cpp:340-540), the stall and timeout block of
SendMessages (:3660-3750) and the outbound chain-sync bookkeeping of ConsiderEviction
(:3106-3156). Constants are those of src/validation.h:100-141 and src/net_processing.h:31-39.

The fetcher only keeps records and decides; net/p2p.py sends the `getdata` and closes peers.
Its lock (`cs_fetch`) is a leaf: nothing is sent, and no other Python lock is taken, under it.
"""
from __future__ import annotations

import time

from ..utils import sync

MAX_BLOCKS_IN_TRANSIT_PER_PEER = 16   # src/validation.h:100
BLOCK_STALLING_TIMEOUT = 2            # seconds (src/validation.h:102)
BLOCK_DOWNLOAD_WINDOW = 1024          # src/validation.h:115
BLOCK_DOWNLOAD_TIMEOUT_BASE = 1.0     # in units of the target spacing (src/validation.h:139)
BLOCK_DOWNLOAD_TIMEOUT_PER_PEER = 0.5  # per other downloading peer (src/validation.h:141)
MAX_OUTBOUND_PEERS_TO_PROTECT_FROM_DISCONNECT = 4  # src/net_processing.h:31
CHAIN_SYNC_TIMEOUT = 20 * 60          # src/net_processing.h:33
HEADERS_RESPONSE_TIME = 2 * 60        # src/net_processing.cpp:3146
STALE_CHECK_INTERVAL = 10 * 60        # src/net_processing.h:35
EXTRA_PEER_CHECK_INTERVAL = 45        # src/net_processing.h:37
MINIMUM_CONNECT_TIME = 30             # src/net_processing.h:39
MAX_REJECTED = 1024                   # this engine's: remembered blocks that failed to connect


class PeerFetchState:
    """The block-download part of CNodeState."""

    def __init__(self):
        self.best_known: bytes | None = None    # pindexBestKnownBlock
        self.best_height = -1
        self.best_work = 0
        self.last_unknown: bytes | None = None  # hashLastUnknownBlock: announced before its header was here
        self.last_common: bytes | None = None   # pindexLastCommonBlock
        self.common_height = -1
        self.queue: list[tuple[bytes, int, float]] = []  # vBlocksInFlight: (hash, height, request time)
        self.downloading_since = 0.0
        self.stalling_since = 0.0
        self.last_block_announcement = 0.0
        # ChainSyncTimeoutState
        self.sync_timeout = 0.0
        self.sync_work = 0
        self.sync_sent_getheaders = False
        self.sync_protect = False


class BlockFetcher:
    def __init__(self, state, clock=time.time, window: int = BLOCK_DOWNLOAD_WINDOW,
                 per_peer: int = MAX_BLOCKS_IN_TRANSIT_PER_PEER):
        self.state = state
        self.clock = clock
        self.window = window
        self.per_peer = per_peer
        self.lock = sync.make_lock("cs_fetch")
        self.peers: dict[int, PeerFetchState] = {}
        self.in_flight: dict[bytes, tuple[int, float]] = {}  # mapBlocksInFlight: hash -> (peer id, request time)
        # stored blocks that failed to connect (newest MAX_REJECTED of them): what builds on them is
        # not fetched. Only a block whose transactions matched its header and that was written gets
        # here, never one refused for what a sender can alter under a real header.
        self.rejected: dict[bytes, None] = {}
        self.protected_outbound = 0

    # ------------------------------------------------------------------ peers
    def add_peer(self, pid: int) -> None:
        with self.lock:
            self.peers.setdefault(pid, PeerFetchState())

    def remove_peer(self, pid: int) -> list[bytes]:
        """FinalizeNode: the peer's in-flight records are freed; the next pass asks the others."""
        with self.lock:
            ps = self.peers.pop(pid, None)
            if ps is None:
                return []
            if ps.sync_protect:
                self.protected_outbound -= 1
            freed = [h for h, _, _ in ps.queue]
            for h in freed:
                if self.in_flight.get(h, (None,))[0] == pid:
                    del self.in_flight[h]
            return freed

    def _has_data(self, h: bytes) -> bool:
        return h in self.state.block_pos or h in self.state._mem_blocks

    # ------------------------------------------------------------------ what a peer has
    def _process_availability(self, ps: PeerFetchState) -> None:
        """ProcessBlockAvailability: an announced hash whose header has arrived since."""
        if ps.last_unknown is not None:
            idx = self.state.chain.find(ps.last_unknown)
            if idx is not None:
                if idx.chain_work > 0 and (ps.best_known is None or idx.chain_work >= ps.best_work):
                    ps.best_known, ps.best_height, ps.best_work = idx.hash, idx.height, idx.chain_work
                ps.last_unknown = None

    def update_availability(self, pid: int, h: bytes, announced: bool = True) -> None:
        """UpdateBlockAvailability: the peer has told us it has block `h` (a header it sent and we
        accepted, or a block inv)."""
        idx = self.state.chain.find(h)
        with self.lock:
            ps = self.peers.get(pid)
            if ps is None:
                return
            self._process_availability(ps)
            if idx is None:
                ps.last_unknown = h
            elif ps.best_known is None or idx.chain_work >= ps.best_work:
                ps.best_known, ps.best_height, ps.best_work = idx.hash, idx.height, idx.chain_work
            if announced:
                ps.last_block_announcement = self.clock()

    # ------------------------------------------------------------------ selection
    def _fork_point(self, a, b):
        chain = self.state.chain
        if a.height > b.height:
            a = a.ancestor(b.height)
        elif b.height > a.height:
            b = b.ancestor(a.height)
        while a is not None and b is not None and a.hash != b.hash:
            a, b = chain.find(a.prev_hash), chain.find(b.prev_hash)
        return a

    def _next_blocks(self, pid: int, ps: PeerFetchState, count: int) -> tuple[list, int | None]:
        """FindNextBlocksToDownload. Returns ([(hash, height)], staller id or None)."""
        out: list[tuple[bytes, int]] = []
        if count <= 0:
            return out, None
        chain = self.state.chain
        self._process_availability(ps)
        tip = self.state.tip()
        best = chain.find(ps.best_known) if ps.best_known is not None else None
        if best is None or best.chain_work < tip.chain_work:
            return out, None  # this peer has nothing interesting
        common = chain.find(ps.last_common) if ps.last_common is not None else None
        if common is None:  # guess: the block of our chain at the peer's height
            common = tip.ancestor(min(best.height, tip.height))
        common = self._fork_point(common, best)
        if common is None:
            return out, None
        # what is stored and linked above it is in common too; the window is measured from there
        while common.height < best.height:
            nxt = best.ancestor(common.height + 1)
            if nxt.hash in self.rejected or not self._has_data(nxt.hash):
                break
            common = nxt
        ps.last_common, ps.common_height = common.hash, common.height
        if common.hash == best.hash:
            return out, None
        # no further than what the peer has, nor than one past the window: that one more is how
        # a stall shows (we could fetch it if the window were one larger)
        window_end = common.height + self.window
        max_height = min(best.height, window_end + 1)
        waiting_for = None
        for height in range(common.height + 1, max_height + 1):
            idx = best.ancestor(height)
            h = idx.hash
            if h in self.rejected:
                return out, None  # the chain this peer is on is invalid
            if self._has_data(h):
                continue
            holder = self.in_flight.get(h)
            if holder is None:
                if height > window_end:
                    if not out and waiting_for is not None and waiting_for != pid:
                        return out, waiting_for
                    return out, None
                out.append((h, height))
                if len(out) == count:
                    return out, None
            elif waiting_for is None:
                waiting_for = holder[0]  # the first already-in-flight block
        return out, None

    def assign(self, pid: int, now: float | None = None) -> tuple[list[tuple[bytes, int]], int | None]:
        """Pick the next blocks for this peer and mark them in flight (MarkBlockAsInFlight). A peer
        named staller gets its `stalling_since` set if it is not. Returns (blocks, staller id)."""
        with self.lock:
            ps = self.peers.get(pid)
            if ps is None:
                return [], None
            blocks, staller = self._next_blocks(pid, ps, self.per_peer - len(ps.queue))
            now = self.clock() if now is None else now
            for h, height in blocks:
                if not ps.queue:
                    ps.downloading_since = now
                ps.queue.append((h, height, now))
                self.in_flight[h] = (pid, now)
            if staller is not None:
                ss = self.peers.get(staller)
                if ss is not None and not ss.stalling_since:
                    ss.stalling_since = now
            return blocks, staller

    def unassign(self, pid: int, hashes) -> None:
        """The request could not be written to the peer: free the records again."""
        gone = set(hashes)
        with self.lock:
            ps = self.peers.get(pid)
            if ps is None:
                return
            ps.queue = [e for e in ps.queue if e[0] not in gone]
            for h in gone:
                if self.in_flight.get(h, (None,))[0] == pid:
                    del self.in_flight[h]

    def received(self, h: bytes) -> int | None:
        """MarkBlockAsReceived: a block arrived (from anybody); its record is cleared. Returns the
        id of the peer it had been asked of."""
        with self.lock:
            rec = self.in_flight.pop(h, None)
            if rec is None:
                return None
            ps = self.peers.get(rec[0])
            if ps is not None:
                if ps.queue and ps.queue[0][0] == h:
                    # the head of the queue came: the next one's clock starts now
                    ps.downloading_since = max(ps.downloading_since, self.clock())
                ps.queue = [e for e in ps.queue if e[0] != h]
                ps.stalling_since = 0.0
            return rec[0]

    def mark_rejected(self, h: bytes) -> None:
        with self.lock:
            self.rejected.pop(h, None)
            self.rejected[h] = None
            while len(self.rejected) > MAX_REJECTED:
                del self.rejected[next(iter(self.rejected))]

    # ------------------------------------------------------------------ penalties
    def check_peer(self, pid: int, spacing: float, now: float | None = None) -> str | None:
        """The stall and timeout rules of SendMessages: a reason to disconnect, or None."""
        now = self.clock() if now is None else now
        with self.lock:
            ps = self.peers.get(pid)
            if ps is None:
                return None
            if ps.stalling_since and ps.stalling_since < now - BLOCK_STALLING_TIMEOUT:
                return "stalling block download"
            if ps.queue:
                others = sum(1 for q, s in self.peers.items() if q != pid and s.queue)
                limit = spacing * (BLOCK_DOWNLOAD_TIMEOUT_BASE + BLOCK_DOWNLOAD_TIMEOUT_PER_PEER * others)
                if now > ps.downloading_since + limit:
                    return f"timeout downloading block at height {ps.queue[0][1]}"
        return None

    def consider_eviction(self, pid: int, now: float | None = None) -> str | None:
        """ConsiderEviction for one outbound peer: "getheaders" when it is due its one reminder,
        "disconnect" when it stayed behind our tip, else None."""
        now = self.clock() if now is None else now
        tip = self.state.tip()
        with self.lock:
            ps = self.peers.get(pid)
            if ps is None or ps.sync_protect:
                return None
            self._process_availability(ps)
            if ps.best_known is not None and ps.best_work >= tip.chain_work:
                if ps.sync_timeout:
                    ps.sync_timeout, ps.sync_work, ps.sync_sent_getheaders = 0.0, 0, False
                if self.protected_outbound < MAX_OUTBOUND_PEERS_TO_PROTECT_FROM_DISCONNECT:
                    ps.sync_protect = True  # it has shown a chain at least as good as ours
                    self.protected_outbound += 1
            elif not ps.sync_timeout or (ps.sync_work and ps.best_known is not None and ps.best_work >= ps.sync_work):
                # behind our tip: noticed for the first time, or it caught up to where we were then
                ps.sync_timeout = now + CHAIN_SYNC_TIMEOUT
                ps.sync_work, ps.sync_sent_getheaders = tip.chain_work, False
            elif now > ps.sync_timeout:
                if ps.sync_sent_getheaders:
                    return "disconnect"
                ps.sync_sent_getheaders = True
                ps.sync_timeout = now + HEADERS_RESPONSE_TIME
                return "getheaders"
        return None

    # ------------------------------------------------------------------ views
    def peer_view(self, pid: int) -> dict:
        with self.lock:
            ps = self.peers.get(pid)
            if ps is None:
                return {"synced_headers": -1, "synced_blocks": -1, "inflight": []}
            return {"synced_headers": ps.best_height, "synced_blocks": ps.common_height,
                    "inflight": [height for _, height, _ in ps.queue]}

    def blocks_in_flight(self, pid: int | None = None) -> int:
        with self.lock:
            if pid is None:
                return len(self.in_flight)
            ps = self.peers.get(pid)
            return len(ps.queue) if ps is not None else 0

    def last_block_announcement(self, pid: int) -> float:
        with self.lock:
            ps = self.peers.get(pid)
            return ps.last_block_announcement if ps is not None else 0.0

    def is_protected(self, pid: int) -> bool:
        with self.lock:
            ps = self.peers.get(pid)
            return bool(ps is not None and ps.sync_protect)
