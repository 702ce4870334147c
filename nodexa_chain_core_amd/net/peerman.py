"""Connection slots and the inbound eviction selection.

Parity: CConnman::AcceptConnection / AttemptToEvictConnection (src/net.cpp:941-1135) and the
constants of src/net.h:46-78. The selection is a pure function over candidate records so that it
can be checked without sockets; net/p2p.py builds the records from its inbound peers.
"""
from __future__ import annotations

import ipaddress
import os
from typing import NamedTuple

from .. import core

_core = core()

DEFAULT_MAX_PEER_CONNECTIONS = 125  # -maxconnections (src/net.h:78)
MAX_FEELER_CONNECTIONS = 1          # one slot kept back, as the reference's nMaxFeeler (no feelers are made yet)
PING_INTERVAL = 2 * 60              # src/net.h:46
TIMEOUT_INTERVAL = 20 * 60          # src/net.h:48
HANDSHAKE_TIMEOUT = 60              # InactivityCheck's first minute (src/net.cpp:1413)

PROTECT_NETGROUP, PROTECT_PING, PROTECT_TX, PROTECT_BLOCK = 4, 8, 4, 4


class EvictionCandidate(NamedTuple):
    """NodeEvictionCandidate (src/net.h). `min_ping` is in seconds (inf while unmeasured)."""
    id: int
    connected: float
    min_ping: float
    last_block_time: float
    last_tx_time: float
    relevant_services: bool
    relay_txs: bool
    bloom_filter: bool
    keyed_net_group: int


def connection_slots(max_connections: int, max_outbound: int) -> tuple[int, int]:
    """(outbound target, inbound limit) for a -maxconnections total: outbound is capped by the
    total, inbound gets what the outbound slots and the feeler slot leave (src/net.cpp:1079)."""
    total = max(0, int(max_connections))
    outbound = min(int(max_outbound), total)
    return outbound, max(0, total - outbound - MAX_FEELER_CONNECTIONS)


class NetGroupKeyer:
    """CNode::CalculateKeyedNetGroup: a per-process SipHash of the peer's network group (the /16
    of an IPv4 address, the /32 of an IPv6 one), so which groups rule 1 protects cannot be guessed."""

    def __init__(self, key: bytes | None = None):
        key = key or os.urandom(16)
        self.k0 = int.from_bytes(key[:8], "little")
        self.k1 = int.from_bytes(key[8:16], "little")

    @staticmethod
    def net_group(host: str) -> bytes:
        try:
            a = ipaddress.ip_address(host.split("%")[0])
        except ValueError:
            return b"\x00" + host.encode()  # a name (an onion service): a group of its own
        if a.version == 6 and a.ipv4_mapped is not None:
            a = a.ipv4_mapped
        return (b"\x04" + a.packed[:2]) if a.version == 4 else (b"\x06" + a.packed[:4])

    def __call__(self, host: str) -> int:
        return _core.siphash24(self.k0, self.k1, self.net_group(host))


def _protect(cands: list, key, n: int) -> list:
    """Sort ascending by `key` (stable) and drop the last n: those are protected."""
    cands = sorted(cands, key=key)
    return cands[:max(0, len(cands) - n)]


def select_node_to_evict(candidates) -> int | None:
    """The id of the inbound peer to drop for a new connection, or None if every candidate is
    protected. The caller passes the inbound, non-whitelisted, not-yet-closing peers."""
    c = list(candidates)
    # 1. four peers by keyed net group (the highest keys: unpredictable without the key)
    c = _protect(c, lambda x: x.keyed_net_group, PROTECT_NETGROUP)
    # 2. the eight lowest minimum ping times
    c = _protect(c, lambda x: -x.min_ping, PROTECT_PING)
    # 3. the four that sent a transaction most recently (then relaying, unfiltered, older peers)
    c = _protect(c, lambda x: (x.last_tx_time, x.relay_txs, not x.bloom_filter, -x.connected), PROTECT_TX)
    # 4. the four that sent a block most recently (then useful services, older peers)
    c = _protect(c, lambda x: (x.last_block_time, x.relevant_services, -x.connected), PROTECT_BLOCK)
    # 5. the longer-connected half of the rest; what is left is ordered youngest first
    c = _protect(c, lambda x: -x.connected, len(c) // 2)
    if not c:
        return None
    # 6. the net group with the most candidates (a tie: the one whose newest member is younger)
    groups: dict[int, list] = {}
    best, best_n, best_t = None, 0, 0.0
    for x in c:
        g = groups.setdefault(x.keyed_net_group, [])
        g.append(x)
        if len(g) > best_n or (len(g) == best_n and g[0].connected > best_t):
            best, best_n, best_t = x.keyed_net_group, len(g), g[0].connected
    return groups[best][0].id
