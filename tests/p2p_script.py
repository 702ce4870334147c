"""Helpers for the peer-management tests: a mock clock and scripted raw-socket peers that speak
net/protocol.py framing (the style of the raw-socket tests in test_p2p_ext.py)."""
import socket
import struct
import threading
import time

from nodexa_chain_core_amd.net import protocol as P

POLL = 10.0  # the bound of every wait on a socket event


def wait(cond, timeout=POLL):
    end = time.time() + timeout
    while time.time() < end:
        if cond():
            return True
        time.sleep(0.01)
    return bool(cond())


class MockClock:
    """Starts at the real time (in whole seconds, so that sums of whole steps are exact), then
    moves only when told to."""

    def __init__(self):
        self.t = float(int(time.time()))

    def __call__(self):
        return self.t

    def advance(self, seconds):
        self.t += seconds
        return self.t


class ChainData:
    """Headers and raw blocks 1..n of a node's active chain, for scripted peers to serve."""

    def __init__(self, core, node):
        self.act = node.params.kawpow_activation_time
        self.core = core
        idx = [node.state.chain.at_height(h) for h in range(1, node.state.height() + 1)]
        self.headers = [i.header for i in idx]
        self.hashes = [i.hash for i in idx]
        self.height = {h: k + 1 for k, h in enumerate(self.hashes)}
        self.raw = {h: node.state.get_block_raw(h) for h in self.hashes}

    def headers_payload(self, upto=None):
        return self.core.headers_msg_encode(self.headers[:upto], self.act)


class ScriptedPeer:
    """One raw-socket peer. A reader thread records every message, completes the handshake from
    either side, answers pings (unless told not to) and hands `getheaders` / `getdata` to the
    optional callbacks `on_getheaders(peer)` and `on_getdata(peer, hashes)`."""

    def __init__(self, magic, sock, answer_pings=True, on_getheaders=None, on_getdata=None, nonce=None):
        self.magic, self.sock = magic, sock
        self.answer_pings = answer_pings
        self.on_getheaders, self.on_getdata = on_getheaders, on_getdata
        self.nonce = nonce or (id(self) & 0xFFFFFFFF) + 1000
        self.msgs = []
        self.lock = threading.Lock()
        self.sent_version = False
        self.handshaken = threading.Event()
        self.closed = threading.Event()  # the node closed the connection (or it broke)
        self.thread = threading.Thread(target=self._run, daemon=True)

    @classmethod
    def dial(cls, port, magic, handshake=True, **kw):
        """An inbound peer of the node listening on `port`."""
        p = cls(magic, socket.create_connection(("127.0.0.1", port)), **kw)
        p.thread.start()
        if handshake:
            p.send_version()
            assert p.handshaken.wait(POLL)
        return p

    def send(self, cmd, payload=b""):
        self.sock.sendall(P.frame(self.magic, cmd, payload))

    def send_version(self):
        self.sent_version = True
        self.send("version", P.version_payload(0, nonce=self.nonce))

    def _run(self):
        try:
            while True:
                cmd, payload = P.read_message(self.sock, self.magic)
                with self.lock:
                    self.msgs.append((cmd, payload))
                if cmd == "version":
                    if not self.sent_version:
                        self.send_version()
                    self.send("verack")
                elif cmd == "verack":
                    self.handshaken.set()
                elif cmd == "ping" and self.answer_pings:
                    self.send("pong", payload)
                elif cmd == "getheaders" and self.on_getheaders:
                    self.on_getheaders(self)
                elif cmd == "getdata" and self.on_getdata:
                    blocks = [h for t, h in P.parse_inv(payload) if t & ~P.MSG_WITNESS_FLAG == P.MSG_BLOCK]
                    if blocks:
                        self.on_getdata(self, blocks)
        except (OSError, P.ProtocolError, struct.error, ValueError):
            pass
        finally:
            self.closed.set()

    def count(self, cmd):
        with self.lock:
            return sum(1 for c, _ in self.msgs if c == cmd)

    def payloads(self, cmd):
        with self.lock:
            return [p for c, p in self.msgs if c == cmd]

    def close(self):
        try:
            self.sock.shutdown(socket.SHUT_RDWR)
        except OSError:
            pass
        self.sock.close()


class ScriptedServer:
    """A listening socket whose accepted connections become ScriptedPeers: the far end of
    ConnectionManager.connect()."""

    def __init__(self, magic, **kw):
        self.magic, self.kw = magic, kw
        self.srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        self.srv.bind(("127.0.0.1", 0))
        self.srv.listen(8)
        self.port = self.srv.getsockname()[1]

    def accept(self):
        self.srv.settimeout(POLL)
        sock, _ = self.srv.accept()
        p = ScriptedPeer(self.magic, sock, **self.kw)
        p.thread.start()
        assert p.handshaken.wait(POLL)
        return p

    def close(self):
        self.srv.close()


def node_peer(node, peer_or_port):
    """The node's Peer object for a scripted peer (matched by the scripted side's local port)."""
    port = peer_or_port if isinstance(peer_or_port, int) else peer_or_port.sock.getsockname()[1]
    for p in list(node.connman.peers):
        if p.addr[1] == port:
            return p
    return None
