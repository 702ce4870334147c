"""The rank supervisor: a GPU-free process that owns the follower ranks of the node's miner world.

Rank 0 is the node, and by the time a follower dies it has initialised its GPU; a process in that
state must not start children. So rank 0 starts this supervisor where it would otherwise spawn the
followers itself (before parallel/world.init, before any GPU call), and every follower, the first
ones and every re-spawn, is a child of the supervisor. The supervisor never imports torch and
never opens a GPU: `assert_gpu_untouched` checks that before every `Popen`.

It runs as a script (`python supervisor.py`, standard library only) and talks to rank 0 over its
stdin / stdout in JSON lines, nothing else:

  commands   {"cmd": "spawn", "gpu": g, "rank": r, "world_size": n, "life": k | absent,
              "join_membership": m | null, "env": {...}, "argv": [...] | absent}
             {"cmd": "status"}    -> {"status": {"pid", "torch_loaded", "children": [...], "lives": {...}}}
             {"cmd": "stop"}
  events     {"event": "exited", "gpu": g, "rank": r, "life": k, "code": c}

`rank` is the follower's global id (the rank it had in the first world; on a GPU node one per
GPU, so the issue of "which GPU" and "which rank" is the same question; host rehearsals put
several ranks on device 0 and tell them apart by it). The follower's environment carries
NODEXA_MINER_LIFE=<k>: 0 for the first process of a rank, +1 per re-spawn. The followers write
to the supervisor's stderr; its stdout carries events only. On `stop`, or when stdin reaches EOF
(the node died), the supervisor terminates its followers, kills what is left after a short wait,
and exits: no follower outlives the node.

The same module holds rank 0's side: `SupervisorClient` (the pipe) and `RejoinPolicy` (whether a
lost rank may come back, a pure decision with an injectable clock).
"""
from __future__ import annotations

import json
import os
import queue
import re
import select
import subprocess
import sys
import threading
import time

_GPU_NODE = re.compile(r"^/dev/(kfd|dri/renderD\d+)$")
TERM_WAIT_S = 3.0  # between SIGTERM and SIGKILL when the supervisor ends its followers
FOLLOWER_ARGV = ["-m", "nodexa_chain_core_amd.miner.service"]


class GpuTouched(RuntimeError):
    """The process that is about to start a child has a GPU device node open."""


def _self_fd_table() -> dict[int, str]:
    table = {}
    for name in os.listdir("/proc/self/fd"):
        try:
            table[int(name)] = os.readlink(f"/proc/self/fd/{name}")
        except OSError:  # the fd of the listing itself, already closed
            continue
    return table


def assert_gpu_untouched(fd_table: dict | None = None) -> None:
    """Fail closed if this process holds the compute device (/dev/kfd) or a render node
    (/dev/dri/renderD*): `fd_table` maps fd -> target (default: /proc/self/fd; a table that cannot
    be read is a failure too)."""
    if fd_table is None:
        try:
            fd_table = _self_fd_table()
        except OSError as e:
            raise GpuTouched(f"cannot read /proc/self/fd ({e}): not spawning") from e
    for fd, target in fd_table.items():
        if _GPU_NODE.match(str(target)):
            raise GpuTouched(f"fd {fd} is {target}: a process that opened a GPU must not spawn ranks")


# ------------------------------------------------------------------------------ eligibility
class RejoinPolicy:
    """-minerrejoin / -minerrejoinmax / -minerrejoinwindow as a pure decision.

    `record_exit(gpu)` notes that the rank's process ended abnormally (75 hung, 76 evicted, a
    signal, or a newcomer that died before it was ready). `decide(now, gpu)`:
      "refused"  re-join is off (delay 0), the world belongs to torchrun, or the rank has ended
                 `max_exits` times within the last `window_s` seconds (it becomes eligible again
                 once enough of those exits are older than the window);
      "wait"     less than `delay_s` since its last exit;
      "spawn"    otherwise."""

    def __init__(self, delay_s: float = 0.0, max_exits: int = 3, window_s: float = 600.0,
                 torchrun: bool = False, clock=time.monotonic):
        self.delay_s, self.max_exits, self.window_s = float(delay_s), int(max_exits), float(window_s)
        self.torchrun = bool(torchrun)
        self.clock = clock
        self.exits: dict[int, list[float]] = {}

    @property
    def enabled(self) -> bool:
        return self.delay_s > 0 and not self.torchrun

    def record_exit(self, gpu: int, now: float | None = None) -> None:
        self.exits.setdefault(int(gpu), []).append(self.clock() if now is None else now)

    def recent_exits(self, now: float, gpu: int) -> int:
        return sum(1 for t in self.exits.get(int(gpu), []) if now - t < self.window_s)

    def decide(self, now: float, gpu: int) -> str:
        if not self.enabled:
            return "refused"
        if self.recent_exits(now, gpu) >= self.max_exits:
            return "refused"
        ex = self.exits.get(int(gpu))
        if ex and now - ex[-1] < self.delay_s:
            return "wait"
        return "spawn"

    def rejoin_in(self, now: float, gpu: int) -> float | None:
        """Seconds until `gpu` may be spawned again (None: refused or never lost)."""
        ex = self.exits.get(int(gpu))
        if not ex or self.decide(now, gpu) == "refused":
            return None
        return max(0.0, self.delay_s - (now - ex[-1]))


# ------------------------------------------------------------------------------ rank 0's side
class SupervisorClient:
    """Rank 0's end of the pipe. Construct it before this process touches a GPU."""

    def __init__(self, python: str | None = None):
        assert_gpu_untouched()
        self.proc = subprocess.Popen([python or sys.executable, os.path.abspath(__file__)],
                                     stdin=subprocess.PIPE, stdout=subprocess.PIPE)
        self._events: queue.Queue = queue.Queue()
        self._status: queue.Queue = queue.Queue()
        self._lock = threading.Lock()
        self._reader = threading.Thread(target=self._read, name="miner-supervisor", daemon=True)
        self._reader.start()

    def _read(self) -> None:
        for line in self.proc.stdout:
            try:
                msg = json.loads(line)
            except ValueError:
                continue
            (self._status if "status" in msg else self._events).put(msg)

    def _send(self, msg: dict) -> None:
        with self._lock:
            self.proc.stdin.write((json.dumps(msg) + "\n").encode())
            self.proc.stdin.flush()

    def spawn(self, *, gpu: int, rank: int, world_size: int, env: dict, join_membership: int | None = None,
              life: int | None = None, argv: list | None = None) -> None:
        msg = {"cmd": "spawn", "gpu": int(gpu), "rank": int(rank), "world_size": int(world_size),
               "join_membership": join_membership, "env": {k: str(v) for k, v in env.items()}}
        if life is not None:
            msg["life"] = int(life)
        if argv is not None:
            msg["argv"] = list(argv)
        self._send(msg)

    def status(self, timeout: float = 5.0) -> dict:
        self._send({"cmd": "status"})
        return self._status.get(timeout=timeout)["status"]

    def events(self) -> list[dict]:
        """The events that arrived since the last call (never blocks)."""
        out = []
        while True:
            try:
                out.append(self._events.get_nowait())
            except queue.Empty:
                return out

    def stop(self, timeout: float = 2 * TERM_WAIT_S + 5) -> None:
        """End the followers and the supervisor (idempotent)."""
        if self.proc.poll() is None:
            try:
                self._send({"cmd": "stop"})
                self.proc.stdin.close()
            except (OSError, ValueError):
                pass
            try:
                self.proc.wait(timeout=timeout)
            except subprocess.TimeoutExpired:
                self.proc.kill()
                self.proc.wait()


def follower_pythonpath() -> str:
    """PYTHONPATH under which a follower finds this package, wherever the node was started."""
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    old = os.environ.get("PYTHONPATH", "")
    return root + (os.pathsep + old if old else "")


# ------------------------------------------------------------------------------ the supervisor
class _Supervisor:
    def __init__(self, out):
        self.out = out
        self.children: dict[int, dict] = {}   # global id -> {proc, gpu, life}
        self.lives: dict[int, int] = {}       # global id -> processes started so far

    def emit(self, msg: dict) -> None:
        self.out.write(json.dumps(msg) + "\n")
        self.out.flush()

    def spawn(self, cmd: dict) -> None:
        rank, gpu, n = int(cmd["rank"]), int(cmd["gpu"]), int(cmd["world_size"])
        old = self.children.get(rank)
        if old is not None and old["proc"].poll() is None:
            raise RuntimeError(f"rank {rank} is still running (pid {old['proc'].pid})")
        self.reap()
        life = int(cmd.get("life", self.lives.get(rank, 0)))
        env = dict(os.environ)
        env.update({"RANK": str(rank), "WORLD_SIZE": str(n), "LOCAL_RANK": str(rank),
                    "NODEXA_MINER_DEVICE": str(gpu), "NODEXA_MINER_LIFE": str(life)})
        if cmd.get("join_membership") is not None:
            env["NODEXA_MINER_JOIN_MEMBERSHIP"] = str(int(cmd["join_membership"]))
        env.update({str(k): str(v) for k, v in (cmd.get("env") or {}).items()})
        argv = [sys.executable] + [str(a) for a in (cmd.get("argv") or FOLLOWER_ARGV)]
        assert_gpu_untouched()
        # the followers' output goes to stderr: stdout belongs to the event stream
        proc = subprocess.Popen(argv, env=env, stdin=subprocess.DEVNULL, stdout=sys.stderr.fileno())
        self.lives[rank] = life + 1
        self.children[rank] = {"proc": proc, "gpu": gpu, "life": life}

    def reap(self) -> None:
        for rank, c in list(self.children.items()):
            code = c["proc"].poll()
            if code is not None:
                del self.children[rank]
                self.emit({"event": "exited", "gpu": c["gpu"], "rank": rank, "life": c["life"], "code": code})

    def status(self) -> dict:
        return {"pid": os.getpid(), "torch_loaded": "torch" in sys.modules,
                "children": [{"rank": r, "gpu": c["gpu"], "life": c["life"], "pid": c["proc"].pid}
                             for r, c in sorted(self.children.items())],
                "lives": {str(r): n for r, n in sorted(self.lives.items())}}

    def handle(self, line: bytes) -> bool:
        """One command line; False on `stop`."""
        try:
            cmd = json.loads(line)
            what = cmd.get("cmd")
            if what == "stop":
                return False
            if what == "spawn":
                self.spawn(cmd)
            elif what == "status":
                self.reap()
                self.emit({"status": self.status()})
            else:
                raise ValueError(f"unknown command {what!r}")
        except Exception as e:  # noqa: BLE001 — a bad command must not take the followers down
            self.emit({"event": "error", "error": f"{type(e).__name__}: {e}"})
        return True

    def shutdown(self) -> None:
        procs = [c["proc"] for c in self.children.values()]
        for p in procs:
            if p.poll() is None:
                p.terminate()
        deadline = time.monotonic() + TERM_WAIT_S
        for p in procs:
            try:
                p.wait(timeout=max(0.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                p.kill()
        for p in procs:
            p.wait()


def main() -> int:
    import signal

    sup = _Supervisor(sys.stdout)
    signal.signal(signal.SIGTERM, lambda *_a: sys.exit(0))  # ends through the `finally` below
    buf = b""
    running = True
    try:
        while running:
            ready, _, _ = select.select([0], [], [], 0.05)
            if ready:
                data = os.read(0, 65536)
                if not data:
                    break  # the node is gone
                buf += data
                while running and b"\n" in buf:
                    line, buf = buf.split(b"\n", 1)
                    if line.strip():
                        running = sup.handle(line)
            sup.reap()
    except OSError:
        pass  # nobody reads the events any more (a broken pipe): the node is gone
    finally:
        sup.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
