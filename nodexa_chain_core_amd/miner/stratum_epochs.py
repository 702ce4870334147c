"""The epoch DAGs a Stratum server keeps for its own share checks (-stratumgpuverify=1).

A node that serves rigs without mining on its own GPU has no resident DAG: ops/verify's registry
holds what the in-process miner built and nothing else. `EpochOwner` fills that gap. The server
tells it the height of every job it serves (`note_job`); for the job's epoch, and for the next one
once the height is within `LOOKAHEAD` blocks of the boundary, it asks the registry whether a DAG is
resident and, if none is and nobody else is building one, has ONE background thread build it: the
light cache first (host, then on the device: from then on the epoch's shares can go through the
light-mode kernel), then the DAG, then the registration. The build never runs under the registry's
lock and the thread that verifies shares never waits for it: `mode(epoch)` only reads.

The owner keeps at most `MAX_OWN` epochs that it built itself and drops its lowest ones beyond
that; it never drops a DAG it did not build (the registry's `drop` takes the object and removes it
only if that very object is still the registered one, so a DAG that the miner shared in place of
the owner's stays). A build that fails is logged once, the epoch is not tried again, and its shares
stay on the host.

Builder and registry are injected, so the policy is tested on the host with fakes
(tests/test_stratum_vardiff.py); `device_builder` / `VerifyRegistry` are the real ones
(tests/test_gpu_stratum_epoch.py).
"""
from __future__ import annotations

import threading
import time

from .. import core
from ..utils import log

_core = core()

LOOKAHEAD = 120   # blocks before an epoch boundary at which the next epoch's build begins
MAX_OWN = 2       # the current epoch and the next


class VerifyRegistry:
    """ops/verify's registry of resident DAGs, as the owner uses it."""

    def is_resident(self, device: int, epoch: int) -> bool:
        from ..ops import verify as V

        return V.is_resident(device, epoch)

    def register(self, device: int, epoch: int, e) -> bool:
        """True when `e` is what is registered now (the miner may have shared its own meanwhile)."""
        from ..ops import verify as V

        with V._epochs_lock:
            V.share_epoch(device, epoch, e)
            return V._epochs.get((device, epoch)) is e

    def drop(self, device: int, epoch: int, e) -> bool:
        from ..ops import verify as V

        return V.drop_resident(device, epoch, e)

    def resident(self, device: int) -> list[int]:
        from ..ops import verify as V

        return [e.epoch for e in V.resident_dags(device)]


class device_builder:
    """The real builder: `light(epoch)` puts the epoch's light cache on the device (ops/verify's
    light epochs, which `gpu_full_hash(mode="light")` reads), `build(epoch)` returns the built
    DeviceEpoch. Everything is queued on one side stream of the builder's own and waited for there;
    with `dag_check` (-dagcheck=1) the build is the checked one (sampled audit, seal)."""

    def __init__(self, device: int, dag_check: bool = True):
        self.device = int(device)
        self.dag_check = bool(dag_check)
        self._stream = None

    def light(self, epoch: int) -> None:
        from ..ops import verify as V

        _core.get_epoch_context(epoch)  # the serial host build; the native LRU hands it on below
        V.light_epoch(epoch, self.device)

    def build(self, epoch: int):
        import torch

        from ..ops.ethash import DeviceEpoch

        with torch.cuda.device(self.device):
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(self._stream):
                e = DeviceEpoch(epoch, device=self.device)
                check = e.build_checked() if self.dag_check else e.build()
                self._stream.synchronize()
                if not e.l1_matches():
                    raise RuntimeError(f"gpu{self.device}: epoch {epoch} DAG failed its L1 self-check")
                if check is not None:
                    check.finish()  # raises RuntimeError when the DAG cannot be made right
                    self._stream.synchronize()
        return e


class EpochOwner:
    def __init__(self, device: int, builder, registry=None, foreign_pending=None):
        """`builder`: an object with `build(epoch) -> DAG object` and optionally `light(epoch)`.
        `foreign_pending(epoch) -> bool`: somebody else (the in-process miner's prebuild) is
        already building that epoch, so the owner leaves it alone."""
        self.device = int(device)
        self.builder = builder
        self.registry = registry if registry is not None else VerifyRegistry()
        self.foreign_pending = foreign_pending
        self.lock = threading.Lock()        # everything below
        self.own: dict[int, object] = {}    # epoch -> the DAG object this owner built and registered
        self.light_ready: set[int] = set()
        self.failed: set[int] = set()
        self.wanted: list[int] = []         # epochs waiting for the build thread, in order
        self.building: int | None = None
        self.stats = {"dag_builds": 0, "dag_build_failures": 0, "dag_last_build_ms": 0.0}
        self._thread: threading.Thread | None = None
        self._stop = False

    # ------------------------------------------------------------------ called by the server
    def note_job(self, height: int) -> None:
        """The server serves a job of this height: see to its epoch, and to the next one when the
        boundary is `LOOKAHEAD` blocks away or less. Returns at once."""
        epoch = int(height) // _core.EPOCH_LENGTH
        want = [epoch]
        if (epoch + 1) * _core.EPOCH_LENGTH - int(height) <= LOOKAHEAD:
            want.append(epoch + 1)
        with self.lock:
            if self._stop:
                return
            for e in want:
                if e in self.failed or e in self.wanted or e == self.building or e in self.own:
                    continue
                if self._covered(e):
                    continue
                self.wanted.append(e)
            if self.wanted and self._thread is None:
                self._thread = threading.Thread(target=self._run, name="stratum-dag", daemon=True)
                self._thread.start()

    def mode(self, epoch: int) -> str:
        """How a share of `epoch` is hashed now: "dag", "light" (the light-mode kernel) or "host"."""
        if self.registry.is_resident(self.device, epoch):
            return "dag"
        with self.lock:
            return "light" if epoch in self.light_ready and epoch not in self.failed else "host"

    def ready(self, epoch: int) -> bool:
        return self.registry.is_resident(self.device, epoch)

    def idle(self) -> bool:
        with self.lock:
            return self.building is None and not self.wanted

    def info(self) -> dict:
        with self.lock:
            out = dict(self.stats)
        out["epochs_resident"] = sorted(self.registry.resident(self.device))
        return out

    def own_epochs(self) -> list[int]:
        with self.lock:
            return sorted(self.own)

    def stop(self, timeout: float = 60.0) -> None:
        """No further build starts; waits for the one that runs, then gives up the owner's DAGs."""
        with self.lock:
            self._stop = True
            self.wanted.clear()
            t = self._thread
        if t is not None:
            t.join(timeout)
        with self.lock:
            mine, self.own = list(self.own.items()), {}
            self.light_ready.clear()
        for k, e in mine:
            self.registry.drop(self.device, k, e)

    # ------------------------------------------------------------------ the build thread
    def _covered(self, epoch: int) -> bool:
        if self.registry.is_resident(self.device, epoch):
            return True
        return bool(self.foreign_pending is not None and self.foreign_pending(epoch))

    def _run(self) -> None:
        while True:
            with self.lock:
                if not self.wanted or self._stop:
                    self._thread = None
                    return
                epoch = self.wanted.pop(0)
                if self._covered(epoch):  # the miner shared it while it waited here
                    continue
                self.building = epoch
            try:
                self._build(epoch)
            except Exception as e:  # noqa: BLE001 — a share check never depends on this build
                with self.lock:
                    self.failed.add(epoch)
                    self.light_ready.discard(epoch)
                    self.stats["dag_build_failures"] += 1
                log.log_printf(f"stratum: building the epoch {epoch} DAG for share checks failed "
                               f"({type(e).__name__}: {e}); its shares are checked on the host")
            finally:
                with self.lock:
                    self.building = None

    def _build(self, epoch: int) -> None:
        t0 = time.perf_counter()
        light = getattr(self.builder, "light", None)
        if light is not None:
            light(epoch)
            with self.lock:
                self.light_ready.add(epoch)
        e = self.builder.build(epoch)
        mine = self.registry.register(self.device, epoch, e)  # built first, registered then
        with self.lock:
            if mine:
                self.own[epoch] = e
            self.stats["dag_builds"] += 1
            self.stats["dag_last_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            drop = [(k, self.own.pop(k)) for k in sorted(self.own)[:max(0, len(self.own) - MAX_OWN)]]
            for k, _ in drop:
                self.light_ready.discard(k)
        for k, old in drop:
            self.registry.drop(self.device, k, old)
