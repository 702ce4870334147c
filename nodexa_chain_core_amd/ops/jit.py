"""Per-period KawPow kernel compilation (the hipRTC-style JIT of SURVEY §7.3).

A ProgPoW period lasts 3 blocks. For each period the C++ generator
(`_core.kawpow_codegen_hip`, csrc/pow/kawpow_codegen.cpp) emits the period's
straight-line program; it is compiled together with
hip/kernels/kawpow_search.hip into a gfx950 code object by the offline
compiler (`hipcc --genco`, run as a child process — never exec'd in place of
a GPU process). Objects are cached on disk keyed by (period, arch, template
hash), so a restart or the next run of the same height reuses them, and
`prefetch()` compiles the next period on a worker thread while the current one
is mining.
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import tempfile
import threading

from .. import _build, _core

TEMPLATE = os.path.join(_build.HIPDIR, "kernels", "kawpow_search.hip")
CACHE_DIR = os.environ.get("NODEXA_KERNEL_CACHE", os.path.join(_build.PKG, "..", ".kernel_cache"))
_pool = cf.ThreadPoolExecutor(max_workers=2, thread_name_prefix="kawpow-jit")
_lock = threading.Lock()
_inflight: dict[tuple, cf.Future] = {}


_INCLUDE = re.compile(rb'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def template_files(template: str | None = None) -> list[str]:
    """The template and every project file it includes, directly or not: `#include "..."` followed
    inside the template's directory, each file once, in the order first met. The period's program
    (`#include KAWPOW_PROGRAM_HEADER`) names no file here; object_path keys it by its text."""
    template = TEMPLATE if template is None else template
    kdir = os.path.dirname(template)
    files, todo = [], [os.path.basename(template)]
    while todo:
        name = todo.pop(0)
        if name in files:
            continue
        files.append(name)
        with open(os.path.join(kdir, name), "rb") as f:
            todo += [m.decode() for m in _INCLUDE.findall(f.read())]
    return [os.path.join(kdir, name) for name in files]


def _template_digest(template: str | None = None) -> str:
    h = hashlib.sha256()
    for path in template_files(template):
        with open(path, "rb") as f:
            h.update(f.read())
    h.update(_build.ARCH.encode())
    return h.hexdigest()[:16]


def _variant_tag(defines: tuple[str, ...]) -> str:
    if not defines:
        return ""
    return "_v" + hashlib.sha256("|".join(sorted(defines)).encode()).hexdigest()[:8]


def object_path(period: int, defines: tuple[str, ...] = ()) -> str:
    # the key covers the template, the generated program text (codegen changes) and the variant
    prog = hashlib.sha256(program_source(period).encode()).hexdigest()[:8]
    return os.path.join(os.path.abspath(CACHE_DIR),
                        f"kawpow_p{period}_{_build.ARCH}_{_template_digest()}{prog}{_variant_tag(defines)}.hsaco")


def program_source(period: int) -> str:
    return _core.kawpow_codegen_hip(period)


def compile_period(period: int, defines: tuple[str, ...] = ()) -> str:
    """Compile (or reuse) the code object for `period`; returns its path.

    `defines` selects tuning variants of the template (e.g. "KP_MIN_WAVES=6")."""
    out = object_path(period, defines)
    if os.path.exists(out):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="kawpow_jit_") as tmp:
        inc = os.path.join(tmp, f"kawpow_program_p{period}.inc")
        with open(inc, "w") as f:
            f.write(program_source(period))
        tmp_out = os.path.join(tmp, "k.hsaco")
        _build.hipcc_genco(TEMPLATE, tmp_out, defines=[f'KAWPOW_PROGRAM_HEADER="{inc}"', *defines])
        _atomic_copy(tmp_out, out)
    return out


def _atomic_copy(src: str, dst: str) -> None:
    tmp = dst + f".tmp{os.getpid()}"
    with open(src, "rb") as a, open(tmp, "wb") as b:
        b.write(a.read())
    os.replace(tmp, dst)


# Tuned variant of the search template (profiles/README.md has the sweep that
# picked it); NODEXA_KAWPOW_DEFINES="A,B=1" overrides it ("none" = plain template).
# r2l / r2m: digests held in registers (the only digest form since r4b) leave only the 64 KiB L1 table in LDS, so
# two 768-thread workgroups share a CU (6 waves/SIMD instead of 4): +0.7 / +0.8 % in two
# interleaved sweeps; 640 / 896 threads (waves uneven across the 4 SIMDs) and 1024 (64 VGPRs,
# heavy spills) lose.
# r3b / r3c: scheduling fences around each round's cache/math program (KP_SCHED_FENCE) keep the
# DAG merge, and with it the wait for the round's HBM gather, at the end of the round: +3.2 / +3.6 %
# in two interleaved 7-round sweeps (profiles/r3b_r3c_sched_fence).
TUNED_DEFINES: tuple[str, ...] = ("KP_HASHES=1", "KP_DPP", "KP_BARRETT", "KP_SBUFFER", "KP_L1X4", "KP_BLOCK=768",
                                  "KP_MIN_WAVES=6", "KP_NT_DAG", "KP_SCHED_FENCE")
_env = os.environ.get("NODEXA_KAWPOW_DEFINES")
DEFAULT_DEFINES: tuple[str, ...] = TUNED_DEFINES if _env is None else tuple(
    d for d in _env.split(",") if d and d != "none")


def defines_for(dag_bytes: int, defines: tuple[str, ...] | None = None) -> tuple[str, ...]:
    """The variant to compile for a DAG of `dag_bytes`: KP_SBUFFER addresses the DAG with 32-bit
    buffer offsets, so for DAGs of 4 GiB or more (epochs >= 385; measured there: the structured
    form is not bit-exact) it becomes KP_PTR64 (64-bit addresses by one v_mad_u64_u32), at the
    same 768 threads / 6 waves per SIMD: profiles/r6_dag_over_4g, epoch 390, 273.0 MH/s against
    268.6 for the 512-thread pointer form it replaces and 283.3 for the buffer form at epoch 384 on
    the same box (1.2 % of that gap is the larger DAG itself: KP_PTR64 at epoch 384 runs 276.4)."""
    d = DEFAULT_DEFINES if defines is None else tuple(defines)
    if dag_bytes >= 1 << 32 and "KP_SBUFFER" in d:  # 32-bit buffer offsets: 64-bit addresses
        d = tuple("KP_PTR64" if x == "KP_SBUFFER" else x for x in d)
    return d


def prefetch(period: int, defines: tuple[str, ...] | None = None) -> cf.Future:
    """Start compiling `period` in the background (idempotent)."""
    defines = DEFAULT_DEFINES if defines is None else tuple(defines)
    key = (period, defines)
    with _lock:
        fut = _inflight.get(key)
        if fut is None:
            fut = _pool.submit(compile_period, period, defines)
            _inflight[key] = fut
        return fut


def get(period: int, defines: tuple[str, ...] | None = None) -> str:
    return prefetch(period, defines).result()


def ready(period: int, defines: tuple[str, ...] | None = None) -> str | None:
    """The path of `period`'s code object if it can be loaded now, else None; never blocks and
    never starts a compile. Ready = its compile future finished without error, or (no compile
    running in this process) the cache file exists."""
    defines = DEFAULT_DEFINES if defines is None else tuple(defines)
    with _lock:
        fut = _inflight.get((period, defines))
    if fut is not None:
        if not fut.done():
            return None
        if fut.exception() is None:
            return fut.result()
    path = object_path(period, defines)
    return path if os.path.exists(path) else None


DEFAULT_BLOCK = 256  # NODEXA_KAWPOW_BLOCK (kernel_params.h): the template's KP_BLOCK when no define sets it


def granule_for(dag_bytes: int, defines: tuple[str, ...] | None = None) -> int:
    """Nonce granularity of a search launch over a DAG of `dag_bytes`: the KP_BLOCK of the variant
    `defines_for` picks, i.e. the workgroup size of the specialised kernel. The period-agnostic
    kernel cuts its launches the same way, so a window is the same whichever kernel runs it."""
    for d in defines_for(dag_bytes, defines):
        if d.startswith("KP_BLOCK="):
            return int(d.split("=", 1)[1])
    return DEFAULT_BLOCK


JIT_MODES = ("wait", "auto", "off")
JIT_FLAG_HINT = "-kawpowjit=auto (or off) mines on the period-agnostic kernel without the compiler"


class KernelChoice:
    """What `KernelChooser.choose` decided for one period."""
    __slots__ = ("kind", "path", "log")

    def __init__(self, kind: str, path: str | None = None, log: str | None = None):
        self.kind = kind  # "jit": load `path`; "generic": the period-agnostic kernel
        self.path = path
        self.log = log    # a line to log now (at most one per period), or None

    def __repr__(self) -> str:
        return f"KernelChoice({self.kind!r}, {self.path!r}, {self.log!r})"


class KernelChooser:
    """Which search kernel a period runs on: the per-period compiled one ("jit") or the
    period-agnostic one ("generic"). No GPU, no compiler: it only sees two callables.

      ready(period) -> path | None     non-blocking: the period's object can be loaded now
      start_compile(period) -> Future  start (or join) the period's compile; result() = the path

    wait: block on the compile (the behaviour before there was a choice). auto: jit when the
    object is there, else start ONE compile for the period and answer generic until its future
    is done; a compile that fails (or cannot start: no compiler) is logged once and the period
    stays on generic, with no second attempt. off: always generic, never compiles."""

    KEEP = 64  # periods remembered (paths, failures): a chain moves one period per 3 blocks

    def __init__(self, mode: str, ready, start_compile):
        if mode not in JIT_MODES:
            raise ValueError(f"kawpow jit mode must be one of {', '.join(JIT_MODES)}, not {mode!r}")
        self.mode = mode
        self._ready = ready
        self._start = start_compile
        self._paths: dict[int, str] = {}
        self._futs: dict[int, object] = {}
        self._failed: dict[int, str] = {}

    def pending(self, period: int):
        """The compile future `period` is waiting on (auto), or None."""
        return self._futs.get(period)

    def _jit(self, period: int, path: str) -> KernelChoice:
        self._paths[period] = path
        while len(self._paths) > self.KEEP:
            self._paths.pop(next(iter(self._paths)))
        return KernelChoice("jit", path)

    def _fail(self, period: int, err: BaseException) -> KernelChoice:
        self._failed[period] = f"{type(err).__name__}: {err}"
        while len(self._failed) > self.KEEP:
            self._failed.pop(next(iter(self._failed)))
        return KernelChoice("generic", None, f"kawpow: no compiled kernel for period {period} ({self._failed[period]}); "
                                             "staying on the period-agnostic kernel")

    def choose(self, period: int) -> KernelChoice:
        path = self._paths.get(period)
        if path is not None:
            return KernelChoice("jit", path)
        if self.mode == "off":
            return KernelChoice("generic")
        if self.mode == "wait":
            try:
                return self._jit(period, self._start(period).result())
            except FileNotFoundError as e:  # no compiler on this machine
                raise FileNotFoundError(f"{e}: the KawPow per-period kernel needs hipcc; {JIT_FLAG_HINT}") from e
        if period in self._failed:
            return KernelChoice("generic")
        fut = self._futs.get(period)
        if fut is None:
            path = self._ready(period)
            if path is not None:
                return self._jit(period, path)
            try:
                fut = self._start(period)
            except Exception as e:
                return self._fail(period, e)
            self._futs[period] = fut
            while len(self._futs) > self.KEEP:  # periods the chain left before their compile ended
                self._futs.pop(next(iter(self._futs)))
        if not fut.done():
            return KernelChoice("generic")
        del self._futs[period]
        err = fut.exception()
        if err is not None:
            return self._fail(period, err)
        return self._jit(period, fut.result())


def hipcc_available() -> bool:
    try:
        subprocess.run([os.path.join(_build.ROCM, "bin", "hipcc"), "--version"], capture_output=True, check=True)
        return True
    except (OSError, subprocess.CalledProcessError):
        return False
