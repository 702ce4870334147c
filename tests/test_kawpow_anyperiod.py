"""Period-agnostic KawPow search, the parts that need no GPU: the built code object, the kernel
choice (wait / auto / off), the -kawpowjit flag and the launch granule."""
import concurrent.futures as cf
import os
import re
import subprocess
import tempfile
import threading

import pytest

from test_node_rpc import node_factory  # noqa: F401 — shared fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------- build
def _kernel_metadata(hsaco: str) -> tuple[dict[str, dict[str, str]], str]:
    """({kernel name: {metadata key: value}}, target) from the code object's AMDGPU metadata note."""
    from nodexa_chain_core_amd.ops import jump_slots

    with tempfile.TemporaryDirectory() as tmp:
        obj = jump_slots._code_object(hsaco, tmp)
        notes = subprocess.run([os.path.join(jump_slots.LLVM, "llvm-readelf"), "--notes", obj],
                               capture_output=True, text=True, check=True).stdout
    # amdhsa.kernels is a list at two spaces of indent; a kernel's own keys sit at four
    kernels, cur, target = {}, None, ""
    for line in notes.splitlines():
        if line.startswith("amdhsa.target:"):
            target = line.split(":", 1)[1].strip()
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)
        if line.startswith("  - "):
            cur = {}
        if m and cur is not None:
            cur[m.group(2)] = m.group(3).strip()
            if m.group(2) == ".name":
                kernels[m.group(3).strip()] = cur
    return kernels, target


def test_build_produces_scratch_free_search_any(core):
    from nodexa_chain_core_amd import _build
    from nodexa_chain_core_amd.ops import jump_slots

    if not os.path.exists(os.path.join(_build.ROCM, "bin", "hipcc")):
        pytest.fail("no hipcc: the static gfx950 code objects cannot be built")
    outs = _build.build_kernels()
    path = os.path.join(_build.PKG, "kernels", "kawpow_anyperiod.hsaco")
    assert any(os.path.samefile(path, o) for o in outs)
    assert _build.ARCH == "gfx950"
    if not os.path.exists(os.path.join(jump_slots.LLVM, "llvm-readelf")):
        pytest.fail("llvm-readelf missing: cannot read the kernel metadata")
    meta, target = _kernel_metadata(path)
    assert target.endswith("gfx950"), target
    assert "kawpow_search_any" in meta and "kawpow_hash_any" in meta, sorted(meta)
    k = meta["kawpow_search_any"]
    assert int(k[".private_segment_fixed_size"]) == 0  # no scratch: the mix stays in registers
    assert int(k[".max_flat_workgroup_size"]) == 256
    assert int(k[".group_segment_fixed_size"]) <= 16384 + 64  # the L1 and the stale word
    assert "kawpow_anyperiod" not in jump_slots.STAMPED  # loads without a jump-slot stamp


# ---------------------------------------------------------------------------- choice logic
class Fakes:
    def __init__(self, on_disk=()):
        self.on_disk = set(on_disk)
        self.futures: dict[int, cf.Future] = {}
        self.started: list[int] = []
        self.ready_calls = 0
        self.start_raises = None

    def ready(self, period):
        self.ready_calls += 1
        return f"/cache/p{period}.hsaco" if period in self.on_disk else None

    def start(self, period):
        self.started.append(period)
        if self.start_raises is not None:
            raise self.start_raises
        return self.futures.setdefault(period, cf.Future())


def _chooser(mode, f):
    from nodexa_chain_core_amd.ops.jit import KernelChooser

    return KernelChooser(mode, f.ready, f.start)


def test_chooser_rejects_unknown_mode():
    with pytest.raises(ValueError, match="wait, auto, off"):
        _chooser("bogus", Fakes())


def test_chooser_wait_blocks_until_compiled():
    entered, release = threading.Event(), threading.Event()

    class Blocking(cf.Future):
        def result(self, timeout=None):
            entered.set()  # the chooser is inside the wait
            assert release.wait(10)
            return super().result(timeout)

    f = Fakes()
    f.futures[7] = Blocking()
    c = _chooser("wait", f)
    out = []
    t = threading.Thread(target=lambda: out.append(c.choose(7)))
    t.start()
    assert entered.wait(10)
    assert t.is_alive() and not out and f.started == [7]  # blocked on the compile it started
    f.futures[7].set_result("/cache/p7.hsaco")
    release.set()
    t.join(10)
    assert not t.is_alive()
    assert (out[0].kind, out[0].path, out[0].log) == ("jit", "/cache/p7.hsaco", None)
    assert c.choose(7).kind == "jit" and f.started == [7]


def test_chooser_wait_names_the_flag_without_compiler():
    f = Fakes()
    c = _chooser("wait", f)
    f.futures[3] = cf.Future()
    f.futures[3].set_exception(FileNotFoundError(2, "No such file or directory", "/opt/rocm/bin/hipcc"))
    with pytest.raises(FileNotFoundError, match="-kawpowjit=auto"):
        c.choose(3)


def test_chooser_auto_generic_then_jit_one_compile():
    f = Fakes()
    c = _chooser("auto", f)
    for _ in range(5):
        r = c.choose(10)
        assert (r.kind, r.path, r.log) == ("generic", None, None)
    assert f.started == [10] and c.pending(10) is f.futures[10]
    f.futures[10].set_result("/cache/p10.hsaco")
    r = c.choose(10)
    assert (r.kind, r.path, r.log) == ("jit", "/cache/p10.hsaco", None)
    assert c.choose(10).kind == "jit"
    assert f.started == [10] and c.pending(10) is None


def test_chooser_auto_uses_object_on_disk_without_compiling():
    f = Fakes(on_disk={4})
    c = _chooser("auto", f)
    r = c.choose(4)
    assert (r.kind, r.path) == ("jit", "/cache/p4.hsaco") and f.started == []


def test_chooser_auto_failed_compile_logs_once_no_retry():
    f = Fakes()
    c = _chooser("auto", f)
    assert c.choose(20).kind == "generic"
    f.futures[20].set_exception(RuntimeError("build failed: boom"))
    r = c.choose(20)
    assert r.kind == "generic" and r.log and "period 20" in r.log and "boom" in r.log
    for _ in range(4):
        r = c.choose(20)
        assert (r.kind, r.log) == ("generic", None)
    assert f.started == [20]
    # another period still gets its own single attempt
    assert c.choose(21).kind == "generic" and f.started == [20, 21]


def test_chooser_auto_no_compiler_logs_once_no_retry():
    f = Fakes()
    f.start_raises = FileNotFoundError(2, "No such file or directory", "hipcc")
    c = _chooser("auto", f)
    r = c.choose(30)
    assert r.kind == "generic" and r.log and "period 30" in r.log
    for _ in range(3):
        r = c.choose(30)
        assert (r.kind, r.log) == ("generic", None)
    assert f.started == [30]


def test_chooser_off_never_compiles():
    f = Fakes(on_disk={1})
    c = _chooser("off", f)
    for p in (1, 2, 1, 3):
        r = c.choose(p)
        assert (r.kind, r.path, r.log) == ("generic", None, None)
    assert f.started == [] and f.ready_calls == 0


def test_chooser_back_to_a_ready_period_is_jit_at_once():
    f = Fakes()
    c = _chooser("auto", f)
    assert c.choose(40).kind == "generic"
    f.futures[40].set_result("/cache/p40.hsaco")
    assert c.choose(40).kind == "jit"
    assert c.choose(41).kind == "generic"  # the chain moves on: 41 is not compiled yet
    calls = f.ready_calls
    r = c.choose(40)  # a reorg back to 40
    assert (r.kind, r.path) == ("jit", "/cache/p40.hsaco")
    assert f.started == [40, 41] and f.ready_calls == calls  # no compile, not even a disk check
    # 41's compile finished while the chain sat on 40; a period never seen but on disk is jit too
    f.futures[41].set_result("/cache/p41.hsaco")
    assert c.choose(41).kind == "jit"
    f.on_disk.add(39)
    assert c.choose(39).kind == "jit" and f.started == [40, 41]


def test_jit_ready_is_non_blocking(core, tmp_path, monkeypatch):
    from nodexa_chain_core_amd.ops import jit

    monkeypatch.setattr(jit, "CACHE_DIR", str(tmp_path))
    monkeypatch.setattr(jit, "_inflight", {})
    period, defines = 123456, ("KP_BLOCK=512",)
    assert jit.ready(period, defines) is None  # nothing on disk, nothing in flight: no compile started
    assert jit._inflight == {}
    gate = threading.Event()

    def slow(p, d=()):
        gate.wait(10)
        out = jit.object_path(p, d)
        open(out, "wb").write(b"x")
        return out

    monkeypatch.setattr(jit, "compile_period", slow)
    fut = jit.prefetch(period, defines)
    assert jit.ready(period, defines) is None and not fut.done()
    gate.set()
    path = fut.result(10)
    assert jit.ready(period, defines) == path
    monkeypatch.setattr(jit, "_inflight", {})
    assert jit.ready(period, defines) == path  # from the cache file alone

    def broken(p, d=()):
        raise FileNotFoundError(2, "No such file or directory", "hipcc")

    monkeypatch.setattr(jit, "compile_period", broken)
    with pytest.raises(FileNotFoundError):
        jit.prefetch(period + 1, defines).result(10)
    assert jit.ready(period + 1, defines) is None


# ---------------------------------------------------------------------------- flag
def _args(*flags):
    from nodexa_chain_core_amd.utils.config import ArgsManager

    a = ArgsManager()
    a.parse_parameters(list(flags))
    return a


def test_flag_values():
    from nodexa_chain_core_amd.utils.config import kawpow_jit_mode

    assert kawpow_jit_mode(_args()) == "wait"
    for m in ("wait", "auto", "off"):
        assert kawpow_jit_mode(_args(f"-kawpowjit={m}")) == m
    with pytest.raises(ValueError, match="-kawpowjit=bogus"):
        kawpow_jit_mode(_args("-kawpowjit=bogus"))


def test_node_refuses_unknown_kawpowjit(core, node_factory):  # noqa: F811
    with pytest.raises(SystemExit, match="-kawpowjit=bogus"):
        node_factory(("-kawpowjit=bogus",))


def test_remote_miner_refuses_unknown_kawpowjit(core, monkeypatch):
    from nodexa_chain_core_amd.miner import remote, service

    def not_refused(*args, **kwargs):  # a miner that takes the value would build its device and mine on
        raise AssertionError("-kawpowjit=bogus was not refused before the device was made")

    monkeypatch.setattr(service, "make_rank_device", not_refused)
    monkeypatch.setattr(remote.RemoteMiner, "run", not_refused)
    with pytest.raises(SystemExit, match="-kawpowjit=bogus"):
        remote.main(["-regtest", "-cpu", "-kawpowjit=bogus"])


@pytest.mark.parametrize("mode", ["wait", "auto", "off"])
def test_flag_reaches_device_and_followers(core, monkeypatch, mode):
    from nodexa_chain_core_amd.miner import search, service
    from nodexa_chain_core_amd.utils.config import kawpow_jit_mode

    seen = {}

    class FakeGpu:
        name, device = "gpu", 0

        def __init__(self, device=0, collective_dag=False, jit_mode="wait"):
            seen.update(device=device, jit_mode=jit_mode)

    monkeypatch.setattr(search, "GpuSearchDevice", FakeGpu)
    got = kawpow_jit_mode(_args(f"-kawpowjit={mode}"))
    service.make_rank_device(False, 0, jit_mode=got)
    assert seen == {"device": 0, "jit_mode": mode}
    # the follower ranks get it through their environment and hand it to their own device
    env = service.follower_env(timeout=60.0, watchdog="120", max_failures=3, fail_rate=0.0, drop_rate=0.0,
                               jit_mode=got)
    assert env["NODEXA_MINER_KAWPOWJIT"] == mode
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert service.follower_jit_mode() == mode
    monkeypatch.setenv("NODEXA_MINER_KAWPOWJIT", "bogus")
    with pytest.raises(ValueError, match="bogus"):
        service.follower_jit_mode()
    monkeypatch.delenv("NODEXA_MINER_KAWPOWJIT")
    assert service.follower_jit_mode() == "wait"


def test_gpu_device_refuses_unknown_mode(core):
    from nodexa_chain_core_amd.miner.search import GpuSearchDevice

    with pytest.raises(ValueError, match="wait, auto, off"):
        GpuSearchDevice(0, jit_mode="bogus")  # refused before it looks for a GPU


def test_record_carries_kernel_kind(core):
    from nodexa_chain_core_amd.miner import service
    from nodexa_chain_core_amd.miner.search import SlotResult

    size = service.RECORD_SIZE
    assert size == 5592  # the kind rides in the status bits: the record did not grow
    for kind in ("jit", "generic", ""):
        raw = service.pack_record(SlotResult(5, 0, 768, 768, [], 1.0, kernel=kind))
        assert len(raw) == size
        rec = service.unpack_record(raw)
        assert (rec.kernel, rec.has_result, rec.alive, rec.hashes) == (kind, True, True, 768)
    assert service.unpack_record(service.pack_record(None)).kernel == ""


# ---------------------------------------------------------------------------- granule
def test_granule_is_the_jit_block(core, monkeypatch):
    from nodexa_chain_core_amd.ops import jit

    def kp_block(defines):
        return next(int(d.split("=")[1]) for d in defines if d.startswith("KP_BLOCK="))

    below, above = (1 << 32) - 256, (1 << 32) + 256
    for dag_bytes in (1 << 30, below, 1 << 32, above):
        assert jit.granule_for(dag_bytes) == kp_block(jit.defines_for(dag_bytes)) == 768
    assert "KP_SBUFFER" in jit.defines_for(below) and "KP_PTR64" in jit.defines_for(above)
    override = tuple("KP_BLOCK=512" if d.startswith("KP_BLOCK=") else d for d in jit.TUNED_DEFINES)
    monkeypatch.setattr(jit, "DEFAULT_DEFINES", override)
    for dag_bytes in (below, above):
        assert jit.granule_for(dag_bytes) == kp_block(jit.defines_for(dag_bytes)) == 512
    monkeypatch.setattr(jit, "DEFAULT_DEFINES", ())  # NODEXA_KAWPOW_DEFINES=none: the template's own block
    assert jit.granule_for(below) == 256


def test_granule_follows_the_environment_override(core):
    """NODEXA_KAWPOW_DEFINES is read when ops/jit.py is imported: a fresh interpreter."""
    code = ("from nodexa_chain_core_amd.ops import jit; d = jit.defines_for(5 << 30); "
            "print(jit.granule_for(1 << 30), jit.granule_for(5 << 30), 'KP_BLOCK=512' in d, 'KP_PTR64' in d)")
    env = dict(os.environ, NODEXA_KAWPOW_DEFINES="KP_HASHES=1,KP_DPP,KP_BARRETT,KP_SBUFFER,KP_L1X4,KP_BLOCK=512")
    out = subprocess.run([os.sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["512", "512", "True", "True"]


# ---------------------------------------------------------------------------- node surfaces
def test_node_reports_kernel_kind_per_rank(core, node_factory):  # noqa: F811
    """getmininginfo.gpus[] / getgpuinfo and the metrics registry carry the kernel of each rank's
    windows. A CPU node has no GPU kernel to report, so the host device's results are tagged here
    the way GpuSearchDevice tags its own: two generic windows, then compiled ones."""
    from nodexa_chain_core_amd.utils.metrics import REGISTRY
    from test_node_rpc import client

    node, addr = node_factory(("-kawpowjit=auto",))
    c = client(node)
    first = c.getmininginfo()["gpus"][0]
    assert (first["kernel"], first["generic_windows"], first["jit_windows"]) == ("", 0, 0)
    dev = node.miner.service.dev.kawpow
    inner, seen = dev.wait, []

    def tagged(slot, timeout_s=None):
        res = inner(slot, timeout_s)
        res.kernel = "generic" if len(seen) < 2 else "jit"
        seen.append(res.kernel)
        return res

    dev.wait = tagged
    before = {k: REGISTRY.counter(f"miner_kawpow_{k}_windows_total", worker="service") for k in ("jit", "generic")}
    assert len(c.generatetoaddress(4, addr)) == 4
    dev.wait = inner
    for info in (c.getmininginfo()["gpus"][0], c.getgpuinfo()[0]):
        assert info["kernel"] == "jit"
        assert info["generic_windows"] == 2 and info["jit_windows"] >= 1
        assert info["generic_windows"] + info["jit_windows"] <= info["windows"]
    assert REGISTRY.counter("miner_kawpow_generic_windows_total", worker="service") - before["generic"] == 2
    assert REGISTRY.counter("miner_kawpow_jit_windows_total", worker="service") - before["jit"] >= 1
