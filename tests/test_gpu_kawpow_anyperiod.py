"""kawpow_search_any / kawpow_hash_any (hip/kernels/kawpow_anyperiod.hip) and the wait / auto / off
kernel choice on the GPU. The oracle is never the code under test: whole windows are hashed by the
static resident-DAG batch kernel kawpow_verify_dag (every nonce of the window, filtered on the host
with the kernel's 64-bit prefix rule), single hashes by the CPU golden model."""
import threading

import pytest

from kawpow_vectors import VECTORS
from search_oracle import as_set, boundary_for, clear_cache, oracle_window

pytestmark = pytest.mark.gpu

HEADER = bytes(range(1, 33))
G = 768                                   # the tuned variants' KP_BLOCK: the launch granule
START = 0x0123456789AB0000 + 5 * G        # non-zero high and low words
PREFIX_128 = (1 << 64) // 128             # mean 12 shares in 2 granules
PREFIX_1024 = (1 << 64) // 1024           # mean 12 shares in 16 granules
# shares the oracle finds in [START, START + 2G) at PREFIX_128 (checked once, asserted below)
ORACLE_COUNTS = {0: 6, 3: 11, 49: 13, 50: 13, 99: 7, 7499: 16}
ORACLE_COUNT_BIG = 11                     # height 50, 16 granules, PREFIX_1024
ORACLE_COUNT_E385 = 9                     # height 2,887,500, 2 granules, PREFIX_128
E385_HEIGHT = 2_887_500


def build_epoch(core, epoch):
    import torch

    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

    e = DeviceEpoch(epoch, device=0, ctx=core.get_epoch_context(epoch))
    e.build()
    torch.cuda.synchronize()
    assert e.l1_matches()
    return e


@pytest.fixture(scope="module")
def epoch0(gpu, core):
    return build_epoch(core, 0)


def check_window(core, ep, height, granules, prefix, expect_count):
    """Test 2's check: the generic kernel's share set over one window against the oracle's."""
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher, parse_results

    n = granules * G
    want = oracle_window(ep, height, START, n, prefix)
    print(f"height {height}: oracle shares {len(want)} in {n} nonces")
    assert 1 <= len(want) <= 64  # the ring's capacity: above it the kernel may drop shares
    assert len(want) == expect_count
    s = KawpowSearcher(ep, height, jit_mode="off")
    assert s.block == G
    s.launch(HEADER, START, n, prefix)
    got = s.collect()
    _shares, count, skipped = parse_results(s.results_host.numpy().tobytes(), s.h.KAWPOW_MAX_SHARES)
    assert s.kernel_kind == "generic"
    assert as_set(got) == set(want)
    assert count == len(want) and skipped == 0
    for sh in got:
        assert sh.verify_full(height, HEADER, boundary_for(prefix), ctx=ep.ctx)


# ------------------------------------------------------------------ 1. vectors
def test_hash_batch_vectors_without_jit(core, epoch0):
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher

    vecs = [v for v in VECTORS if v[0] in (0, 49, 50, 99)]
    assert [v[0] for v in vecs] == [0, 49, 50, 99]
    s = KawpowSearcher(epoch0, 0, jit_mode="off")
    for block, header, nonce, mix, final in vecs:
        s.set_block(block)
        (f, m), = s.hash_batch([bytes.fromhex(header)], [int(nonce, 16)])
        assert (m.hex(), f.hex()) == (mix, final), block
    assert s.kernel is None and s.hash_kernel is None and s.kernel_kind == "generic"
    # a batch that is not a multiple of the block or of a 16-lane group, against the golden model
    heads = [i.to_bytes(2, "little") * 16 for i in range(300)]
    nonces = [(i * 0x9E3779B97F4A7C15) & (2**64 - 1) for i in range(300)]
    out = s.hash_batch(heads, nonces)
    for i in (0, 15, 16, 255, 256, 299):
        assert out[i] == core.kawpow_hash(epoch0.ctx, 99, heads[i], nonces[i]), i


# ------------------------------------------------------------------ 2. share set == oracle
@pytest.mark.parametrize("height", [0, 3, 49, 50, 99, 7499])
def test_share_set_equals_oracle(core, epoch0, height):
    check_window(core, epoch0, height, 2, PREFIX_128, ORACLE_COUNTS[height])


# ------------------------------------------------------------------ 3. larger window
def test_larger_window(core, epoch0):
    check_window(core, epoch0, 50, 16, PREFIX_1024, ORACLE_COUNT_BIG)


# ------------------------------------------------------------------ 4. stale work
def test_stale_work_searches_nothing(core, epoch0, monkeypatch):
    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, Work
    from nodexa_chain_core_amd.ops.kawpow import parse_results

    want = oracle_window(epoch0, 50, START, 2 * G, PREFIX_128)
    dev = GpuSearchDevice(0, jit_mode="off")
    try:
        dev.epochs[0] = epoch0
        work = Work(HEADER, boundary_for(PREFIX_128), 50, job_id=9, flags=0)
        dev.generation = 5  # the host word still says 0: every workgroup finds its launch stale
        dev.submit(0, work, START, 2 * G)
        res = dev.wait(0)
        _s, count, skipped = parse_results(dev.host[0].numpy().tobytes(), dev.h.KAWPOW_MAX_SHARES)
        assert count == 0 and skipped == 2  # one workgroup per granule
        assert (res.hashes, res.aborted, res.shares, res.kernel) == (0, 2, [], "generic")
        dev.h.host_word_store(dev.gen_ptr, 0, 5)
        dev.submit(1, work, START, 2 * G)
        res = dev.wait(1)
        assert (res.hashes, res.aborted) == (2 * G, 0)
        assert as_set(res.shares) == set(want) and want
    finally:
        dev.close()


# ------------------------------------------------------------------ 5. DAG above 4 GiB
def test_dag_above_4gib(core, gpu):
    import torch

    ep = build_epoch(core, E385_HEIGHT // 7500)
    try:
        assert ep.dag_bytes >= 1 << 32
        check_window(core, ep, E385_HEIGHT, 2, PREFIX_128, ORACLE_COUNT_E385)
    finally:
        clear_cache()
        del ep
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 6. no compiler
def _no_compiler(monkeypatch, tmp_path):
    from nodexa_chain_core_amd.ops import jit

    def missing(period, defines=()):
        raise FileNotFoundError(2, "No such file or directory", "hipcc")

    monkeypatch.setattr(jit, "compile_period", missing)
    monkeypatch.setattr(jit, "_inflight", {})
    monkeypatch.setattr(jit, "CACHE_DIR", str(tmp_path))  # no object of an earlier run either


@pytest.mark.parametrize("mode", ["auto", "off"])
def test_no_compiler_mines_on_generic(core, epoch0, monkeypatch, tmp_path, mode):
    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, SearchPipeline, Work

    _no_compiler(monkeypatch, tmp_path)
    dev = GpuSearchDevice(0, jit_mode=mode)
    try:
        dev.epochs[0] = epoch0
        work = Work(HEADER, boundary_for(PREFIX_128), 50, job_id=1, flags=0)
        pipe = SearchPipeline(dev)
        assert pipe.step(work, START, 2 * G) is None
        results = [pipe.step(work, START + 2 * G, 2 * G), pipe.drain()]
        for k, res in enumerate(results):
            want = oracle_window(epoch0, 50, START + k * 2 * G, 2 * G, PREFIX_128)
            assert (res.start, res.count, res.hashes, res.kernel) == (START + k * 2 * G, 2 * G, 2 * G, "generic")
            assert as_set(res.shares) == set(want)
        assert dev.kernel_kind == "generic" and dev.searchers[0].kernel_kind == "generic"
    finally:
        dev.close()


def test_no_compiler_wait_raises_and_names_the_flag(core, epoch0, monkeypatch, tmp_path):
    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, Work

    _no_compiler(monkeypatch, tmp_path)
    dev = GpuSearchDevice(0, jit_mode="wait")
    try:
        dev.epochs[0] = epoch0
        with pytest.raises(FileNotFoundError, match="-kawpowjit=auto"):
            dev.submit(0, Work(HEADER, boundary_for(PREFIX_128), 50, job_id=1, flags=0), START, 2 * G)
    finally:
        dev.close()


# ------------------------------------------------------------------ 7. hot swap
COMPILE_LIMIT_S = 60  # one hipcc run of the tuned variant takes about 5 s (profiles/README.md): 12x headroom


def test_hot_swap_generic_to_jit(core, epoch0, monkeypatch, tmp_path):
    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, SearchPipeline, Work
    from nodexa_chain_core_amd.ops import jit

    height = 2000 * 3 + 1  # epoch 0; a period no other test compiles
    period = height // 3
    gate = threading.Event()
    real = jit.compile_period

    def gated(p, defines=()):
        if p != period:
            raise RuntimeError("only one period is compiled in this test")
        assert gate.wait(COMPILE_LIMIT_S)
        return real(p, defines)

    monkeypatch.setattr(jit, "compile_period", gated)
    monkeypatch.setattr(jit, "_inflight", {})
    monkeypatch.setattr(jit, "CACHE_DIR", str(tmp_path))  # a cache of its own: the period is not in it
    dev = GpuSearchDevice(0, jit_mode="auto")
    try:
        dev.epochs[0] = epoch0
        work = Work(HEADER, boundary_for(PREFIX_128), height, job_id=1, flags=0)
        pipe = SearchPipeline(dev)
        n = 2 * G
        assert pipe.step(work, START, n) is None
        block = dev.block_for(height)
        fut = dev.searchers[0].chooser.pending(period)
        assert fut is not None
        first = pipe.step(work, START + n, n)
        assert first.kernel == "generic" and not fut.done()  # it arrived while the compile was pending
        gate.set()
        path = fut.result(COMPILE_LIMIT_S)
        assert jit.ready(period, dev.searchers[0].defines) == path
        results = [first, pipe.step(work, START + 2 * n, n), pipe.step(work, START + 3 * n, n), pipe.drain()]
        assert [r.kernel for r in results] == ["generic", "generic", "jit", "jit"]
        assert dev.block_for(height) == block == G
        assert dev.searchers[0].kernel_kind == "jit"
        for k, r in enumerate(results):  # the windows tile [START, START + 4n): no gap, no overlap
            assert (r.start, r.count, r.hashes) == (START + k * n, n, n)
        for k in (0, 3):  # a generic window and a jit window
            want = oracle_window(epoch0, height, START + k * n, n, PREFIX_128)
            assert as_set(results[k].shares) == set(want), results[k].kernel
        assert any(oracle_window(epoch0, height, START + k * n, n, PREFIX_128) for k in (0, 3))
    finally:
        gate.set()
        dev.close()
