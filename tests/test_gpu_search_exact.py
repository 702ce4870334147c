"""The KawPow search kernels return exactly the nonces that qualify: kawpow_search in the variant
that ships at each DAG size (epoch 0 and 384: KP_SBUFFER, epoch 390: KP_PTR64) and kawpow_search_any,
over a 2-granule window (two workgroups, every wave of each, all 16 lanes of a group), with the
target on, one under and far from the smallest hash of the window, the share ring at and past its
capacity, and nonce windows that carry into the seed's high word and wrap at 2^64.

The oracle is tests/search_oracle.py: the static batch kernel kawpow_verify_dag over every nonce of
the window with the prefix rule applied on the host, itself checked here against the host golden
model. A share that is computed wrongly is caught by the miner's host re-hash; a share that is
missed is caught by nothing but these tests."""
import os

import pytest

from search_oracle import (G, HEADER, M64, START, as_set, boundary_for, clear_cache, head64, host_window, in_window,
                           le256_be, oracle_rows, oracle_window)

pytestmark = pytest.mark.gpu

N = 2 * G
PREFIX_64 = (1 << 64) // 64   # mean 24 shares in 2 granules
PREFIX_8 = (1 << 64) // 8     # mean 192: three times the ring
HEIGHT = {0: 1, 384: 384 * 7500 + 123, 390: 390 * 7500 + 123}  # period kernels that build() compiles
HEIGHT_P1 = 4                 # epoch 0, period 1
# shares of [START, START + N) at PREFIX_64, counted on the host golden model (search_oracle.host_window)
ORACLE_COUNTS = {(0, 1): 18, (0, 4): 25, (384, HEIGHT[384]): 26, (390, HEIGHT[390]): 27}
START_2_32 = (1 << 32) - G - 5  # the seed's low nonce word carries into the high one at offset G + 5
START_2_64 = (1 << 64) - G - 5  # the window goes on from nonce 0 at offset G + 5

_big = pytest.mark.skipif(os.environ.get("NODEXA_FAST_GPU_TESTS") == "1", reason="4 GiB DAG builds")
# (epoch, height) of the share-set windows and (epoch, kernel choice) of the edge launches
WINDOWS = [(0, 1), (0, HEIGHT_P1), pytest.param(384, HEIGHT[384], marks=_big), pytest.param(390, HEIGHT[390], marks=_big)]
EDGES = [(0, "wait"), (0, "off"), pytest.param(384, "wait", marks=_big), pytest.param(390, "wait", marks=_big)]


def _epoch_fixture(epoch):
    @pytest.fixture(scope="module", name=f"ep{epoch}")
    def fixture(gpu, core):
        import torch

        from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

        e = DeviceEpoch(epoch, device=0, ctx=core.get_epoch_context(epoch))
        e.build()
        torch.cuda.synchronize()
        assert e.l1_matches()
        yield e
        clear_cache()
        del e
        torch.cuda.empty_cache()

    return fixture


ep0, ep384, ep390 = _epoch_fixture(0), _epoch_fixture(384), _epoch_fixture(390)


def searcher(ep, height, jit_mode="wait"):
    """The searcher of the variant that ships for this DAG size (jit_mode "off": the period-agnostic kernel)."""
    from nodexa_chain_core_amd.ops import jit
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher

    variant = jit.defines_for(ep.dag_bytes)
    assert ("KP_SBUFFER" in variant) == (ep.epoch < 385) and ("KP_PTR64" in variant) == (ep.epoch >= 385)
    assert "KP_BLOCK=768" in variant
    s = KawpowSearcher(ep, height, jit_mode=jit_mode)
    assert s.block == G
    return s


def run(s, start, n, target64):
    """(shares, count, skipped) of one launch, on the kernel the searcher's mode names."""
    from nodexa_chain_core_amd.ops.kawpow import parse_results

    s.launch(HEADER, start, n, target64)
    shares = s.collect()
    assert s.kernel_kind == ("generic" if s.jit_mode == "off" else "jit")
    _shares, count, skipped = parse_results(s.results_host.numpy().tobytes(), s.h.KAWPOW_MAX_SHARES)
    return shares, count, skipped


def check_share_set(s, ep, height, start, expect_count=None):
    want = oracle_window(ep, height, start, N, PREFIX_64)
    print(f"epoch {ep.epoch} height {height} start {start:#x}: oracle shares {len(want)} in {N} nonces")
    assert 8 <= len(want) <= s.h.KAWPOW_MAX_SHARES  # above the ring's capacity the kernel drops shares
    if expect_count is not None:
        assert len(want) == expect_count
    got, count, skipped = run(s, start, N, PREFIX_64)
    missed = sorted(set(want) - as_set(got))
    # a missed nonce's place in the launch: (nonce, workgroup, wave, lane of its 16-lane group)
    where = [(x, (x - start) % (1 << 64) // G, (x - start) % (1 << 64) % G // 64, (x - start) % 16) for x, _, _ in missed]
    assert as_set(got) == set(want), where
    assert count == len(want) and skipped == 0
    return want


# ------------------------------------------------------------------ 1. share set == oracle
@pytest.mark.parametrize("epoch, height", WINDOWS)
def test_share_set_equals_oracle(request, epoch, height):
    ep = request.getfixturevalue(f"ep{epoch}")
    check_share_set(searcher(ep, height), ep, height, START, ORACLE_COUNTS[epoch, height])


# ------------------------------------------------------------------ 2. the oracle against the host
def spread_offsets(is_share):
    """16 offsets of non-shares in the window: eight per workgroup, in eight different waves of it,
    group lanes 0, 7, 8 and 15 among them (a share moves on by whole groups: the lane stays)."""
    out = []
    for wg in range(2):
        for q, lane in enumerate((0, 7, 8, 15, 3, 12, 0, 15)):
            o = wg * G + q * 96 + lane
            while is_share(o):
                o += 16
            assert o // G == wg and o % 16 == lane
            out.append(o)
    assert len(set(out)) == 16 and {0, 7, 8, 15} <= {o % 16 for o in out}
    return out


@pytest.mark.parametrize("epoch, height", WINDOWS)
def test_oracle_equals_host(request, core, epoch, height):
    """A common error of the two device kernels over one resident DAG would cancel in the share-set
    test: the oracle's rows are the host golden model's."""
    from nodexa_chain_core_amd.ops.kawpow import Share

    ep = request.getfixturevalue(f"ep{epoch}")
    rows = oracle_rows(ep, height, START, N)
    assert [r[0] for r in rows] == list(range(START, START + N))
    shares = [r for r in rows if head64(r[2]) <= PREFIX_64]
    assert len(shares) == ORACLE_COUNTS[epoch, height]
    for nonce, mix, fin in shares:
        assert Share(nonce, mix, fin).verify_full(height, HEADER, boundary_for(PREFIX_64), ctx=ep.ctx), nonce
    for o in spread_offsets(lambda o: head64(rows[o][2]) <= PREFIX_64):
        nonce, mix, fin = rows[o]
        assert core.kawpow_hash(ep.ctx, height, HEADER, nonce) == (fin, mix), (o, nonce)
    if epoch == 0:
        assert rows == host_window(core, ep.ctx, height, HEADER, START, N)


# ------------------------------------------------------------------ 3. the prefix compare at its edge
@pytest.mark.parametrize("epoch, jit_mode", EDGES)
def test_prefix_edge(request, epoch, jit_mode):
    ep = request.getfixturevalue(f"ep{epoch}")
    height = HEIGHT[epoch]
    rows = oracle_rows(ep, height, START, N)
    by_nonce = {r[0]: r for r in rows}
    heads = sorted(head64(r[2]) for r in rows)
    m = heads[0]
    assert 0 < m < heads[1]  # the smallest head is unique
    s = searcher(ep, height, jit_mode)
    cap = s.h.KAWPOW_MAX_SHARES
    got, count, skipped = run(s, START, N, m)  # on the target: <=, not <
    assert as_set(got) == {r for r in rows if head64(r[2]) == m} and (count, skipped) == (1, 0)
    for target in (m - 1, 0):
        got, count, skipped = run(s, START, N, target)
        assert (got, count, skipped) == ([], 0, 0), target
    got, count, skipped = run(s, START, N, M64)  # everything qualifies: the count stays exact past the ring
    assert (count, skipped) == (N, 0) and N > cap
    assert len(got) == cap == len({x.nonce for x in got})
    for x in got:
        assert in_window(x.nonce, START, N) and (x.nonce, x.mix_hash, x.final_hash) == by_nonce[x.nonce]


# ------------------------------------------------------------------ 4. the ring limit through the miner
@pytest.mark.parametrize("jit_mode", ["wait", "off"])
def test_ring_limit_through_miner(ep0, jit_mode):
    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, Work

    height = HEIGHT[0]
    want = oracle_window(ep0, height, START, N, PREFIX_8)
    dev = GpuSearchDevice(0, jit_mode=jit_mode)
    try:
        cap = dev.h.KAWPOW_MAX_SHARES
        assert len(want) > cap
        dev.epochs[0] = ep0
        dev.submit(0, Work(HEADER, boundary_for(PREFIX_8), height, job_id=3, flags=0), START, N)
        res = dev.wait(0)
        assert res.kernel == ("generic" if jit_mode == "off" else "jit")
        assert (res.start, res.count, res.hashes, res.aborted) == (START, N, N, 0)
        assert res.dropped == len(want) - cap
        assert len(res.shares) == cap == len({x.nonce for x in res.shares})
        assert as_set(res.shares) <= set(want)
    finally:
        dev.close()


# ------------------------------------------------------------------ 5. search()'s 256-bit host filter
def test_full_boundary_filter(ep0):
    height = HEIGHT[0]
    rows = oracle_rows(ep0, height, START, N)
    shares = sorted(oracle_window(ep0, height, START, N, PREFIX_64), key=lambda r: r[2])
    pick = shares[len(shares) // 2]  # shares under it and over it
    F = pick[2]
    s = searcher(ep0, height)
    below = (int.from_bytes(F, "big") - 1).to_bytes(32, "big")
    assert F[8:] != bytes(24) and below[:8] == F[:8]  # F - 1 keeps the prefix: only the host's compare can drop it
    for boundary, has_pick in ((F, True), (below, False), (F[:8] + bytes(24), False), (F[:8] + b"\xff" * 24, True)):
        want = {r for r in rows if le256_be(r[2], boundary)}
        assert (pick in want) == has_pick and len(want) <= s.h.KAWPOW_MAX_SHARES
        assert as_set(s.search(HEADER, START, N, boundary)) == want, boundary.hex()


# ------------------------------------------------------------------ 6. nonce carries
@pytest.mark.parametrize("jit_mode", ["wait", "off"])
def test_window_across_2_32(ep0, jit_mode):
    height = HEIGHT[0]
    want = check_share_set(searcher(ep0, height, jit_mode), ep0, height, START_2_32)
    assert {x >> 32 for x, _, _ in want} == {0, 1}  # shares on both sides of the carry


def test_window_across_2_64(ep0):
    height = HEIGHT[0]
    want = check_share_set(searcher(ep0, height), ep0, height, START_2_64)
    assert all(0 <= x <= M64 for x, _, _ in want)
    assert any(x >= START_2_64 for x, _, _ in want) and any(x < N for x, _, _ in want)  # both sides of the wrap


def test_search_trims_a_wrapping_window(ep0):
    """search() pads the launch to whole workgroups and drops what lies past the window, mod 2^64."""
    height = HEIGHT[0]
    num = 1000  # ends 227 nonces after the wrap; the launch is padded to 2 granules
    padded = oracle_window(ep0, height, START_2_64, N, PREFIX_64)
    want = {r for r in padded if in_window(r[0], START_2_64, num)}
    assert any(x < START_2_64 for x, _, _ in want)  # in the window, past the wrap
    assert set(padded) - want                      # qualifying nonces in the padding: they must go
    got = searcher(ep0, height).search(HEADER, START_2_64, num, boundary_for(PREFIX_64))
    assert as_set(got) == want
