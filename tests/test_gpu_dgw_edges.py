"""hip/kernels/dgw.hip (`dgw_batch`) on the MI355X against the big-int oracle of
tests/dgw_oracle.py, bit for bit, on raw synthetic series: the arithmetic at its edges (clamp,
negative spans, nTime across 2^31 and 2^32, wrapping and tiny targets, the GetCompact
renormalisation), the index logic (`a`, `base_height`, `dgw_activation_block`, block tails), the
era switches and the 0 = "host decides" value. tests/test_dgw_series.py checks the host twin on the
same series; the fixture test in tests/test_gpu_verify.py only compares the twins with each other."""
import os

import numpy as np
import pytest

import dgw_oracle as O

pytestmark = pytest.mark.gpu

EQ_LIMIT = ((1 << 236) - 1).to_bytes(32, "little")
MARKER = -0x21524111  # 0xdeadbeef as int32


def _run(core, params, times, bits, a, n, base_height):
    """dgw_batch over the series == the oracle for all n outputs, == core.dgw_average wherever
    the window is full. Returns the kernel's output."""
    from nodexa_chain_core_amd.ops import dgw

    assert len(times) == len(bits) == a + n
    tb, bb = O.pack(times), O.pack(bits)
    got = dgw.expected_bits(params, tb, bb, a, n, base_height)
    want = np.array(O.expected_bits_oracle(core.dgw_constants(params), times, bits, a, n, base_height), np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), hex(got[i]), hex(want[i])) for i in bad[:8]]
    for i in range(n):
        j, last_height = a - 1 + i, base_height + i
        if j >= O.PAST - 1 and last_height >= O.PAST and last_height + 1 >= params.dgw_activation_block:
            assert got[i] == core.dgw_average(params, tb, bb, j, times[j + 1]), i
    return got


@pytest.mark.parametrize("net", ["test", "regtest"])
@pytest.mark.parametrize("family", O.FAMILIES)
def test_arithmetic_families(core, gpu, net, family):
    """One launch per start time: 11 concatenated 181-entry blocks, so output 181 w is the header
    that sees exactly block w's window and the outputs between see windows across two blocks. At
    most 1 % of a family's own windows may be compact 0."""
    p = core.make_chain_params(net)
    span = core.dgw_constants(p)["target_timespan"]
    own = []
    for t0 in O.T0S:
        times, bits = O.family_series(family, t0, span)
        got = _run(core, p, times, bits, O.PAST, len(times) - O.PAST, 1_000_000)
        own += [int(x) for x in got[::O.WINDOW]]
    assert len(own) == len(O.T0S) * len(O.spans(span))
    assert sum(1 for x in own if x == 0) <= len(own) // 100


@pytest.mark.parametrize("a", [0, 1, 179, 180])
def test_from_genesis(core, gpu, a):
    """Series entry k is the block at height k: pow-limit compact while the parent is below height
    180, computed values from the header at height 181 on, wherever the batch starts."""
    p = core.make_chain_params("test")
    n = 400
    times, bits = O.smooth_series(a + n)
    got = _run(core, p, times, bits, a, n, a - 1)
    limit = core.dgw_constants(p)["compacts"][0]
    first = 181 - a  # the output of the header at height 181
    heights = np.arange(a, a + n)
    assert got[0] == (0 if a == 0 else limit)  # the genesis block itself is before DGW's activation
    assert (got[(heights >= 1) & (heights <= 180)] == limit).all()
    assert (got[first:] != limit).all() and (got[first:] != 0).all()


def test_full_ancestors_high_up(core, gpu):
    p = core.make_chain_params("test")
    times, bits = O.smooth_series(180 + 300)
    got = _run(core, p, times, bits, 180, 300, 0x7FFF0000)
    assert (got != 0).all()


def test_short_ancestors(core, gpu):
    """100 ancestors at height 5000: the window is full from series index 179 on, so outputs
    0..79 are left to the host and output 80 is the first computed one."""
    p = core.make_chain_params("test")
    times, bits = O.smooth_series(100 + 300)
    got = _run(core, p, times, bits, 100, 300, 5000)
    assert (got[:80] == 0).all() and (got[80:] != 0).all()


def test_activation_block_inside_batch(core, gpu):
    p = core.make_chain_params("test")
    base, k = 5000, 137
    p.dgw_activation_block = base + 1 + k  # output k: last_height + 1 == the activation block
    times, bits = O.smooth_series(180 + 300)
    got = _run(core, p, times, bits, 180, 300, base)
    assert (got[:k] == 0).all() and (got[k:] != 0).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_block_tail_leaves_slack_alone(core, gpu, n):
    """Through the raw launcher with n + 64 output slots: the last block's idle lanes write nothing."""
    import torch

    from nodexa_chain_core_amd.ops import runtime

    p = core.make_chain_params("test")
    c = core.dgw_constants(p)
    a, base = 180, 77_000
    times, bits = O.smooth_series(a + n)
    d_t = torch.from_numpy(np.array(times, np.uint32).view(np.int32)).to(gpu)
    d_b = torch.from_numpy(np.array(bits, np.uint32).view(np.int32)).to(gpu)
    d_o = torch.full((n + 64,), MARKER, dtype=torch.int32, device=gpu)
    runtime.hip().launch_dgw(runtime.static_kernel("dgw", "dgw_batch"), d_t.data_ptr(), d_b.data_ptr(), d_o.data_ptr(),
                             a, n, base, c["dgw_activation_block"], c["kawpow_time"], c["equihash_time"], c["limits"],
                             c["compacts"], c["target_timespan"], runtime.current_stream_handle())
    out = d_o.cpu().numpy()
    assert (out[n:] == MARKER).all()
    want = np.array(O.expected_bits_oracle(c, times, bits, a, n, base), np.uint32)
    assert np.array_equal(out[:n].view(np.uint32), want) and (want != 0).all()


@pytest.mark.parametrize("eq_limit", [None, EQ_LIMIT], ids=["null-eq-limit", "eq-limit"])
@pytest.mark.parametrize("order", ["kawpow-first", "equihash-first"])
@pytest.mark.parametrize("shift", [0, 1], ids=["at-a-block-time", "one-past-a-block-time"])
def test_era_switches(core, gpu, eq_limit, order, shift):
    """The series and activation placement of tests/test_dgw_series.py::test_era_switches (which
    pins where each bootstrap starts and ends): windows with 0, 1 .. 179, 180 blocks at or past each
    activation, next_time equal to it and one below, both orders, Equihash winning the overlap."""
    p = core.make_chain_params("test")
    if eq_limit:
        p.equihash_limit = eq_limit
    times, bits = O.smooth_series(760)
    first, second = times[250] + shift, times[350] + shift
    p.kawpow_activation_time, p.equihash_activation_time = (first, second) if order == "kawpow-first" else (second, first)
    got = _run(core, p, times, bits, 180, 580, 9000)
    pow_c, kaw_c, eq_c = core.dgw_constants(p)["compacts"]
    assert eq_c == (0x1E0FFFFF if eq_limit else pow_c)
    at = lambda h: int(got[h - 180])  # noqa: E731
    assert at(350 + shift) == eq_c and at(429 + shift) == eq_c  # both bootstraps apply: Equihash wins
    assert at(250 + shift) == (kaw_c if order == "kawpow-first" else eq_c)
    assert at(249 + shift) not in (pow_c, eq_c) and at(530 + shift) not in (pow_c, eq_c)


def test_zero_sentinel(core, gpu):
    """Every window target zero: the true DGW value is compact 0, which the kernel returns and the
    host reads as "not decided". A real batch accepted with those zeros as its `bits` ends on the
    same tip as one accepted without: the host recomputed every header."""
    from nodexa_chain_core_amd.models import synthetic

    params, headers = synthetic.load(os.path.join(os.path.dirname(__file__), "data", "testnet_kawpow_10k.hdr"))
    hs = list(headers)[:300]
    n = len(hs)
    times, _ = O.smooth_series(180 + n)
    bits = [0x01003456] * (180 + n)
    got = _run(core, core.make_chain_params("test"), times, bits, 180, n, 5000)
    assert (got == 0).all()
    adj = hs[-1].time + 3600
    plain, fed = core.HeaderChain(params), core.HeaderChain(params)
    assert all(r.ok for r in plain.accept_headers(hs, adj, False))
    assert all(r.ok for r in fed.accept_headers(hs, adj, False, None, got.tobytes()))
    assert fed.height() == plain.height() == n
    assert fed.tip().hash == plain.tip().hash
