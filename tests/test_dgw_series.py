"""The host's DarkGravityWave model (csrc/chain/pow_rules.cpp dgw_average, reached over a raw
series through core.dgw_average) against the big-int oracle of tests/dgw_oracle.py, bit for bit.

The host model and hip/kernels/dgw.hip share their limb loop and reciprocal division, so this is
the comparison that can see a mistake made in both; tests/test_gpu_dgw_edges.py repeats it for the
kernel. Series: tests/dgw_oracle.py (clamp edges, negative spans, nTime across 2^31 and 2^32, six
nBits families), under the mainnet-style limit and under regtest's 0x207fffff limit."""
import pytest

import dgw_oracle as O

NETWORKS = ("test", "regtest")
# a limit below every network's pow limit, so the Equihash bootstrap shows in the result
EQ_LIMIT = ((1 << 236) - 1).to_bytes(32, "little")


def _check(core, params, times, bits, js=None):
    """core.dgw_average == the oracle at every series index of `js` (default: every full window)."""
    c = core.dgw_constants(params)
    tb, bb = O.pack(times), O.pack(bits)
    paths = []
    for j in js if js is not None else range(O.PAST - 1, len(times) - 1):
        want, path = O.dgw_path(c, times, bits, j, times[j + 1])
        got = core.dgw_average(params, tb, bb, j, times[j + 1])
        assert got == want, (j, hex(got), hex(want), path)
        paths.append((want, path))
    return paths


def test_oracle_limits_match_constants(core):
    """The oracle's own GetCompact of the limbs gives the compacts the kernel is handed."""
    for net in NETWORKS:
        p = core.make_chain_params(net)
        for eq in (None, EQ_LIMIT):
            if eq:
                p.equihash_limit = eq
            c = core.dgw_constants(p)
            assert [O.get_compact(O.limit(c, k)) for k in range(3)] == list(c["compacts"])
            assert c["target_timespan"] == 180 * p.pow_target_spacing
    assert O.get_compact(int.from_bytes(EQ_LIMIT, "little")) == 0x1E0FFFFF
    for v in (0, 1, 0x80, 0x7FFFFF, 0x800000, 0x123456 << 200, (1 << 256) - 1):
        assert O.get_compact(v) == core.get_compact(v)
    for b in (0, 0x01003456, 0x02008000, 0x03123456, 0x04123456, 0x1D00FFFF, 0x207FFFFF, 0x2100FFFF, 0x22000001):
        assert O.set_compact(b) == core.set_compact(b)[0]


def test_short_window_throws(core):
    p = core.make_chain_params("test")
    times, bits = O.smooth_series(200)
    with pytest.raises(Exception):
        core.dgw_average(p, O.pack(times), O.pack(bits), 178, times[179])
    with pytest.raises(Exception):
        core.dgw_average(p, O.pack(times), O.pack(bits), 200, 0)
    assert core.dgw_average(p, O.pack(times), O.pack(bits), 179, times[180]) != 0


@pytest.mark.parametrize("net", NETWORKS)
@pytest.mark.parametrize("family", O.FAMILIES)
def test_host_matches_oracle(core, net, family):
    """Every window of the family (3 start times x 11 spans), and every window that straddles two
    of them. At most 1 % of a family's own windows may come out as compact 0 (the kernel's "host
    decides" value), and nearly all must reach the arithmetic and not a bootstrap."""
    p = core.make_chain_params(net)
    span = core.dgw_constants(p)["target_timespan"]
    own = []
    for t0 in O.T0S:
        times, bits = O.family_series(family, t0, span)
        paths = _check(core, p, times, bits)
        own += paths[::O.WINDOW]
    assert len(own) == len(O.T0S) * len(O.spans(span))
    assert sum(1 for v, _ in own if v == 0) <= len(own) // 100
    assert sum(1 for _, path in own if path == "computed") >= len(own) * 9 // 10


@pytest.mark.parametrize("net", NETWORKS)
@pytest.mark.parametrize("eq_limit", [None, EQ_LIMIT], ids=["null-eq-limit", "eq-limit"])
@pytest.mark.parametrize("order", ["kawpow-first", "equihash-first"])
@pytest.mark.parametrize("shift", [0, 1], ids=["at-a-block-time", "one-past-a-block-time"])
def test_era_switches(core, net, eq_limit, order, shift):
    """Both activation times inside one series, 100 blocks apart: the windows hold 0, 1 .. 179, 180
    blocks at or past each, next_time hits the activation exactly (shift 0) or is one below it
    (shift 1), and for 80 headers both bootstraps apply, where the Equihash one must win."""
    p = core.make_chain_params(net)
    if eq_limit:
        p.equihash_limit = eq_limit
    times, bits = O.smooth_series(760)
    first, second = times[250] + shift, times[350] + shift
    p.kawpow_activation_time, p.equihash_activation_time = (first, second) if order == "kawpow-first" else (second, first)
    paths = _check(core, p, times, bits)
    kinds = [path for _, path in paths]  # header j + 1 for j = 179 ..
    assert {"computed", "kawpow", "equihash"} == set(kinds)
    at = lambda h: kinds[h - 180]  # noqa: E731
    s = shift
    assert at(249 + s) == "computed"  # next_time == activation - 1 when s == 1
    if order == "kawpow-first":
        want = {250 + s: "kawpow", 349 + s: "kawpow", 350 + s: "equihash", 429 + s: "equihash", 529 + s: "equihash"}
    else:
        want = {250 + s: "equihash", 350 + s: "equihash", 429 + s: "equihash", 430 + s: "kawpow", 529 + s: "kawpow"}
    want[530 + s] = "computed"
    assert {h: at(h) for h in want} == want
