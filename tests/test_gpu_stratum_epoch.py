"""The Stratum server's own share-check DAGs on the MI355X (-stratumgpuverify=1): a server with a
device and no miner builds the served epoch's DAG itself and hashes its shares on it, builds the
next epoch's ahead of the boundary, hashes with the light-mode kernel while a build runs, and
without the flag does what it always did. Epochs 0 and 1 (1 GiB DAGs, the smallest).

The shares are found with the host's light-mode search at an easy target (4 bits), so every hash
the device returns is compared with the host golden model through the share itself: the server
accepts a share only if its recomputed final hash and mix equal the submitted ones."""
import threading

import pytest

from test_stratum import Peer, _wait

pytestmark = pytest.mark.gpu

H = bytes([0x11]) * 32
BLOCK_TARGET = (1 << 216) - 1
BITS = 4
TARGET = (1 << (256 - BITS)) - 1


@pytest.fixture()
def empty_registry(gpu):
    """No DAG and no light cache of device 0 registered (an earlier test's miner may have shared
    its own); they are put back afterwards."""
    from nodexa_chain_core_amd.ops import verify as V

    with V._epochs_lock:
        kept = {k: V._epochs.pop(k) for k in [k for k in V._epochs if k[0] == 0]}
    with V._light_lock:
        kept_light = {k: V._light.pop(k) for k in [k for k in V._light if k[0] == 0]}
    yield V
    with V._epochs_lock:
        for k in [k for k in V._epochs if k[0] == 0]:
            V._epochs.pop(k)
        V._epochs.update(kept)
    with V._light_lock:
        V._light.update(kept_light)


def _job(job_id, height, tip="tipA"):
    from nodexa_chain_core_amd.miner.stratum_server import ServerJob

    return ServerJob(job_id, H, height, BLOCK_TARGET, 0x1D00FFFF, True, tip)


def _find(core, height, prefix, start=0):
    """(nonce, final, mix) of the first share at TARGET under the 2-byte nonce prefix, on the host."""
    ctx = core.get_epoch_context(height // core.EPOCH_LENGTH)
    ok, nonce, fin, mix = core.kawpow_search_light(ctx, height, H, TARGET.to_bytes(32, "big"), (prefix << 48) + start, 4096)
    assert ok and nonce >> 48 == prefix and (fin, mix) == tuple(core.kawpow_hash(ctx, height, H, nonce))
    return nonce, fin, mix


def _submit(p, msg_id, job_id, nonce, mix):
    return p.call(msg_id, "mining.submit", ["w", job_id, "0x%016x" % nonce, "0x" + H.hex(), "0x" + mix.hex()])


def _flipped(core, height, nonce, mix):
    """`mix` with one bit flipped, such that the cheap check still passes."""
    for bit in range(256):
        bad = bytearray(mix)
        bad[bit // 8] ^= 1 << (bit % 8)
        if int.from_bytes(core.kawpow_hash_no_verify(height, H, bytes(bad), nonce), "big") <= TARGET:
            return bytes(bad)
    raise AssertionError("no single-bit flip passes the cheap check")


@pytest.mark.timeout(120)
def test_server_builds_its_own_dag(empty_registry, core):
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    V = empty_registry
    src = StaticJobSource()
    src.push(_job("j1", 1))
    srv = StratumServer(src, share_bits=BITS, device=0, gpu_verify=True).start()
    p = q = None
    try:
        _wait(lambda: srv.epochs.ready(0) and srv.epochs.idle(), timeout=90, what="the owner's epoch 0")
        info = srv.info()
        assert info["dag_builds"] == 1 and info["dag_build_failures"] == 0 and info["epochs_resident"] == [0], info
        assert info["dag_last_build_ms"] > 0 and srv.epochs.own_epochs() == [0]
        assert V.resident_dags(0)[0].seal_table is not None  # the checked build: audited and sealed
        # the device's hashes on that DAG, and the light-mode kernel's, equal the host's byte for byte
        ctx = core.get_epoch_context(0)
        nonces = [(1 << 48) + 17 * k for k in range(40)]
        want = [tuple(bytes(x) for x in core.kawpow_hash(ctx, 1 + k % 3, H, n)) for k, n in enumerate(nonces)]
        heights = [1 + k % 3 for k in range(40)]
        assert V.gpu_full_hash(heights, [H] * 40, nonces, device=0, mode="auto") == want
        assert V.gpu_full_hash(heights, [H] * 40, nonces, device=0, mode="light") == want
        # one bit of the mix flipped: the connection is closed
        p = Peer.connect(srv.port)
        p.login()
        nonce, fin, mix = _find(core, 1, 1)
        r = _submit(p, 3, "j1", nonce, _flipped(core, 1, nonce, mix))
        assert r["error"][0] == 20 and "mix" in r["error"][1] and p.recv() is None
        # a valid share is accepted, and it was hashed on the DAG
        q = Peer.connect(srv.port)
        q.login()
        nonce, fin, mix = _find(core, 1, 2)
        assert _submit(q, 3, "j1", nonce, mix) == {"id": 3, "result": True, "error": None}
        info = srv.info()
        assert (info["verified_gpu"], info["verified_host"], info["verified_gpu_light"]) == (2, 0, 0), info
        assert info["accepted"] == 1 and info["dag_builds"] == 1
    finally:
        for x in (p, q):
            if x is not None:
                x.close()
        srv.stop()
    assert not V.is_resident(0, 0)  # a stopped server gives its DAGs up


@pytest.mark.timeout(120)
def test_next_epoch_is_built_ahead(empty_registry, core):
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    E = core.EPOCH_LENGTH
    src = StaticJobSource()
    src.push(_job("j1", E - 1 - 100))
    srv = StratumServer(src, share_bits=BITS, device=0, gpu_verify=True).start()
    p = None
    try:
        _wait(lambda: srv.epochs.ready(1) and srv.epochs.idle(), timeout=90, what="epochs 0 and 1")
        assert srv.epochs.own_epochs() == [0, 1] and srv.info()["dag_builds"] == 2
        src.push(_job("j2", E, tip="tipB"))
        p = Peer.connect(srv.port)
        p.login()
        nonce, fin, mix = _find(core, E, 1)
        assert _submit(p, 3, "j2", nonce, mix)["result"] is True
        info = srv.info()
        assert (info["verified_gpu"], info["verified_host"], info["verified_gpu_light"]) == (1, 0, 0), info
        assert info["epochs_resident"] == [0, 1] and srv.epochs.own_epochs() == [0, 1] and info["dag_builds"] == 2
    finally:
        if p is not None:
            p.close()
        srv.stop()


@pytest.mark.timeout(120)
def test_light_mode_while_the_build_runs(empty_registry, core):
    """The DAG build held back: once the light cache is on the device the share goes through the
    light-mode kernel, not through the host, and the verifier does not wait for the build."""
    from nodexa_chain_core_amd.miner.stratum_epochs import EpochOwner, device_builder
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    gate = threading.Event()

    class Held(device_builder):
        def build(self, epoch):
            assert gate.wait(60)
            return super().build(epoch)

    own = EpochOwner(0, Held(0))
    src = StaticJobSource()
    src.push(_job("j1", 1))
    srv = StratumServer(src, share_bits=BITS, device=0, epoch_owner=own).start()
    p = None
    try:
        _wait(lambda: own.mode(0) == "light", timeout=60, what="the light cache on the device")
        p = Peer.connect(srv.port)
        p.login()
        nonce, fin, mix = _find(core, 1, 1)
        assert _submit(p, 3, "j1", nonce, mix)["result"] is True
        info = srv.info()
        assert (info["verified_gpu"], info["verified_host"], info["verified_gpu_light"]) == (0, 0, 1), info
        assert info["dag_builds"] == 0 and not own.idle()
        gate.set()
        _wait(lambda: own.ready(0) and own.idle(), timeout=60, what="the build")
        nonce, fin, mix = _find(core, 1, 1, start=(nonce & 0xFFFF) + 1)
        assert _submit(p, 4, "j1", nonce, mix)["result"] is True
        info = srv.info()
        assert (info["verified_gpu"], info["verified_host"], info["verified_gpu_light"]) == (1, 0, 1), info
    finally:
        gate.set()
        if p is not None:
            p.close()
        srv.stop()


@pytest.mark.timeout(120)
def test_flag_off_counts_only_the_host(empty_registry, core):
    from nodexa_chain_core_amd.miner.stratum_server import StaticJobSource, StratumServer

    src = StaticJobSource()
    src.push(_job("j1", 1))
    srv = StratumServer(src, share_bits=BITS, device=0).start()
    p = Peer.connect(srv.port)
    try:
        p.login()
        nonce, fin, mix = _find(core, 1, 1)
        assert _submit(p, 3, "j1", nonce, mix)["result"] is True
        info = srv.info()
        assert (info["verified_gpu"], info["verified_host"]) == (0, 1) and srv.epochs is None
        assert "dag_builds" not in info and "verified_gpu_light" not in info and empty_registry.resident_dags(0) == []
    finally:
        p.close()
        srv.stop()
