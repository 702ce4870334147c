"""Stratum on the MI355X: the pool client mining a loopback pool on the device (every share of a
window submitted, the server's full hashes batched onto the DAG the searcher built, a clean job
reaching the device-side abort within two steps), and a GPU miner process mining regtest blocks
for a node through -stratum. Epoch 0 (1 GiB DAG, the smallest); heights as in
tests/test_gpu_remote_miner.py, whose per-period kernels build() ships."""
import ast
import os
import socket
import subprocess
import sys
import time

import pytest

from test_stratum import KAWPOW_REGTEST, ROOT, _start_node, _stop_node, _wait

pytestmark = pytest.mark.gpu

HEIGHT = 1
BLOCK_TARGET = (1 << 216) - 1   # 2^-40
SHARE_BITS = 18                 # ~4 shares per 2^20-nonce window: far below the 64-entry ring and the 16-share record


@pytest.mark.timeout(180)
def test_loopback_pool_on_the_device(gpu, core):
    from nodexa_chain_core_amd.miner.search import FLAG_CLEAN, GpuSearchDevice
    from nodexa_chain_core_amd.miner.service import MiningService
    from nodexa_chain_core_amd.miner.stratum_client import StratumConnection, StratumLeader
    from nodexa_chain_core_amd.miner.stratum_server import ServerJob, StaticJobSource, StratumServer

    h1, h2 = core.sha256d(b"stratum gpu job 1"), core.sha256d(b"stratum gpu job 2")
    src = StaticJobSource()
    src.push(ServerJob("j1", h1, HEIGHT, BLOCK_TARGET, 0x1D00FFFF, True, "tipA"))
    srv = StratumServer(src, share_bits=SHARE_BITS, device=0).start()
    conn = StratumConnection([("127.0.0.1", srv.port)], "gpu0", "x", backoff=(0.05, 0.2)).start()
    leader = StratumLeader(conn)
    packets = []
    next_work = leader.next_work
    leader.next_work = lambda repartitioned=False: packets.append(next_work(repartitioned)) or packets[-1]
    dev = GpuSearchDevice(0)
    svc = MiningService(dev, leader, window=1 << 20)
    ok = False
    try:
        deadline = time.monotonic() + 90
        while conn.stats["accepted"] < 3:
            assert time.monotonic() < deadline, (conn.stats, srv.stats)
            svc.step()
        st = dict(conn.stats)
        assert st["rejected"] == 0 and st["lost"] == 0 and st["shares_dropped"] == 0 and st["bad_shares"] == 0, st
        ext = srv.info()["connections"][0]["extranonce"]
        assert len(ext) == 4 and conn.sent and all("%016x" % s.nonce == ext + ("%016x" % s.nonce)[4:] for s in conn.sent)
        assert all(s.job_id == "j1" and s.header_hash == h1 for s in conn.sent)
        # the server's batch ran on the DAG the searcher built (share_epoch registered it)
        assert srv.stats["verified_gpu"] > 0 and srv.stats["verified_host"] == 0, srv.stats
        assert srv.stats["verify_batches_gpu"] <= srv.stats["verified_gpu"] and srv.blocks_found == 0
        assert svc.kernel_windows["jit"] > 0
        # a clean job: on the loop's next packet, and the old job's shares stop
        jobs = conn.stats["jobs"]
        src.push(ServerJob("j2", h2, HEIGHT, BLOCK_TARGET, 0x1D00FFFF, True, "tipA"))
        _wait(lambda: conn.stats["jobs"] == jobs + 1, what="the pushed job")
        n = len(packets)
        svc.step()
        svc.step()
        fresh = [w for w in packets[n:n + 2] if w.header_hash == h2]
        assert fresh and fresh[0].flags & FLAG_CLEAN and fresh[0].job_id != packets[n - 1].job_id, packets[n:n + 2]
        # nothing of j1 is queued after that packet: the leader dropped j1 when it handed out j2, and what
        # had been queued before is dropped by the connection thread (a clean job arrived since)
        before = len(conn.sent)
        for _ in range(8):
            svc.step()
        _wait(lambda: conn.shares.empty() and any(s.job_id == "j2" for s in conn.sent), what="shares of the new job")
        ids = [s.job_id for s in conn.sent]
        assert len(ids) < 256  # conn.sent keeps the last 256: nothing was trimmed, `before` still points right
        assert set(ids[before:]) == {"j2"}, ids  # sent since the packet: the new job's only
        assert "j1" not in ids[ids.index("j2"):], ids  # and on any timing, none of j1 behind the first of j2
        assert all(s.header_hash == h2 for s in conn.sent if s.job_id == "j2")
        assert conn.stats["bad_shares"] == 0 and conn.stats["shares_dropped"] == 0
        ok = True
    finally:
        # after a failure nothing more is started on the device: the loop is not stepped again
        conn.stop()
        srv.stop()
        if ok:
            svc.pipe.drain()
        dev.close()


@pytest.mark.timeout(420)
def test_node_and_gpu_miner_process(gpu, core, tmp_path):
    """tests/test_stratum.py's node case with the GPU miner as a fresh child process."""
    node, c, stratum_port = _start_node(tmp_path, core, [KAWPOW_REGTEST])
    trap = socket.socket()
    trap.bind(("127.0.0.1", 0))
    trap.listen(4)
    trap.setblocking(False)
    try:
        assert c.getstratuminfo()["serving"]
        miner = subprocess.run([sys.executable, "-m", "nodexa_chain_core_amd.miner.remote", "-regtest", "-gpu=0",
                                "-minerwindow=256", f"-stratum=127.0.0.1:{stratum_port}", "-stratumuser=gpu0", "-blocks=2",
                                f"-rpcport={trap.getsockname()[1]}", "-printtoconsole=0"],
                               env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
        assert miner.returncode == 0, miner.stdout[-2000:] + miner.stderr[-4000:]
        stats = ast.literal_eval(miner.stdout.strip().splitlines()[-1])
        assert stats["accepted"] >= 2 and stats["bad_shares"] == 0 and stats["lost"] == 0 and stats["jobs"] >= 2, stats
        assert stats["rejected"] == stats["rejected_stale"] and stats["kernel"] == "jit", stats
        with pytest.raises(BlockingIOError):
            trap.accept()  # the miner never made an RPC connection
        assert c.getblockcount() >= 2
        _wait(lambda: c.getstratuminfo()["height"] == c.getblockcount() + 1, what="the pushed job")
        info = c.getstratuminfo()
        assert info["blocks_found"] >= 2 and info["accepted"] >= 2 and info["jobs_sent"] >= 3, info
        rig = [x for x in info["connections"] + info["recent_connections"] if x["user"] == "gpu0"]
        assert len(rig) == 1 and rig[0]["accepted"] >= 2 and rig[0]["hashrate"] > 0 and rig[0]["last_share"] > 0, rig
        assert rig[0]["agent"].startswith("nodexa-miner") and len(rig[0]["extranonce"]) == 4
        # this node has no GPU of its own: its full share hashes ran on the host
        assert info["verified_host"] >= 2 and info["verified_gpu"] == 0 and info["job"]["header_hash"], info
    finally:
        trap.close()
        _stop_node(node, c)
