"""Rank 0 of a miner world whose lost ranks come back (tests/test_miner_rejoin.py over gloo on CPU
devices, tests/test_gpu_miner_rejoin.py with every rank on GPU 0).

Starts the rank supervisor before it touches torch.distributed or a GPU, has it start ranks
1..n-1, and mines a regtest chain (KawPow from genesis+1) until what NODEXA_TEST_EXPECT names has
happened ("rejoin": a rank came back and hashed again; "refused": a rank was refused; "failed": a
re-join attempt failed and the survivors went on), then NODEXA_TEST_BLOCKS more blocks, then
sends the stop packet. Writes the supervisor's status to argv[2] once the first world mines (the
test takes a follower's pid from it) and a JSON report to argv[1]."""
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_path: str, status_path: str) -> int:
    from nodexa_chain_core_amd.miner import supervisor as SV

    n = int(os.environ["NODEXA_TEST_RANKS"])
    gpu = os.environ.get("NODEXA_TEST_GPU") == "1"
    timeout = float(os.environ.get("NODEXA_MINER_COLLECTIVE_TIMEOUT", "30"))
    window = int(os.environ.get("NODEXA_MINER_WINDOW", "8"))
    policy = SV.RejoinPolicy(float(os.environ.get("NODEXA_TEST_REJOIN_DELAY", "0.3")),
                             int(os.environ.get("NODEXA_TEST_REJOIN_MAX", "3")), 600.0)
    SV.assert_gpu_untouched()
    assert "torch" not in sys.modules, "rank 0 must start the supervisor before it imports torch"
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)

    # the supervisor and the first followers, before anything of torch or the GPU
    sup = SV.SupervisorClient()
    from nodexa_chain_core_amd.miner import service as MS

    env = {k: v for k, v in os.environ.items() if k.startswith("NODEXA_MINER_")}
    env.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "NODEXA_MINER_CPU": "0" if gpu else "1",
                "PYTHONPATH": SV.follower_pythonpath()})
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        store_port = sk.getsockname()[1]
    env["NODEXA_MINER_STORE_PORT"] = str(store_port)
    argv = json.loads(os.environ["NODEXA_TEST_NEWCOMER_ARGV"]) if os.environ.get("NODEXA_TEST_NEWCOMER_ARGV") else None
    rj = MS.Rejoiner(sup, policy, gpus=[0] * n, env=env, argv=argv)
    rj.spawn_first()
    try:
        return mine(rj, out_path, status_path, n, gpu, timeout, window, store_port)
    finally:
        rj.close()


def mine(rj, out_path, status_path, n, gpu, timeout, window, store_port) -> int:
    from nodexa_chain_core_amd.chain.state import REGTEST_KAWPOW_FROM_GENESIS, ChainState, make_params
    from nodexa_chain_core_amd.miner import service as MS
    from nodexa_chain_core_amd.parallel import world as W

    W.init(use_gpu=gpu, device_index=0 if gpu else None, rank=0, world_size=n, elastic=True,
           timeout_s=max(int(timeout), W.rendezvous_timeout()), collective_timeout_s=timeout, store_port=store_port)
    state = ChainState(make_params("regtest", REGTEST_KAWPOW_FROM_GENESIS), None)
    leader = MS.ChainLeader(state, target_bits=int(os.environ.get("NODEXA_TEST_TARGET_BITS", "7")))
    fail = MS.injected_fail_rate(float(os.environ.get("NODEXA_MINER_FAILRATE", "0") or 0), 0)
    dev = MS.make_rank_device(not gpu, 0 if gpu else None, collective_dag=gpu, window=window, fail_rate=fail)
    svc = MS.MiningService(dev, leader, window=window, collective_timeout_s=timeout, record_windows=True, rejoin=rj,
                           max_failures=int(os.environ.get("NODEXA_MINER_MAXFAILURES", "3")),
                           grace_s=float(os.environ["NODEXA_TEST_GRACE"]) if os.environ.get("NODEXA_TEST_GRACE") else None)
    expect = os.environ.get("NODEXA_TEST_EXPECT", "rejoin")
    blocks = int(os.environ.get("NODEXA_TEST_BLOCKS", "2"))
    t0 = time.time()
    rep = {"sizes": [svc.world_size], "gpus_first": None, "gpus_out": None}
    hashes_at_rejoin, blocks_at_rejoin, failed_at_step = None, None, None
    shares_after = os.environ.get("NODEXA_TEST_SHARES_AFTER") == "1"  # the rank that came back must find blocks too

    def blocks_of(g):
        return leader.per_rank.get(g, {}).get("blocks", 0)

    def step():
        if time.time() - t0 > float(os.environ.get("NODEXA_TEST_DEADLINE", "200")):
            raise SystemExit(f"rank 0: took too long ({expect}; sizes {rep['sizes']}, {rj.ranks}, {rj.counters})")
        try:
            svc.step()
        except MS.CollectiveError as e:  # a lost rank: the survivors shrink, as without re-join
            svc.recover(e)
        if svc.world_size != rep["sizes"][-1]:
            rep["sizes"].append(svc.world_size)
        if rep["gpus_first"] is None and svc.steps >= 3:
            rep["gpus_first"] = svc.rank_info()
            with open(status_path + ".tmp", "w") as f:
                json.dump(rj.sup.status(), f)
            os.replace(status_path + ".tmp", status_path)
        if rep["gpus_out"] is None and any(st["state"] != "mining" for st in rj.ranks.values()) \
                and svc.world_size < n:
            rep["gpus_out"] = svc.rank_info()

    leader.mine(bytes([0x51]))  # until the expected event
    while True:
        step()
        c = rj.counters
        if expect == "rejoin" and c["miner_rejoins_total"] >= 1:
            back = [g for g in rj.ranks if rj.ranks[g]["lives"] > 1]
            if hashes_at_rejoin is None:
                hashes_at_rejoin = {g: svc.rank_hashes.get(g, 0) for g in back}
                blocks_at_rejoin = {g: blocks_of(g) for g in back}
            if all(svc.rank_hashes.get(g, 0) > hashes_at_rejoin[g] for g in back) and \
                    (not shares_after or all(blocks_of(g) > blocks_at_rejoin[g] for g in back)):
                break
        elif expect == "refused" and c["miner_rejoin_refused_total"] >= 1:
            break
        elif expect == "failed" and c["miner_rejoin_failed_total"] >= 1:
            failed_at_step = failed_at_step or svc.steps
            if svc.steps >= failed_at_step + 20:
                break
    rep["height_at_event"] = state.height()
    req = leader.mine(bytes([0x52]), blocks=blocks)
    while not req.done.is_set():
        step()
    leader.shutdown()
    while svc.step():
        pass
    rj.wait_followers(30)
    kd = getattr(svc.dev, "kawpow", None)
    rep.update({"height": state.height(), "found": list(req.found), "windows": svc.windows,
                "world_size": svc.world_size, "hashes_total": svc.hashes_total, "stats": leader.stats,
                "steps": svc.steps, "rank_hashes": svc.rank_hashes, "hashes_at_rejoin": hashes_at_rejoin, "blocks_at_rejoin": blocks_at_rejoin,
                "gpus_last": svc.rank_info(), "per_rank": leader.per_rank, "counters": rj.counters,
                "exits": rj.exit_log, "reforms": svc.reforms, "membership": svc.membership,
                "exit_event_at": rj.last_event, "torch_in_supervisor": rj.sup.status()["torch_loaded"],
                "dag_builds": getattr(kd, "dag_builds", None),
                "dag_build_mode": {str(k): v for k, v in getattr(kd, "dag_build_mode", {}).items()},
                "dag_build_s": {str(k): v for k, v in getattr(kd, "dag_build_s", {}).items()}})
    with open(out_path, "w") as f:
        json.dump(rep, f)
    W.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
