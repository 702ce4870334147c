"""A one-rank RCCL world that is re-formed (tests/test_gpu_miner_rejoin.py runs this as a fresh process).

parallel/world.init(force_collectives=True, store_port=...) makes a real "nccl" (= RCCL) process
group of one rank over the stand-alone rendezvous store. With NODEXA_MINER_REFORM_AT=3 rank 0 sends
a FLAG_REFORM packet on step 3: the loop communicator and the default group are destroyed and made
again on RCCL under the next store prefix (parallel/world.reform), and the loop mines on: a regtest
chain, KawPow at epoch 0, every share re-hashed on the host. This is the part of the RCCL re-form
that a box with one GPU can run. Writes a JSON report to argv[1]."""
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(out_path: str) -> int:
    import torch.distributed as dist

    from nodexa_chain_core_amd.chain.state import REGTEST_KAWPOW_FROM_GENESIS, ChainState, make_params
    from nodexa_chain_core_amd.miner import service as MS
    from nodexa_chain_core_amd.parallel import world as W

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        store_port = sk.getsockname()[1]
    w = W.init(use_gpu=True, force_collectives=True, timeout_s=60, collective_timeout_s=30, elastic=True,
               rank=0, world_size=1, store_port=store_port)
    assert w.backend == "nccl" and w.world_size == 1 and w.collective
    rep = {"backend": w.backend, "epoch_before": W.epoch()}
    state = ChainState(make_params("regtest", REGTEST_KAWPOW_FROM_GENESIS), None)
    leader = MS.ChainLeader(state, target_bits=int(os.environ.get("NODEXA_TEST_TARGET_BITS", "20")))
    window = 1 << 20
    dev = MS.make_rank_device(False, w.device.index, collective_dag=True, window=window)
    svc = MS.MiningService(dev, leader, window=window, collective_timeout_s=30)
    assert svc.comm.active and svc.comm.gpu and svc.reform_at == 3
    default_before, loop_before = dist.distributed_c10d._get_default_group(), svc.comm.group
    req = leader.mine(bytes([0x51]))
    t0 = time.time()
    blocks_at_reform = None
    while time.time() - t0 < 100:
        svc.step()
        if svc.reforms and blocks_at_reform is None:
            blocks_at_reform = leader.stats["blocks"]
            rep["step_of_reform"] = svc.steps
        if blocks_at_reform is not None and leader.stats["blocks"] >= blocks_at_reform + 3:
            break
    leader.shutdown()
    while svc.step():
        pass
    w2 = W.get()
    rep.update({"reforms": svc.reforms, "epoch_after": W.epoch(), "membership": svc.membership,
                "backend_after": w2.backend, "world_size": w2.world_size, "ids": list(w2.member_ids),
                "default_group_replaced": dist.distributed_c10d._get_default_group() is not default_before,
                "loop_group_replaced": svc.comm.group is not loop_before and svc.comm.group is not None,
                "loop_backend": dist.get_backend(svc.comm.group), "steps": svc.steps,
                "blocks_at_reform": blocks_at_reform, "stats": leader.stats, "height": state.height(),
                "found": len(req.found), "hashes_total": svc.hashes_total,
                "dag_builds": dev.kawpow.dag_builds, "dag_build_mode": {str(k): v for k, v in dev.kawpow.dag_build_mode.items()}})
    with open(out_path, "w") as f:
        json.dump(rep, f)
    dev.close()
    W.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
