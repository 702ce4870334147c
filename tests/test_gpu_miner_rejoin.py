"""A lost miner rank comes back, on the GPU (-minerrejoin; miner/supervisor.py, miner/service.Rejoiner,
parallel/world.reform). Regtest KawPow at epoch 0 (a 1 GiB DAG), windows of 2^20 nonces, an easy
share target so that every rank finds blocks; every share is re-hashed on the host.

A. two ranks share GPU 0 and exchange over gloo (RCCL refuses two ranks on one device): rank 1 is
   evicted in its first life by the injected fail rate and comes back; its second life builds the
   DAG alone while rank 0 builds nothing again.
B. a one-rank RCCL world re-forms itself once (NODEXA_MINER_REFORM_AT): the default group and the
   loop communicator are destroyed and made again on RCCL under the next store prefix."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def _env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_one_rank_rccl_world_reforms(gpu, tmp_path):
    out = tmp_path / "reform.json"
    env = _env(NODEXA_MINER_REFORM_AT="3", NODEXA_TEST_TARGET_BITS="20", TORCH_NCCL_ASYNC_ERROR_HANDLING="0")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "rccl_reform_one_rank.py"), str(out)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-5000:])
    rep = json.load(open(out))
    print(json.dumps(rep))
    assert rep["backend"] == "nccl" and rep["backend_after"] == "nccl" and rep["loop_backend"] == "nccl"
    assert rep["reforms"] == 1 and rep["step_of_reform"] == 3
    assert rep["epoch_before"] == 0 and rep["epoch_after"] == 1 and rep["membership"] == 1
    assert rep["default_group_replaced"] and rep["loop_group_replaced"]
    assert rep["world_size"] == 1 and rep["ids"] == [0]
    # mining went on after the re-form, and every share passed the host's full re-hash
    assert rep["stats"]["blocks"] >= rep["blocks_at_reform"] + 3 and rep["height"] == rep["stats"]["blocks"]
    assert rep["stats"]["bad_shares"] == 0 and rep["stats"]["rejected"] == 0
    assert rep["dag_builds"] == 1 and rep["dag_build_mode"] == {"0": "collective"}  # the DAG outlives the re-form


def test_two_ranks_on_one_gpu_rank_evicted_and_back(gpu, tmp_path):
    report, status = tmp_path / "rank0.json", tmp_path / "status.json"
    env = _env(NODEXA_DIST_BACKEND="gloo", NODEXA_TEST_GPU="1", NODEXA_TEST_RANKS="2", NODEXA_TEST_EXPECT="rejoin",
               NODEXA_TEST_BLOCKS="2", NODEXA_TEST_SHARES_AFTER="1", NODEXA_TEST_TARGET_BITS="24",
               NODEXA_MINER_WINDOW=str(1 << 20), NODEXA_MINER_COLLECTIVE_TIMEOUT="30", NODEXA_TEST_GRACE="1",
               NODEXA_MINER_WATCHDOG="60", NODEXA_TEST_REJOIN_DELAY="0.001", NODEXA_TEST_DEADLINE="150",
               NODEXA_MINER_FAILRATE="1", NODEXA_MINER_FAILRATE_RANK="1", NODEXA_MINER_FAILRATE_LIVES="1",
               NODEXA_MINER_WINDOWS_LOG=str(tmp_path / "follower{id}.json"))
    r = subprocess.run([sys.executable, os.path.join(TESTS, "miner_rejoin_rank0.py"), str(report), str(status)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    rep = json.load(open(report))
    life0 = json.load(open(tmp_path / "follower1.json"))
    life1 = json.load(open(tmp_path / "follower1.json.life1"))
    # measured, not gated: the `exited` event -> the first completed window of the new life, and its DAG build
    print(json.dumps({"rejoin_s": round(life1["first_window_at"] - rep["exit_event_at"]["1"], 3),
                      "solo_dag_build_s": life1["dag_build_s"], "rank0_dag_build_s": rep["dag_build_s"],
                      "life0_dag_build_s": life0["dag_build_s"], "steps": rep["steps"], "height": rep["height"]}))
    assert [(e["rank"], e["life"], e["code"]) for e in rep["exits"]] == [(1, 0, 76), (1, 1, 0)]
    assert rep["sizes"] == [2, 1, 2] and rep["world_size"] == 2 and rep["reforms"] == 1
    assert rep["counters"] == {"miner_rejoins_total": 1, "miner_rejoin_failed_total": 0, "miner_rejoin_refused_total": 0}
    assert rep["torch_in_supervisor"] is False
    # the first world built the DAG together; the rank that came back built it alone, rank 0 nothing again
    assert life0["dag_build_mode"] == {"0": "collective"} and rep["dag_build_mode"] == {"0": "collective"}
    assert life1["dag_build_mode"] == {"0": "solo"} and life1["life"] == 1 and life1["world_size"] == 2
    assert rep["dag_builds"] == 1
    # blocks from rank 1 after the re-join, each re-hashed on the host: that is what proves its DAG
    assert rep["per_rank"]["1"]["blocks"] > rep["blocks_at_rejoin"]["1"] and life1["own_hashes"] > 0
    assert rep["stats"]["bad_shares"] == 0 and rep["per_rank"]["1"]["bad_shares"] == 0
    assert rep["height"] == rep["height_at_event"] + 2 and rep["height"] < 7500  # epoch 0 throughout
    gpus = {g["id"]: g for g in rep["gpus_last"]}
    assert gpus[1]["lives"] == 2 and gpus[1]["state"] == "mining" and gpus[1]["last_exit"] == 76
    assert gpus[1]["epochs_resident"] == [0] and gpus[0]["epochs_resident"] == [0]
    # for every job, the windows of both ranks and both lives are pairwise disjoint
    by_job = {}
    for who, windows in (("rank0", rep["windows"]), ("life0", life0["windows"]), ("life1", life1["windows"])):
        for job, start, count in windows:
            by_job.setdefault(job, []).append((start, start + count, who))
    shared = 0
    for job, ivs in by_job.items():
        ivs.sort()
        shared += len({w for *_x, w in ivs}) > 1
        for a, b in zip(ivs, ivs[1:]):
            assert a[1] <= b[0], f"job {job}: windows {a} and {b} overlap"
    assert shared > 0
