"""A lost miner rank comes back (-minerrejoin): the GPU-free rank supervisor, the eligibility
policy, the solo / collective DAG rule, and gloo worlds on CPU devices that shrink and grow again
(3 -> 2 -> 3, 8 -> 7 -> 8), a rank that keeps failing, a newcomer that dies early, and the node."""
import json
import os
import signal
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CHILD = os.path.join(TESTS, "miner_rejoin_child.py")


def _load_supervisor():
    from nodexa_chain_core_amd.miner import supervisor

    return supervisor


def _wait_for(fn, timeout=10.0, what="condition"):
    deadline = time.monotonic() + timeout
    while time.monotonic() < deadline:
        v = fn()
        if v:
            return v
        time.sleep(0.02)
    raise AssertionError(f"timed out waiting for {what}")


def _gone(pid: int) -> bool:
    try:
        with open(f"/proc/{pid}/stat") as f:
            return f.read().rsplit(")", 1)[1].split()[0] == "Z"  # a zombie of ours has ended too
    except OSError:
        return True


# ------------------------------------------------------------------------------ 1. supervisor
def test_supervisor_spawns_reports_and_counts_lives(tmp_path):
    SV = _load_supervisor()
    sup = SV.SupervisorClient()
    try:
        events = []

        def exited(n):
            events.extend(e for e in sup.events() if e.get("event") == "exited")
            return len(events) >= n

        out0, out1 = tmp_path / "life0.json", tmp_path / "life1.json"
        sup.spawn(gpu=5, rank=2, world_size=3, env={"EXTRA": "x"}, argv=[CHILD, str(out0), "76"])
        _wait_for(lambda: exited(1), what="the first exit event")
        assert events[0] == {"event": "exited", "gpu": 5, "rank": 2, "life": 0, "code": 76}
        env0 = json.load(open(out0))
        assert env0 == {"RANK": "2", "WORLD_SIZE": "3", "LOCAL_RANK": "2", "NODEXA_MINER_DEVICE": "5",
                        "NODEXA_MINER_LIFE": "0", "NODEXA_MINER_JOIN_MEMBERSHIP": None, "EXTRA": "x"}
        # a second spawn for the same GPU is its next life
        sup.spawn(gpu=5, rank=2, world_size=3, env={}, join_membership=4, argv=[CHILD, str(out1), "0"])
        _wait_for(lambda: exited(2), what="the second exit event")
        assert events[1] == {"event": "exited", "gpu": 5, "rank": 2, "life": 1, "code": 0}
        env1 = json.load(open(out1))
        assert env1["NODEXA_MINER_LIFE"] == "1" and env1["NODEXA_MINER_JOIN_MEMBERSHIP"] == "4"
        st = sup.status()
        assert st["torch_loaded"] is False and st["children"] == [] and st["lives"] == {"2": 2}
        assert st["pid"] == sup.proc.pid
    finally:
        sup.stop()
    assert sup.proc.returncode == 0


def test_supervisor_ends_its_children_when_stdin_closes(tmp_path):
    SV = _load_supervisor()
    sup = SV.SupervisorClient()
    try:
        out = tmp_path / "sleeper.json"
        sup.spawn(gpu=0, rank=1, world_size=2, env={}, argv=[CHILD, str(out), "sleep"])
        _wait_for(out.exists, what="the sleeping child")
        (child,) = sup.status()["children"]
        assert child["rank"] == 1 and child["life"] == 0 and not _gone(child["pid"])
        t0 = time.monotonic()
        sup.proc.stdin.close()  # the node died
        assert sup.proc.wait(timeout=10) == 0
        assert _gone(child["pid"]) and time.monotonic() - t0 < 8
    finally:
        if sup.proc.poll() is None:
            sup.proc.kill()


# ------------------------------------------------------------------------------ 2. the GPU check
def test_assert_gpu_untouched():
    SV = _load_supervisor()
    clean = {0: "/dev/pts/0", 1: "pipe:[1]", 2: "/dev/null", 3: "/tmp/x/dev/kfd.txt", 4: "socket:[5]"}
    SV.assert_gpu_untouched(clean)
    with pytest.raises(SV.GpuTouched, match="/dev/kfd"):
        SV.assert_gpu_untouched({**clean, 7: "/dev/kfd"})
    with pytest.raises(SV.GpuTouched, match="renderD128"):
        SV.assert_gpu_untouched({**clean, 9: "/dev/dri/renderD128"})


# ------------------------------------------------------------------------------ 3. DAG build mode
def test_dag_build_mode(core):
    from nodexa_chain_core_amd.miner.search import WorldEpochView, dag_build_mode

    none = [set(), set(), set()]
    assert dag_build_mode([set(), set(), set()], none, 0) == "collective"   # everybody lacks it
    assert dag_build_mode([{0}, {0}, set()], none, 0) == "solo"             # one rank lacks it
    assert dag_build_mode([{0}, {0}, set()], none, 1) == "collective"       # the next one: nobody has it
    assert dag_build_mode([set(), set()], [set(), {3}], 3) == "solo"        # a peer is building it
    assert dag_build_mode(None, None, 0) == "solo"                          # a newcomer without records
    # the view a device keeps: the start of a world, a newcomer, a re-formed world, a vote
    first = WorldEpochView()
    assert first.mode(0, 3) == "collective"
    late = WorldEpochView(joined_late=True)
    assert late.mode(0, 3) == "solo"
    late.update([range(0, 1), range(0, 1), range(0)])
    assert late.mode(0, 3) == "solo" and late.mode(1, 3) == "collective"
    late.vote_passed(1)  # a unanimous vote step: pending everywhere from here on
    assert late.mode(1, 3) == "solo" and late.mode(2, 3) == "collective"
    late.update([range(0, 2)] * 3)  # resident everywhere: the vote is history
    assert late.voted == set()
    first.update([range(0)] * 3)
    first.reset()
    assert first.mode(0, 3) == "solo"


# ------------------------------------------------------------------------------ 4. eligibility
def test_rejoin_policy():
    SV = _load_supervisor()
    now = [1000.0]
    p = SV.RejoinPolicy(5.0, max_exits=3, window_s=600.0, clock=lambda: now[0])
    assert p.decide(now[0], 2) == "spawn"  # never lost: nothing to wait for
    p.record_exit(2)
    assert p.decide(1000.0, 2) == "wait" and p.decide(1004.9, 2) == "wait" and p.rejoin_in(1002.0, 2) == 3.0
    assert p.decide(1005.0, 2) == "spawn"
    now[0] = 1100.0
    p.record_exit(2)
    assert p.decide(1106.0, 2) == "spawn"
    now[0] = 1200.0
    p.record_exit(2)  # the third exit inside the window
    assert p.decide(1300.0, 2) == "refused" and p.rejoin_in(1300.0, 2) is None
    assert p.decide(1300.0, 1) == "spawn"  # other GPUs are not affected
    assert p.decide(1599.9, 2) == "refused"
    assert p.decide(1600.0, 2) == "spawn"  # the first exit has left the window
    off = SV.RejoinPolicy(0.0, clock=lambda: now[0])
    off.record_exit(1)
    assert off.decide(9999.0, 1) == "refused" and not off.enabled
    tr = SV.RejoinPolicy(5.0, torchrun=True, clock=lambda: now[0])
    tr.record_exit(1)
    assert tr.decide(9999.0, 1) == "refused" and not tr.enabled


# ------------------------------------------------------------------------------ 5-8. gloo worlds
def _start_world(tmp_path, n, *, expect="rejoin", blocks=2, timeout_s=4.0, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        e.pop(k, None)
    e.update({"NODEXA_TEST_RANKS": str(n), "NODEXA_TEST_EXPECT": expect, "NODEXA_TEST_BLOCKS": str(blocks),
              "NODEXA_MINER_WINDOW": "8", "NODEXA_MINER_COLLECTIVE_TIMEOUT": str(timeout_s),
              "NODEXA_MINER_WATCHDOG": "3", "NODEXA_MINER_WINDOWS_LOG": str(tmp_path / "follower{id}.json"),
              "NODEXA_TEST_REJOIN_DELAY": "0.3", "PYTHONPATH": ROOT, "OMP_NUM_THREADS": "1"})
    e.update(env or {})
    report, status = tmp_path / "rank0.json", tmp_path / "status.json"
    p = subprocess.Popen([sys.executable, os.path.join(TESTS, "miner_rejoin_rank0.py"), str(report), str(status)],
                         env=e, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return p, report, status


def _finish(p, report, timeout=280):
    try:
        out, _ = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        out, _ = p.communicate()
        raise AssertionError("the world did not finish:\n" + out.decode(errors="replace")[-6000:])
    out = out.decode(errors="replace")
    assert p.returncode == 0, out[-6000:]
    return json.load(open(report)), out


def _follower_logs(tmp_path):
    """The windows log of every follower process (the `{id}` of the path is the rank's id, and a
    later life appends `.life<k>`)."""
    return [json.load(open(p)) for p in sorted(tmp_path.glob("follower*.json*"))]


def _check_disjoint(rep, logs):
    """For every job, the windows of all ranks and all lives are pairwise disjoint."""
    by_job = {}
    for who, windows in [("rank0", rep["windows"])] + [(f"id{l['id']}/life{l['life']}", l["windows"]) for l in logs]:
        for job, start, count in windows:
            by_job.setdefault(job, []).append((start, start + count, who))
    shared = 0
    for job, ivs in by_job.items():
        ivs.sort()
        shared += len({w for *_x, w in ivs}) > 1
        for a, b in zip(ivs, ivs[1:]):
            assert a[1] <= b[0], f"job {job}: windows {a} and {b} overlap"
    return shared


def _check_back(tmp_path, rep, out, n, lost, first_code):
    """What tests 5 and 6 share: rank `lost` went (exit `first_code`) and came back."""
    life = {(e["rank"], e["life"]): e["code"] for e in rep["exits"]}
    assert life[(lost, 0)] == first_code, out[-4000:]
    assert life[(lost, 1)] == 0, out[-4000:]  # the second life ends at the stop packet
    assert all(code == 0 for (r, _l), code in life.items() if r != lost), life
    assert rep["sizes"] == [n, n - 1, n] and rep["world_size"] == n, rep["sizes"]
    assert rep["stats"]["bad_shares"] == 0 and rep["reforms"] == 1
    assert rep["height"] == rep["height_at_event"] + 2 and len(rep["found"]) == 2  # the requested height
    gpus = {g["id"]: g for g in rep["gpus_last"]}
    assert sorted(gpus) == list(range(n))
    assert gpus[lost]["lives"] == 2 and gpus[lost]["state"] == "mining" and gpus[lost]["last_exit"] == first_code
    assert all(g["lives"] == 1 and g["state"] == "mining" for i, g in gpus.items() if i != lost)
    # while it was out it kept its entry
    out_entry = {g["id"]: g for g in rep["gpus_out"]}
    assert sorted(out_entry) == list(range(n)) and out_entry[lost]["state"] in ("evicted", "rejoining")
    assert out_entry[lost]["rank"] == -1 and out_entry[lost]["alive"] is False
    # its hash count grew after the re-join
    assert rep["rank_hashes"][str(lost)] > rep["hashes_at_rejoin"][str(lost)]
    assert rep["counters"] == {"miner_rejoins_total": 1, "miner_rejoin_failed_total": 0, "miner_rejoin_refused_total": 0}
    assert rep["torch_in_supervisor"] is False
    logs = _follower_logs(tmp_path)
    lives = sorted((l["id"], l["life"]) for l in logs)
    # (a process that was killed wrote no log of its first life)
    assert lives == sorted([(r, 0) for r in range(1, n) if r != lost or first_code > 0] + [(lost, 1)]), lives
    second = next(l for l in logs if (l["id"], l["life"]) == (lost, 1))
    assert second["own_hashes"] > 0 and second["windows"] and second["world_size"] == n
    assert _check_disjoint(rep, logs) > 0
    return logs


def test_gloo_world3_rank_evicted_and_back(tmp_path, core):
    """3 -> 2 -> 3: rank 2 fails every window in its first life (exit 76), is started again after
    the delay, joins the survivors' next world and mines to the end."""
    from nodexa_chain_core_amd.miner.service import EXIT_DEVICE_FAILED

    p, report, _ = _start_world(tmp_path, 3, env={"NODEXA_MINER_FAILRATE": "1", "NODEXA_MINER_FAILRATE_RANK": "2",
                                                  "NODEXA_MINER_FAILRATE_LIVES": "1"})
    rep, out = _finish(p, report)
    logs = _check_back(tmp_path, rep, out, 3, 2, EXIT_DEVICE_FAILED)
    first = next(l for l in logs if (l["id"], l["life"]) == (2, 0))
    assert first["failures"] >= 3


def test_gloo_world8_rank_killed_and_back(tmp_path, core):
    """8 -> 7 -> 8: rank 3's process is killed from outside (its pid from the supervisor's status)."""
    p, report, status = _start_world(tmp_path, 8, timeout_s=20.0)
    try:
        _wait_for(status.exists, timeout=240, what="the world of 8 to mine")
        pid = next(c["pid"] for c in json.load(open(status))["children"] if c["rank"] == 3)
        os.kill(pid, signal.SIGKILL)
    except BaseException:
        p.kill()
        raise
    rep, out = _finish(p, report)
    _check_back(tmp_path, rep, out, 8, 3, -signal.SIGKILL)


def test_gpu_that_keeps_failing_is_refused(tmp_path, core):
    """The fail rate is on in every life and -minerrejoinmax is 2: after the second exit the rank
    stays evicted and the world ends at 2."""
    p, report, _ = _start_world(tmp_path, 3, expect="refused",
                                env={"NODEXA_MINER_FAILRATE": "1", "NODEXA_MINER_FAILRATE_RANK": "2",
                                     "NODEXA_TEST_REJOIN_MAX": "2"})
    rep, out = _finish(p, report)
    assert [(e["rank"], e["life"], e["code"]) for e in rep["exits"] if e["rank"] == 2] == [(2, 0, 76), (2, 1, 76)], out[-4000:]
    assert rep["world_size"] == 2 and rep["sizes"] == [3, 2, 3, 2]
    assert rep["counters"]["miner_rejoin_refused_total"] == 1 and rep["counters"]["miner_rejoins_total"] == 1
    entry = next(g for g in rep["gpus_last"] if g["id"] == 2)
    assert entry["state"] == "refused" and entry["lives"] == 2 and entry["last_exit"] == 76 and entry["rank"] == -1
    assert rep["stats"]["bad_shares"] == 0 and len(rep["found"]) == 2
    _check_disjoint(rep, _follower_logs(tmp_path))


def test_newcomer_that_dies_early_does_not_stall_the_survivors(tmp_path, core):
    """The re-spawned process exits 3 before it is ready: the attempt is cancelled and counts as a
    life, the survivors never get a FLAG_REFORM packet and keep mining."""
    argv = json.dumps([os.path.join(TESTS, "miner_rejoin_exit3.py")])
    p, report, _ = _start_world(tmp_path, 3, expect="failed",
                                env={"NODEXA_MINER_FAILRATE": "1", "NODEXA_MINER_FAILRATE_RANK": "2",
                                     "NODEXA_TEST_NEWCOMER_ARGV": argv})
    rep, out = _finish(p, report)
    assert [(e["rank"], e["life"], e["code"]) for e in rep["exits"] if e["rank"] == 2][:2] == [(2, 0, 76), (2, 1, 3)], out[-4000:]
    assert rep["reforms"] == 0 and rep["world_size"] == 2 and rep["sizes"] == [3, 2]
    assert rep["counters"]["miner_rejoin_failed_total"] >= 1 and rep["counters"]["miner_rejoins_total"] == 0
    entry = next(g for g in rep["gpus_last"] if g["id"] == 2)
    assert entry["lives"] >= 2 and entry["state"] in ("evicted", "rejoining", "refused") and entry["last_exit"] == 3
    survivor = next(l for l in _follower_logs(tmp_path) if l["id"] == 1)
    assert survivor["reforms"] == 0 and survivor["world_size"] == 2
    assert rep["stats"]["bad_shares"] == 0 and len(rep["found"]) == 2  # they kept mining


# ------------------------------------------------------------------------------ 9. the node
def _descendants(pid: int) -> list[int]:
    parent = {}
    for name in os.listdir("/proc"):
        if name.isdigit():
            try:
                with open(f"/proc/{name}/stat") as f:
                    parent[int(name)] = int(f.read().rsplit(")", 1)[1].split()[1])
            except OSError:
                pass
    out, todo = [], [pid]
    while todo:
        p = todo.pop()
        kids = [c for c, pp in parent.items() if pp == p]
        out += kids
        todo += kids
    return out


def test_node_brings_a_failing_rank_back(core, tmp_path):
    """nodexad -regtest -minerservice -minerranks=3 -minerrejoin=0.5 with rank 2 failing in its first
    life: getmininginfo shows 3 live ranks, then 2 and one evicted / rejoining, then 3 again; after
    stop neither a follower nor the supervisor is left."""
    import socket

    from nodexa_chain_core_amd.rpc.client import RPCClient

    addr = core.base58check_encode(bytes([42]) + bytes(range(20)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        rpc_port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", NODEXA_MINER_FAILRATE_RANK="2",
               NODEXA_MINER_FAILRATE_LIVES="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    node = subprocess.Popen([sys.executable, "-m", "nodexa_chain_core_amd.node", "-regtest",
                             "-kawpowactivationtime=1524179367", f"-datadir={tmp_path}", f"-rpcport={rpc_port}",
                             "-rpcuser=u", "-rpcpassword=p", f"-miningaddress={addr}", "-listen=0", "-printtoconsole=0",
                             "-minerservice", "-minerranks=3", "-minerrejoin=0.5", "-gpufailrate=1", "-gpuintensity=8",
                             "-minertargetbits=5", "-minercollectivetimeout=4", "-rest"], env=env, cwd=ROOT)
    c = RPCClient("127.0.0.1", rpc_port, "u", "p", timeout=30)
    pids = set()
    try:
        def up():
            try:
                return c.getblockcount() == 0
            except (OSError, RuntimeError):
                assert node.poll() is None, "nodexad exited"
                return False

        _wait_for(up, timeout=120, what="the node's RPC")
        pids |= set(_descendants(node.pid))
        assert len(pids) == 3  # the supervisor and its two followers
        c.setgenerate(True)
        seen = []

        def phase():
            gpus = c.getmininginfo()["gpus"]
            live = sum(1 for g in gpus if g["rank"] >= 0)
            states = sorted(g["state"] for g in gpus)
            want = len(seen)
            if want == 0 and live == 3 and states == ["mining"] * 3:
                seen.append(gpus)
            elif want == 1 and live == 2 and len(gpus) == 3 and states[0] in ("evicted", "rejoining"):
                seen.append(gpus)
            elif want == 2 and live == 3 and states == ["mining"] * 3 and max(g["lives"] for g in gpus) == 2:
                seen.append(gpus)
            return len(seen) == 3

        _wait_for(phase, timeout=150, what="3 -> 2 -> 3 in getmininginfo")
        back = next(g for g in seen[2] if g["id"] == 2)
        assert back["lives"] == 2 and back["last_exit"] == 76 and back["rank"] == 2
        pids |= set(_descendants(node.pid))
        assert len(pids) == 4  # the second life of rank 2 is a new process, under the same supervisor
        h = back["hashes"]
        _wait_for(lambda: next(g for g in c.getmininginfo()["gpus"] if g["id"] == 2)["hashes"] > h, timeout=60,
                  what="the re-joined rank to hash")
        assert c.getgpuinfo()[2]["state"] == "mining"
        c.setgenerate(False)
        assert c.getblockcount() > 0
        import urllib.request

        with urllib.request.urlopen(f"http://127.0.0.1:{rpc_port}/rest/metrics", timeout=30) as r:
            body = r.read().decode()
        line = next(x for x in body.splitlines() if "miner_rejoins_total" in x and not x.startswith("#"))
        assert float(line.split()[-1]) == 1.0, line
    finally:
        try:
            c.stop()
        except (OSError, RuntimeError):
            node.terminate()
        try:
            node.wait(timeout=90)
        except subprocess.TimeoutExpired:
            node.kill()
            raise
    assert node.returncode == 0
    assert all(_gone(p) for p in pids), [p for p in pids if not _gone(p)]
