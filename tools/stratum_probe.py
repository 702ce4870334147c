#!/usr/bin/env python3
"""From a tip change at the node to the first window of the new job queued at the miner, over
loopback: the Stratum path (mining.notify pushed) against the getblocktemplate path (RemoteLeader:
one getbestblockhash round trip per step).

One process, so one clock: a regtest node (KawPow from block 1, CPU devices) with -stratumport and
RPC, and this engine's mining loop as its miner, on a GPU (--gpu N) or on the host (--cpu). The
node mines `--changes` blocks itself, one at a time; `updated_block_tip` stamps the change, and a
wrapper around the miner's device stamps the first `submit` of a window at the new height. The
wrapper also discards the miner's shares: on regtest nearly every hash is a block, and a miner
that moved the tip would measure itself.

    python tools/stratum_probe.py --gpu 0 [--changes 20] [--window 33554432] [--kawpowjit wait|auto|off]
                                  [--order stratum,getblocktemplate] [--markdown]

`--mode verify` needs no miner and no node: it measures the server's share checks alone. Two
servers with a `StaticJobSource` in this one process, one as a node without -stratumgpuverify and
without a miner sees it (no device: every share on the host) and one with -stratumgpuverify=1 on
`--gpu`, are sent the same pipelined `mining.submit` lines in turn (0, 1, 0, 1, ...): batches of
`--batches` submits written in one piece, at `--epochs`, `--repeats` timed rounds after `--warmups`
untimed ones, median (min-max) of submits answered per second. Every nonce is a share (the jobs'
block target is 2^256 - 1), its mix computed beforehand on the host. Then, per epoch, the time from
the start of a fresh -stratumgpuverify=1 server (no DAG resident; the host's light cache is in the
native cache after the warm-ups) until the first share it answers was hashed on its DAG, one share
being submitted after the other meanwhile.

    python tools/stratum_probe.py --mode verify --gpu 0 [--epochs 0,384] [--batches 1,16,256] [--markdown]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StampingDevice:
    """First submit time per height; no share leaves the device."""

    def __init__(self, inner):
        self.inner = inner
        self.first_submit: dict[int, float] = {}

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def submit(self, slot, work, start, count):
        self.first_submit.setdefault(work.height, time.perf_counter())
        self.inner.submit(slot, work, start, count)

    def wait(self, slot, timeout_s=None):
        res = self.inner.wait(slot, timeout_s)
        res.shares = []
        return res


def measure(node, addr, leader, dev, window: int, changes: int, on_stop=None) -> tuple[list[float], float]:
    """(interval per tip change in ms, the loop's mean step time in ms)."""
    from nodexa_chain_core_amd.chain.state import ValidationInterface
    from nodexa_chain_core_amd.miner.service import MiningService

    tip_time: dict[int, float] = {}

    class _Tip(ValidationInterface):
        def updated_block_tip(self, tip, fork, initial_download: bool) -> None:
            tip_time[tip.height] = time.perf_counter()

    listener = _Tip()
    node.state.register(listener)
    stamp = StampingDevice(dev)
    svc = MiningService(stamp, leader, window=window)
    stop = threading.Event()
    err = []

    def loop():
        try:
            while not stop.is_set():
                svc.step()
        except Exception as e:  # noqa: BLE001
            err.append(e)

    t = threading.Thread(target=loop, daemon=True)
    t.start()
    out = []
    rng = random.Random(1)
    t_start, steps_start = time.perf_counter(), svc.steps
    try:
        for _ in range(changes):
            h = node.state.height()
            deadline = time.monotonic() + 120
            while h + 1 not in stamp.first_submit:  # the miner works on the current tip's job
                if err or time.monotonic() > deadline:
                    raise RuntimeError(f"the miner never started height {h + 1}: {err}")
                time.sleep(0.002)
            time.sleep(rng.uniform(0.02, 0.27))  # not in step with the loop (a GPU window is ~0.11 s)
            node.miner.generate(node.mining_script, 1)
            while h + 2 not in stamp.first_submit:
                if err or time.monotonic() > deadline:
                    raise RuntimeError(f"the miner never started height {h + 2}: {err}")
                time.sleep(0.0005)
            out.append((stamp.first_submit[h + 2] - tip_time[h + 1]) * 1e3)
    finally:
        step_ms = (time.perf_counter() - t_start) * 1e3 / max(1, svc.steps - steps_start)
        stop.set()
        t.join(30)
        if on_stop is not None:
            on_stop()
        try:
            svc.pipe.drain()
        except Exception:  # noqa: BLE001
            pass
        node.state.unregister(listener)
    return out, step_ms


def _minmax(v: list[float], nd: int = 1) -> dict:
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd),
            "samples": [round(x, nd) for x in v]}


def verify_mode(a) -> int:
    import socket

    from nodexa_chain_core_amd import _core
    from nodexa_chain_core_amd.miner import stratum as S
    from nodexa_chain_core_amd.miner.stratum_server import ServerJob, StaticJobSource, StratumServer

    epochs = [int(x) for x in a.epochs.split(",")]
    batches = [int(x) for x in a.batches.split(",")]
    hh = _core.sha256d(b"stratum probe header")
    top = (1 << 256) - 1
    seq = [0]

    def server(flag: int):
        src = StaticJobSource()
        srv = StratumServer(src, device=a.gpu if flag else None, gpu_verify=bool(flag)).start()
        sock = socket.create_connection(("127.0.0.1", srv.port), timeout=120)
        f = sock.makefile("rb")
        sock.sendall(S.subscribe(1, "probe") + S.authorize(2, "probe", "x"))
        f.readline(), f.readline()
        return srv, src, sock, f

    def new_job(src, f, height: int) -> str:
        seq[0] += 1
        job = ServerJob("p%x" % seq[0], hh, height, top, 0x207FFFFF, True, "tip")
        src.push(job)
        while True:  # set_target (first job only), then the notify
            if S.decode(f.readline()).method == "mining.notify":
                return job.job_id

    def lines(job_id: str, shares) -> bytes:
        return b"".join(S.submit(10 + i, S.Submit("probe", job_id, n, hh, mix)) for i, (n, mix) in enumerate(shares))

    def answered(f, n: int) -> None:
        for _ in range(n):
            m = S.decode(f.readline())
            if m.result is not True:
                raise RuntimeError(f"a share was refused: {m.error}")

    out = {"mode": "verify", "device": f"gpu{a.gpu}", "repeats": a.repeats, "warmups": a.warmups, "rate": {}, "first_dag_share_ms": {}}
    for epoch in epochs:
        height = epoch * _core.EPOCH_LENGTH + 1
        ctx = _core.get_epoch_context(epoch)
        shares = [(n, _core.kawpow_hash(ctx, height, hh, n)[1]) for n in range(1 << 48, (1 << 48) + max(batches))]
        pair = {flag: server(flag) for flag in (0, 1)}
        try:
            job_id = new_job(pair[1][1], pair[1][3], height)
            deadline = time.monotonic() + 300
            while not (pair[1][0].epochs.ready(epoch) and pair[1][0].epochs.idle()):
                if time.monotonic() > deadline:
                    raise RuntimeError(f"no DAG of epoch {epoch}: {pair[1][0].info()}")
                time.sleep(0.01)
            for n in batches:
                rates = {0: [], 1: []}
                for rep in range(a.warmups + a.repeats):
                    for flag in (0, 1):
                        srv, src, sock, f = pair[flag]
                        job_id = new_job(src, f, height)
                        data = lines(job_id, shares[:n])
                        before = dict(srv.stats)
                        t0 = time.perf_counter()
                        sock.sendall(data)
                        answered(f, n)
                        dt = time.perf_counter() - t0
                        key = "verified_gpu" if flag else "verified_host"
                        if srv.stats[key] - before[key] != n:
                            raise RuntimeError(f"flag {flag}: the shares were not all hashed where they should be: {srv.stats}")
                        if rep >= a.warmups:
                            rates[flag].append(n / dt)
                out["rate"][f"epoch{epoch}_batch{n}"] = {f"gpuverify{flag}": _minmax(v) for flag, v in rates.items()}
            out.setdefault("dag_build_ms", {})[f"epoch{epoch}"] = pair[1][0].info()["dag_last_build_ms"]
        finally:
            for srv, _src, sock, _f in pair.values():
                sock.close()
                srv.stop()
        first, before_dag = [], []
        for rep in range(a.warmups + a.repeats):
            t0 = time.perf_counter()
            srv, src, sock, f = server(1)
            try:
                job_id = new_job(src, f, height)
                k = 0
                while srv.stats["verified_gpu"] == 0:
                    sock.sendall(lines(job_id, shares[k:k + 1]))
                    answered(f, 1)
                    k += 1
                    if k >= len(shares):
                        job_id, k = new_job(src, f, height), 0
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmups:
                    first.append(dt)
                    before_dag.append({"host": srv.stats["verified_host"], "light": srv.stats["verified_gpu_light"]})
            finally:
                sock.close()
                srv.stop()
        out["first_dag_share_ms"][f"epoch{epoch}"] = dict(_minmax(first), shares_before=before_dag)
    if a.markdown:
        print("| epoch | submits in one piece | -stratumgpuverify=0: shares/s median (min-max) | =1: shares/s median (min-max) |\n|---|---|---|---|")
        for key, v in out["rate"].items():
            e, n = key.split("_")
            c = [f"{v[f'gpuverify{i}']['median']} ({v[f'gpuverify{i}']['min']}-{v[f'gpuverify{i}']['max']})" for i in (0, 1)]
            print(f"| {e[5:]} | {n[5:]} | {c[0]} | {c[1]} |")
        print("\n| epoch | server start to first DAG-verified share, ms median (min-max) |\n|---|---|")
        for key, v in out["first_dag_share_ms"].items():
            print(f"| {key[5:]} | {v['median']} ({v['min']}-{v['max']}) |")
        print()
    print(json.dumps(out))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="tip", choices=("tip", "verify"))
    ap.add_argument("--epochs", default="0,384")
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--gpu", type=int, default=None)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--changes", type=int, default=20)
    ap.add_argument("--window", type=int, default=None)
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--kawpowjit", default="wait", choices=("wait", "auto", "off"),
                    help="the miner's -kawpowjit: with wait (its default) every third block, the first of a "
                         "ProgPoW period, also waits for that period's kernel")
    ap.add_argument("--order", default="stratum,getblocktemplate", help="which path is measured first")
    a = ap.parse_args()
    if a.mode == "verify":
        if a.gpu is None:
            ap.error("--mode verify needs --gpu")
        return verify_mode(a)
    cpu = a.cpu or a.gpu is None
    window = a.window or (8 if cpu else 1 << 25)

    from nodexa_chain_core_amd import _core
    from nodexa_chain_core_amd.miner.remote import RemoteLeader
    from nodexa_chain_core_amd.miner.service import make_rank_device
    from nodexa_chain_core_amd.miner.stratum_client import StratumConnection, StratumLeader
    from nodexa_chain_core_amd.node import Node
    from nodexa_chain_core_amd.rpc.client import RPCClient
    from nodexa_chain_core_amd.utils.config import ArgsManager

    addr = _core.base58check_encode(bytes([42]) + bytes(range(20)))
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        args = ArgsManager()
        args.parse_parameters(["-regtest", "-kawpowactivationtime=1524179367", f"-datadir={tmp}", "-rpcport=0",
                               "-rpcuser=u", "-rpcpassword=p", f"-miningaddress={addr}", "-printtoconsole=0",
                               "-stratumport=0"])
        node = Node(args)
        node.start()
        dev = make_rank_device(cpu, None if cpu else a.gpu, window=window, jit_mode=a.kawpowjit)
        try:
            for path in a.order.split(","):
                if path == "stratum":
                    conn = StratumConnection([("127.0.0.1", node.stratum.port)], "probe", "x").start()
                    results[path] = measure(node, addr, StratumLeader(conn), dev, window, a.changes, on_stop=conn.stop)
                else:
                    rpc = RPCClient("127.0.0.1", node.rpc.port, "u", "p", timeout=60.0)
                    results["getblocktemplate"] = measure(node, addr, RemoteLeader(rpc), dev, window, a.changes)
        finally:
            node.stop()
            dev.close()
    clocks = {}
    if not cpu:
        try:
            from nodexa_chain_core_amd.utils import gpuinfo

            clocks = gpuinfo.snapshot(a.gpu)
        except Exception as e:  # noqa: BLE001
            clocks = {"error": str(e)}
    summary = {"device": "cpu" if cpu else f"gpu{a.gpu}", "window": window, "changes": a.changes,
               "kawpowjit": a.kawpowjit, "clocks": clocks}
    for k, (v, step_ms) in results.items():
        summary[k] = {"mean_step_ms": round(step_ms, 3), "median_ms": round(statistics.median(v), 3), "max_ms": round(max(v), 3),
                      "min_ms": round(min(v), 3), "samples_ms": [round(x, 3) for x in v]}
    if a.markdown:
        print(f"device {summary['device']}, window {window} nonces, -kawpowjit={a.kawpowjit}, {a.changes} tip changes, "
              f"clocks {json.dumps(clocks)}\n")
        print("| path (in the order measured) | median ms | max ms | min ms | mean loop step ms |\n|---|---|---|---|---|")
        for k in results:
            s = summary[k]
            print(f"| {k} | {s['median_ms']} | {s['max_ms']} | {s['min_ms']} | {s['mean_step_ms']} |")
        print()
    print(json.dumps(summary))
    return 0


if __name__ == "__main__":
    sys.exit(main())
