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


def main() -> int:
    ap = argparse.ArgumentParser()
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
