"""DAG integrity on the host: the digest's host model (`_core.dag_digest`, the oracle of
hip/kernels/ethash_dag_check.hip), the checked all-gather of parallel/dag.py over gloo, the record's
STATUS_DAG_BAD bit and the `verifydag` RPC on a node without a GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384
M32 = 0xFFFFFFFF


def _mix(w: np.ndarray, g: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The digest's two per-word mixes written out from its definition, on uint64 masked to 32 bits."""
    w, g = w.astype(np.uint64), g.astype(np.uint64) & M32
    x = w ^ ((g * 0x9E3779B1) & M32)
    a = (x * 0x85EBCA6B) & M32
    a ^= a >> 13
    a = (a * 0xC2B2AE35) & M32
    a ^= a >> 16
    b = ((x ^ 0xA5A5A5A5) * 0x27D4EB2F) & M32
    b ^= b >> 15
    b = (b * 0x165667B1) & M32
    b ^= b >> 13
    return a, b


def _model(words: np.ndarray, first_item: int) -> list[int]:
    """numpy model of dag_digest over whole items (words: u32, 16 per item)."""
    out = []
    n = len(words) // 16
    lo = first_item
    while lo < first_item + n:
        hi = min(first_item + n, (lo // CHUNK + 1) * CHUNK)
        w = words[(lo - first_item) * 16:(hi - first_item) * 16]
        a, b = _mix(w, np.arange(lo * 16, hi * 16, dtype=np.uint64))
        out.append((int(a.sum()) & M32) | ((int(b.sum()) & M32) << 32))
        lo = hi
    return out


def _halves(d: int) -> tuple[int, int]:
    return d & M32, d >> 32


def _add(x: int, y: int) -> int:
    return ((x + y) & M32) | ((((x >> 32) + (y >> 32)) & M32) << 32)


def test_digest_golden_values(core):
    k = np.arange(1024, dtype=np.uint64)
    w = ((k * 2654435761 + 12345) % (1 << 32)).astype("<u4")
    assert core.dag_digest(w, 1000) == [0x60f1091b | (0xbf89d6f5 << 32)]
    # a single zero word at g = 0, by the definition; the host model agrees with the definition on
    # whole items (it takes nothing smaller), the zero item included
    a, b = _mix(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64))
    assert (int(a[0]), int(b[0])) == (0, 0x6f32d031)
    assert core.dag_digest(np.zeros(16, dtype="<u4"), 0) == _model(np.zeros(16, dtype="<u4"), 0)
    rng = np.random.default_rng(1)
    r = rng.integers(0, 1 << 32, size=16 * 300, dtype=np.uint64).astype("<u4")
    assert core.dag_digest(r, CHUNK - 100) == _model(r, CHUNK - 100)  # two chunks, both partial
    assert core.dag_digest(r, (1 << 28) - 7) == _model(r, (1 << 28) - 7)  # g wraps past 2^32
    assert core.dag_digest(r[:0], 5) == []
    assert core.dag_digest(r.tobytes(), 3) == core.dag_digest(r, 3)  # any buffer
    with pytest.raises(ValueError):
        core.dag_digest(r[:15], 0)


def test_digest_parts_add_up(core):
    """A range's digests equal the half-wise sums of its two parts', for splits next to and on the
    chunk grid (three chunks: 5 .. 5 + 2 * 16384 + 100)."""
    rng = np.random.default_rng(2)
    first, n = 5, 2 * CHUNK + 100
    w = rng.integers(0, 1 << 32, size=16 * n, dtype=np.uint64).astype("<u4")
    whole = core.dag_digest(w, first)
    assert len(whole) == 3
    for split in (1, 16383, 16384, 16385):
        left, right = core.dag_digest(w[:16 * split], first), core.dag_digest(w[16 * split:], first + split)
        c0 = first // CHUNK
        got = {}
        for base, part in ((first, left), (first + split, right)):
            for j, d in enumerate(part):
                c = base // CHUNK + j
                got[c] = _add(got.get(c, 0), d)
        assert [got[c0 + j] for j in range(3)] == whole, split


def test_digest_detects_bit_flips_and_swaps(core):
    rng = np.random.default_rng(3)
    n = 64
    w = rng.integers(0, 1 << 32, size=16 * n, dtype=np.uint64).astype("<u4")
    a0, b0 = _halves(core.dag_digest(w, 777)[0])
    for _ in range(512):
        i, bit = int(rng.integers(0, 16 * n)), int(rng.integers(0, 32))
        w[i] ^= np.uint32(1 << bit)
        a, b = _halves(core.dag_digest(w, 777)[0])
        w[i] ^= np.uint32(1 << bit)
        assert a != a0 and b != b0, (i, bit)
    s = w.copy()
    s[16 * 3:16 * 4], s[16 * 40:16 * 41] = w[16 * 40:16 * 41], w[16 * 3:16 * 4]
    assert core.dag_digest(s, 777) != core.dag_digest(w, 777)


# ----------------------------------------------------------------------------- gather_checked, 3 ranks

ITEMS = 100000  # shards of 33334 items: both shard boundaries fall inside a chunk


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        import torch

        from nodexa_chain_core_amd import _core
        from nodexa_chain_core_amd.parallel import dag as pdag
        from nodexa_chain_core_amd.parallel import world as W

        W.init(use_gpu=False)
        per_items = (ITEMS + world - 1) // world
        per = per_items * 64
        truth = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=per * world, dtype=np.uint8))
        truth[ITEMS * 64:] = 0  # the padding past the last item

        def fresh():
            full = torch.zeros(per * world, dtype=torch.uint8)
            full[rank * per:(rank + 1) * per] = truth[rank * per:(rank + 1) * per]
            return full

        def digest_of(full, before=None):
            def fn(first, count):
                if before is not None:
                    before(first, count)
                d = _core.dag_digest(full[first * 64:(first + count) * 64].numpy(), first)
                return torch.from_numpy(np.array(d, dtype=np.uint64).view(np.int64))
            return fn

        report = {}
        # 1. clean: nothing reported, no repair
        full, calls = fresh(), []
        report["clean"] = pdag.gather_checked(full, per, digest_of(full), lambda f, c: calls.append((f, c)), ITEMS)
        report["clean_calls"] = calls
        report["clean_equal"] = bool(torch.equal(full, truth))

        # 2./3. rank 2's copy of rank 0's shard is damaged after the gather, before it is compared:
        # when rank 2 is first asked for the digest of what it received from rank 0
        bad_item = 20000  # chunk 1, inside rank 0's shard [0, 33334)
        for name, restore in (("repaired", True), ("unrepaired", False)):
            full, calls, state = fresh(), [], {"damaged": False}

            def damage(first, count):
                if rank == 2 and not state["damaged"] and (first, count) == pdag.shard_of(0, per_items, ITEMS):
                    state["damaged"] = True
                    full[bad_item * 64:(bad_item + 1) * 64] = 0xA5

            def repair(first, count):
                calls.append((first, count))
                if restore:
                    full[first * 64:(first + count) * 64] = truth[first * 64:(first + count) * 64]
                return 1

            try:
                report[name] = pdag.gather_checked(full, per, digest_of(full, damage), repair, ITEMS)
            except RuntimeError as e:
                report[name] = "raised: " + str(e)
            report[name + "_calls"] = calls
            report[name + "_equal"] = bool(torch.equal(full, truth))
        W.barrier()
        W.shutdown()
        q.put((rank, report))
    except Exception as e:  # pragma: no cover - reported to the parent
        import traceback

        q.put((rank, traceback.format_exc() or repr(e)))


@pytest.mark.timeout(300)
def test_gather_checked_three_ranks(core):
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=280) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        rep = results[r]
        assert isinstance(rep, dict), rep
        assert rep["clean"] == [] and rep["clean_calls"] == [] and rep["clean_equal"], (r, rep)
        if r != 2:
            for name in ("repaired", "unrepaired"):
                assert rep[name] == [] and rep[name + "_calls"] == [] and rep[name + "_equal"], (r, name, rep)
    rep = results[2]
    # exactly (owner 0, chunk 1), and the repair gets that chunk's items of rank 0's shard
    assert rep["repaired"] == [(0, 1)] and rep["repaired_calls"] == [(CHUNK, CHUNK)] and rep["repaired_equal"], rep
    assert isinstance(rep["unrepaired"], str) and rep["unrepaired"].startswith("raised: "), rep
    assert rep["unrepaired_calls"] == [(CHUNK, CHUNK)] and not rep["unrepaired_equal"], rep


def test_table_len_covers_straddling_shards():
    from nodexa_chain_core_amd.parallel import dag as pdag

    per_items = (ITEMS + 2) // 3
    assert pdag.table_len(per_items) == 4
    for r in range(3):
        first, count = pdag.shard_of(r, per_items, ITEMS)
        assert (first + count - 1) // CHUNK - first // CHUNK + 1 <= pdag.table_len(per_items)
    assert pdag.shard_of(2, per_items, ITEMS) == (66668, 33332)


# ----------------------------------------------------------------------------- record bit, RPC

def test_record_carries_dag_bad(core):
    from nodexa_chain_core_amd.miner.search import SlotResult
    from nodexa_chain_core_amd.miner.service import STATUS_DAG_BAD, _REC_HEAD, RECORD_SIZE, pack_record, unpack_record

    assert STATUS_DAG_BAD == 64
    res = SlotResult(7, 0, 64, 64, [])
    plain, flagged = pack_record(res, epochs=[0]), pack_record(res, epochs=[0], dag_bad=True)
    assert len(plain) == len(flagged) == RECORD_SIZE
    assert not unpack_record(plain).dag_bad and unpack_record(flagged).dag_bad
    assert unpack_record(pack_record(None, dag_bad=True)).dag_bad
    # the bit is the only difference, and a record without it parses as before
    sp, sf = _REC_HEAD.unpack_from(plain, 0)[-2], _REC_HEAD.unpack_from(flagged, 0)[-2]
    assert sf == sp | STATUS_DAG_BAD and not sp & STATUS_DAG_BAD
    a, b = unpack_record(plain), unpack_record(flagged)
    b.dag_bad = False
    assert a == b and a.job_id == 7 and a.hashes == 64 and a.epochs == [0] and a.has_result and a.alive


def test_verifydag_without_gpu(core, tmp_path):
    from nodexa_chain_core_amd.node import Node
    from nodexa_chain_core_amd.rpc.client import CONVERT, RPCClient
    from nodexa_chain_core_amd.utils.config import ArgsManager

    addr = core.base58check_encode(bytes([42]) + bytes(range(20)))
    args = ArgsManager()
    args.parse_parameters(["-regtest", f"-datadir={tmp_path}", "-rpcport=0", "-rpcuser=u", "-rpcpassword=p",
                           f"-miningaddress={addr}", "-printtoconsole=0", "-kawpowactivationtime=1524179367"])
    n = Node(args)
    n.start()
    try:
        c = RPCClient("127.0.0.1", n.rpc.port, "u", "p")
        assert c.verifydag() == []
        assert c.verifydag(0, True, False) == []
        assert "verifydag" in c.help("verifydag")
    finally:
        n.stop()
    assert {("verifydag", 0), ("verifydag", 1), ("verifydag", 2)} <= CONVERT


def test_dag_flags_validate():
    from nodexa_chain_core_amd.utils.config import ArgsManager, dag_check_args

    def parse(*flags):
        a = ArgsManager()
        a.parse_parameters(list(flags))
        return dag_check_args(a)

    assert parse() == (None, None)
    assert parse("-dagcheck=0", "-dagscrub=2.5") == (False, 2.5)
    assert parse("-dagcheck=1") == (True, None)
    for bad in (("-dagcheck=maybe",), ("-dagscrub=-1",), ("-dagscrub=soon",)):
        with pytest.raises(ValueError):
            parse(*bad)
