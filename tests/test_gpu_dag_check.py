"""DAG integrity on the GPU (hip/kernels/ethash_dag_check.hip through ops/ethash.DeviceEpoch): the
digest against its host model, the audit of a built DAG, detection and repair of damage, the seal,
the scrub inside the search loop and the `verifydag` RPC. Epoch 0: 1 GiB, 16777186 items, so the
last of its 1024 chunks is partial."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 16384


@pytest.fixture(scope="module")
def ep(core, gpu):
    import torch

    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

    e = DeviceEpoch(0, device=0, ctx=core.get_epoch_context(0))
    e.build()
    torch.cuda.synchronize()
    assert e.l1_matches() and e.items512 == 16777186 and e.chunks == 1024
    yield e
    del e
    torch.cuda.empty_cache()


def _u64(t) -> list[int]:
    return [int(x) & 0xFFFFFFFFFFFFFFFF for x in t.cpu().tolist()]


def _flip(ep, item: int, quarters=(0, 1, 2, 3), bit: int = 3) -> None:
    """Flip one bit in each named 16-byte quarter of an item."""
    for q in quarters:
        ep.dag[item * 64 + q * 16 + 5] ^= 1 << bit


RANGES = [(0, 1), (5, 16383), (16384, 16384), (16383, 2), (7, 3 * CHUNK + 9), (-16354 - 3, 16357)]


@pytest.mark.parametrize("first,count", RANGES)
def test_digest_matches_host_model(core, ep, first, count):
    import torch

    if first < 0:
        first += ep.items512
        assert first + count == ep.items512  # reaches the last item
    piece = ep.dag[first * 64:(first + count) * 64]
    saved = piece.clone()
    try:
        piece.copy_(torch.randint(0, 256, (count * 64,), dtype=torch.uint8, device=ep.device,
                                  generator=torch.Generator(device=ep.device).manual_seed(first + count)))
        table = ep.digest(first, count)
        want = core.dag_digest(piece.cpu().numpy(), first)
        assert len(want) == (first + count - 1) // CHUNK - first // CHUNK + 1
        assert _u64(table) == want
    finally:
        piece.copy_(saved)
        torch.cuda.synchronize()


def test_digest_of_nothing_writes_nothing(ep):
    import torch

    table = torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=ep.device)
    assert ep.digest(12345, 0, out=table) is table
    assert ep.digest(12345, 0).numel() == 0
    torch.cuda.synchronize()
    assert table.cpu().tolist() == [0x5A5A5A5A5A5A5A5A] * 3
    with pytest.raises(ValueError):
        ep.digest(ep.items512 - 1, 2)


def test_audit_of_built_dag_is_clean(ep):
    n = ep.items512
    for first, count in ((0, 64), (1, 63), (n - 65, 65)):
        r = ep.audit_result(first, count)
        assert (r.mismatches, r.first_bad, r.repaired, r.checked) == (0, None, 0, count), (first, count, r)
    r = ep.audit_result(stride=4099)
    assert (r.mismatches, r.repaired, r.checked) == (0, 0, (n + 4098) // 4099)
    with pytest.raises(ValueError):
        ep.audit(n - 10, 11)
    with pytest.raises(ValueError):
        ep.audit(0, (n + 4098) // 4099 + 1, stride=4099)


def test_corruption_is_found_and_repaired(core, ep):
    import torch

    n = ep.items512
    tail_first, tail_count = 70001, 37  # a window that ends inside a wave and inside a workgroup
    items = sorted({0, tail_first + 18, n - 1, int(np.random.default_rng(11).integers(CHUNK, n - CHUNK))})
    assert len(items) == 4
    for i in items:
        _flip(ep, i)  # one bit in each of the item's four 16-byte quarters
    torch.cuda.synchronize()
    damaged = {i: ep.item512(i) for i in items}
    assert all(damaged[i] != core.dataset_item_512(ep.ctx, i) for i in items)

    r = ep.audit_result()
    assert (r.mismatches, r.first_bad, r.repaired, r.checked) == (4, 0, 0, n)
    assert {i: ep.item512(i) for i in items} == damaged  # an audit without repair writes nothing
    r = ep.audit_result(tail_first, tail_count)
    assert (r.mismatches, r.first_bad, r.checked) == (1, tail_first + 18, tail_count)
    r = ep.audit_result(repair=True)
    assert (r.mismatches, r.first_bad, r.repaired, r.checked) == (4, 0, 4, n)
    for i in items:
        assert ep.item512(i) == core.dataset_item_512(ep.ctx, i), i
    r = ep.audit_result()
    assert (r.mismatches, r.repaired, r.checked) == (0, 0, n)
    assert ep.l1_matches()


def test_seal_names_damaged_chunks_and_repair_restores_them(core, ep):
    import torch

    ep.seal()
    assert ep.seal_table.numel() == 1024 and ep.check_seal() == []
    a, b = 5 * CHUNK + 77, 1023 * CHUNK + 3  # the second in the partial last chunk
    _flip(ep, a, quarters=(2,))
    _flip(ep, b, quarters=(0, 3))
    torch.cuda.synchronize()
    assert ep.check_seal() == [5, 1023]
    assert ep.repair_chunks([5, 1023]) == [] and ep.last_repaired == 2
    assert ep.check_seal() == []
    assert ep.item512(a) == core.dataset_item_512(ep.ctx, a) and ep.item512(b) == core.dataset_item_512(ep.ctx, b)

    # a damaged light cache: the repair recomputes from wrong parents, so the chunk cannot come back
    # to its seal (or the audit disagrees with the resident items): the caller sees a non-empty result
    c = 300
    word = ep.light.view(torch.int32)[16 * 1000 + 3].clone()
    try:
        ep.light.view(torch.int32)[16 * 1000 + 3] ^= 0x10
        _flip(ep, c * CHUNK + 9, quarters=(1,))
        torch.cuda.synchronize()
        left = ep.repair_chunks([c])
        disagreeing = ep.audit_result(c * CHUNK, CHUNK).mismatches
        assert left == [c] or disagreeing, (left, disagreeing)
    finally:
        ep.light.view(torch.int32)[16 * 1000 + 3] = word
        torch.cuda.synchronize()
    assert ep.repair_chunks([c]) == []
    assert ep.check_seal() == [] and ep.audit_result(c * CHUNK, CHUNK).clean

    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

    with pytest.raises(ValueError):
        DeviceEpoch(0, device=0, ctx=ep.ctx, light_only=True).digest()
    with pytest.raises(ValueError):
        DeviceEpoch(0, device=0, ctx=ep.ctx, light_only=True).audit()


def test_checked_build_seals_and_finds_damage(core, gpu):
    """build_checked: build + sampled audit + seal queued without a host wait; finish() after a
    synchronisation. Damage done before finish() to an item of the sample is repaired there."""
    import torch

    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch
    from nodexa_chain_core_amd.parallel import dag as pdag

    e = DeviceEpoch(0, device=0, ctx=core.get_epoch_context(0))
    check = e.build_checked()
    assert e.seal_table is None and not check.done
    torch.cuda.synchronize()
    check.finish()
    assert check.done and check.events == 0 and e.seal_table.numel() == 1024 and e.check_seal() == []
    assert check.sample == (pdag.sample_offset(0), pdag.SAMPLE_STRIDE)

    # the same with an item of the sampled residue class damaged between the build and the audit
    e2 = DeviceEpoch(0, device=0, ctx=e.ctx)
    e2.build()
    item = pdag.sample_offset(0) + 1000 * pdag.SAMPLE_STRIDE
    _flip(e2, item, quarters=(3,))
    check = pdag._queue_tail(e2, None)
    torch.cuda.synchronize()
    check.finish()
    assert check.repaired_items == 1 and check.events == 1
    assert e2.item512(item) == core.dataset_item_512(e.ctx, item)
    assert e2.seal_table.tolist() == e.seal_table.tolist()  # sealed again after the repair
    del e, e2
    torch.cuda.empty_cache()


def test_scrub_in_the_search_loop(core, gpu):
    import torch

    from nodexa_chain_core_amd.miner.search import GpuSearchDevice, SearchPipeline, Work

    dev = GpuSearchDevice(0, jit_mode="off", dag_check=True, dag_scrub_s=0.05)
    height, hh = 4242, core.sha256d(b"scrub")
    w = Work(hh, bytes.fromhex("0001" + "ff" * 30), height, 1, 0, 0)  # ~1 in 32768 passes
    pipe = SearchPipeline(dev, watchdog_s=60)
    n = dev.block_for(height) * 512
    assert pipe.step(w, 0, n) is None
    e = dev.epochs[0]
    assert e.seal_table is not None and (dev.dag_scrubs, dev.dag_bad_chunks, dev.dag_repaired_items) == (0, 0, 0)
    item = 7 * CHUNK + 4321
    _flip(e, item, quarters=(2,))
    torch.cuda.synchronize()
    k = 1
    while dev.dag_bad_chunks == 0 and k < 4000:  # a few windows of ~1 ms each per 50 ms scrub interval
        pipe.step(w, k * n, n)
        k += 1
    assert (dev.dag_bad_chunks, dev.dag_repaired_items, dev.dag_check_events) == (1, 1, 1), k
    assert dev.dag_scrubs >= 1 and dev.dag_last_scrub_ms > 0
    assert dev.take_dag_bad() and not dev.take_dag_bad()
    assert e.item512(item) == core.dataset_item_512(e.ctx, item)
    shares = []
    while not shares and k < 8000:
        shares = pipe.step(w, k * n, n).shares
        k += 1
    pipe.drain()
    assert shares and all(sh.verify_full(height, hh, w.boundary, ctx=e.ctx) for sh in shares[:4])
    assert e.check_seal() == []
    dev.close()

    off = GpuSearchDevice(0, jit_mode="off", dag_check=False, dag_scrub_s=0.05)
    pipe = SearchPipeline(off, watchdog_s=60)
    pipe.step(w, 0, n)
    pipe.drain()
    assert off.epochs[0].seal_table is None and off.dag_scrub_s == 0
    for name in ("dag_scrubs", "dag_bad_chunks", "dag_repaired_items", "dag_last_scrub_ms", "dag_check_events"):
        assert not hasattr(off, name), name
    off.close()
    del dev, off, e
    torch.cuda.empty_cache()


def test_verifydag_rpc(core, gpu, tmp_path):
    from nodexa_chain_core_amd.node import Node
    from nodexa_chain_core_amd.ops import verify as V
    from nodexa_chain_core_amd.rpc.client import RPCClient
    from nodexa_chain_core_amd.utils.config import ArgsManager

    with V._epochs_lock:  # DAGs that earlier tests of this process left in the registry
        V._epochs.clear()
    addr = core.base58check_encode(bytes([42]) + bytes(range(20)))
    args = ArgsManager()
    args.parse_parameters(["-regtest", "-kawpowactivationtime=1524179367", f"-datadir={tmp_path}", "-rpcport=0",
                           "-rpcuser=u", "-rpcpassword=p", f"-miningaddress={addr}", "-printtoconsole=0", "-gpus=0",
                           "-kawpowjit=off"])
    n = Node(args)
    n.start()
    try:
        c = RPCClient("127.0.0.1", n.rpc.port, "u", "p", timeout=300)
        assert c.generatetoaddress(1, addr, 1 << 40) and c.getblockcount() == 1
        (r,) = c.verifydag()
        assert r["epoch"] == 0 and r["items"] == 16777186 and r["chunks"] == 1024
        assert r["sealed"] is True and r["bad_chunks"] == [] and r["mismatches"] == 0 and r["first_bad"] is None
        assert r["audited"] == (16777186 + 63) // 64 and r["repaired"] == 0 and r["ms"] > 0
        (r,) = c.verifydag(0, True)
        assert r["audited"] == r["items"] and r["mismatches"] == 0 and r["bad_chunks"] == []
        assert c.verifydag(5) == []
        g = c.getmininginfo()["gpus"][0]
        assert g["dag_check_events"] == 0 and g["dag_bad_chunks"] == 0 and g["dag_repaired_items"] == 0
    finally:
        n.stop()
