"""The per-period search kernel with the seed's words parked in LDS (no second seed keccak, the
hashes' mix seeds read from the parked words) against the host golden model, at epoch 0:
kawpow_hash_batch with a last workgroup that is not full, kawpow_search over three workgroups (the
parked seed feeds every hash of the group and kp_final), and one light-verify batch."""
import concurrent.futures as cf
import random

import pytest

pytestmark = pytest.mark.gpu

BLOCK = 768  # threads per workgroup of the tuned variant


def host_hashes(core, ctx, height, headers, nonces):
    with cf.ThreadPoolExecutor(16) as ex:  # kawpow_hash releases the GIL
        return list(ex.map(lambda hn: core.kawpow_hash(ctx, height, hn[0], hn[1]), zip(headers, nonces)))


@pytest.fixture(scope="module")
def epoch0(gpu, core):
    import torch

    from nodexa_chain_core_amd.ops.ethash import DeviceEpoch

    e = DeviceEpoch(0, device=0, ctx=core.get_epoch_context(0))
    e.build()
    torch.cuda.synchronize()
    return e


PERIODS = (0, 1)  # two programs, both compiled by build()


@pytest.mark.parametrize("which", [0, 1])
def test_hash_batch_every_job_vs_host(core, epoch0, which):
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher

    height = PERIODS[which] * 3 + 1
    s = KawpowSearcher(epoch0, height)
    assert s.block == BLOCK
    n = 2 * BLOCK + 5  # the last workgroup is not full, nor is its last 16-lane group
    rng = random.Random(100 + which)
    headers = [rng.randbytes(32) for _ in range(n)]
    nonces = [rng.getrandbits(64) for _ in range(n)]
    assert n % BLOCK and n % 16 and {0, 7, 8, 15} <= {j % 16 for j in range(n)}
    got = s.hash_batch(headers, nonces)
    want = host_hashes(core, epoch0.ctx, height, headers, nonces)
    bad = [j for j in range(n) if got[j] != want[j]]
    assert not bad, (len(bad), bad[:8])


def test_search_window_vs_host(core, epoch0):
    """Every nonce of a 3-workgroup window hashed on the host: the search must return exactly the
    nonces at or under the boundary, with the host's mix and final hashes."""
    from nodexa_chain_core_amd.ops.kawpow import KawpowSearcher

    height = PERIODS[0] * 3 + 2
    s = KawpowSearcher(epoch0, height)
    hh = core.sha256d(b"valu-search")
    start, n = 0x1234_5678_0000_0100, 3 * BLOCK
    host = host_hashes(core, epoch0.ctx, height, [hh] * n, range(start, start + n))
    boundary = bytes.fromhex("03" + "ff" * 31)  # 1 in 64 passes: 36 expected of 2304, under the 64-slot ring
    want = {start + i: fm for i, fm in enumerate(host) if core.hash_le(fm[0], boundary)}
    assert 8 <= len(want) < 64
    got = {sh.nonce: (sh.final_hash, sh.mix_hash) for sh in s.search(hh, start, n, boundary)}
    assert got == want


def test_light_verify_batch_vs_host(core, gpu):
    from nodexa_chain_core_amd.ops.verify import gpu_full_hash

    rng = random.Random(77)
    blocks = [rng.randrange(0, 7500) for _ in range(32)]
    headers = [rng.randbytes(32) for _ in blocks]
    nonces = [rng.getrandbits(64) for _ in blocks]
    res = gpu_full_hash(blocks, headers, nonces, device=0, mode="light")
    ctx = core.get_epoch_context(0)
    assert res == host_hashes_multi(core, ctx, blocks, headers, nonces)


def host_hashes_multi(core, ctx, blocks, headers, nonces):
    with cf.ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda a: core.kawpow_hash(ctx, *a), zip(blocks, headers, nonces)))
