"""Oracles for the search kernels' tests: who qualifies in a nonce window, decided away from the
kernel that is under test.

Three kernels decide "does this nonce meet the target" on the device (kawpow_search /
kawpow_search_any: 64-bit prefix; x16r_hits: 256 bits, little-endian words; ethash_final_batch:
256 bits, big-endian bytes). Their tests compare them with one of these, never with themselves
(and never with `hash_batch` of the same code object):

* `oracle_rows` / `oracle_window`: every nonce of a KawPow window hashed by the static resident-DAG
  batch kernel kawpow_verify_dag, the prefix rule applied on the host;
* `host_window`: every nonce on the host golden model (`core.kawpow_hash`, light mode);
* plain Python integers for the compares and for the window arithmetic mod 2^64.
"""
import concurrent.futures as cf

import numpy as np

M64 = (1 << 64) - 1
M256 = (1 << 256) - 1
HEADER = bytes(range(1, 33))
G = 768                                   # the tuned variants' KP_BLOCK: the launch granule
START = 0x0123456789AB0000 + 5 * G        # non-zero high and low words


# ------------------------------------------------------------------ integers
def head64(final: bytes) -> int:
    """The 64 bits the KawPow search kernels test: bswap32(word 0) : bswap32(word 1) of the final
    hash, i.e. its first eight bytes as a big-endian number."""
    return int.from_bytes(final[:8], "big")


def le256_be(a: bytes, b: bytes) -> bool:
    """a <= b as 256-bit numbers written most significant byte first (KawPow and Ethash boundaries)."""
    return int.from_bytes(a, "big") <= int.from_bytes(b, "big")


def le256_le(a: bytes, b: bytes) -> bool:
    """a <= b as 256-bit numbers written least significant byte first (uint256 storage order: X16R)."""
    return int.from_bytes(a, "little") <= int.from_bytes(b, "little")


def in_window(nonce: int, start: int, n: int) -> bool:
    """nonce is one of the n nonces start, start + 1, ... counted mod 2^64."""
    return (nonce - start) % (1 << 64) < n


def boundary_for(prefix: int) -> bytes:
    """A 256-bit boundary whose full compare equals the 64-bit prefix test."""
    return prefix.to_bytes(8, "big") + b"\xff" * 24


def words_plain(h: bytes, order: str) -> bool:
    """No 32-bit word of the 256-bit number h (byte order `order`) is 0 or 0xffffffff: adding or
    subtracting 1 << 32 k changes word k alone."""
    v = int.from_bytes(h, order)
    return all(0 < (v >> 32 * k) & 0xFFFFFFFF < 0xFFFFFFFF for k in range(8))


# ------------------------------------------------------------------ KawPow windows
def as_set(shares):
    return {(s.nonce, s.mix_hash, s.final_hash) for s in shares}


_rows_cache: dict[tuple, list] = {}


def clear_cache() -> None:
    _rows_cache.clear()


def oracle_rows(ep, height, start, n, header=HEADER):
    """[(nonce, mix, final)] of the n nonces from `start` (mod 2^64), hashed by kawpow_verify_dag
    (one job per 16-lane group, program and mix in LDS). Computed once per window."""
    key = (ep.epoch, height, start, n, header)
    if key not in _rows_cache:
        import torch

        from nodexa_chain_core_amd.ops import runtime
        from nodexa_chain_core_amd.ops import verify as V

        nonces = [(start + i) & M64 for i in range(n)]
        jobs = V._pack_jobs([height] * n, [header] * n, nonces)
        with torch.cuda.device(ep.device):
            dj, progs, nprog, jp = V._grouped(jobs, ep.device)
            res = torch.empty(n * 16, dtype=torch.int32, device=ep.device)
            runtime.hip().launch_kawpow_verify_dag(
                runtime.static_kernel("kawpow_verify_light", "kawpow_verify_dag"), ep.dag.data_ptr(), ep.items2048,
                ep.l1.data_ptr(), dj.data_ptr(), progs.data_ptr(), nprog, jp.data_ptr(), n, res.data_ptr(),
                runtime.current_stream_handle())
            rows = res.cpu().numpy().view(np.uint8).reshape(n, 64)
        _rows_cache[key] = [(nonces[i], rows[i, :32].tobytes(), rows[i, 32:].tobytes()) for i in range(n)]
    return list(_rows_cache[key])


def oracle_window(ep, height, start, n, prefix, header=HEADER):
    """The rows of `oracle_rows` with head64(final) <= prefix: what a search of the window returns."""
    return [r for r in oracle_rows(ep, height, start, n, header) if head64(r[2]) <= prefix]


def host_window(core, ctx, height, header, start, n):
    """[(nonce, mix, final)] of the n nonces from `start` (mod 2^64) on the host golden model."""
    nonces = [(start + i) & M64 for i in range(n)]
    with cf.ThreadPoolExecutor(16) as ex:  # kawpow_hash releases the GIL
        out = list(ex.map(lambda x: core.kawpow_hash(ctx, height, header, x), nonces))
    return [(x, mix, fin) for x, (fin, mix) in zip(nonces, out)]
