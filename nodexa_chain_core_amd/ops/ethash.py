"""Ethash epoch state resident on one MI355X: light cache + full DAG.

The light cache is built on the host (inherently serial keccak chain,
SURVEY K5) by `_core` and uploaded once; the DAG is generated on the GPU by
`ethash_dag_build` (hip/kernels/ethash_dag.hip) straight into a torch-owned
buffer. A 4 GiB DAG is 1.4 % of one GPU's 288 GB HBM3E, so several epochs can
stay resident (next-epoch prebuild, cross-epoch batch verification).

For multi-GPU nodes `build(shard=(rank, world))` computes only this rank's
contiguous slice in place; parallel/dag.py then all-gathers the slices over
RCCL ("DAG sharding").
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _core
from . import runtime
from ..utils.trace import traced

# 512-bit items per launch: keeps a single dispatch well under a second even
# at epoch 384 while still giving >> 256 CUs x 8 waves of work.
_DAG_CHUNK = 1 << 22
# DAG integrity (hip/kernels/ethash_dag_check.hip): items per digest chunk (1 MiB, global grid)
DAG_CHUNK_ITEMS = 16384
_U64 = (1 << 64) - 1


@dataclass(frozen=True)
class AuditResult:
    """The four words an audit leaves on the device."""
    mismatches: int
    first_bad: int | None  # lowest mismatching item index
    repaired: int
    checked: int

    @classmethod
    def parse(cls, words) -> "AuditResult":
        w = [int(x) & 0xFFFFFFFF for x in (words.tolist() if hasattr(words, "tolist") else words)]
        return cls(w[0], None if w[0] == 0 else w[1], w[2], w[3])

    @property
    def clean(self) -> bool:
        return self.mismatches == 0


def chunk_span(first: int, count: int, chunk_items: int = DAG_CHUNK_ITEMS) -> tuple[int, int]:
    """(first chunk, number of chunks) of the global grid that items [first, first + count) touch."""
    if count <= 0:
        return first // chunk_items, 0
    c0 = first // chunk_items
    return c0, (first + count - 1) // chunk_items - c0 + 1


# hashes per 16-lane row of ethash_hash_batch (EH_HASHES in hip/kernels/ethash_hashimoto.hip)
EH_HASHES = 2
# entries of ethash_search's hit list: a window with more hits than this is read back in full
ETHASH_MAX_HITS = 1024


class DeviceEpoch:
    def __init__(self, epoch: int, device: int | torch.device | None = None, ctx=None, world_size: int = 1,
                 light_only: bool = False):
        """`light_only`: keep just the light cache and the 16 KiB L1 on the device (light-mode
        batch verification, ops/verify.py) — no DAG allocation."""
        runtime.require_gpu()
        self.epoch = int(epoch)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device.index if isinstance(device, torch.device) else int(device)))
        self.ctx = ctx if ctx is not None else _core.get_epoch_context(self.epoch)
        self.full_items = int(self.ctx.full_items)          # 1024-bit items
        self.items512 = 2 * self.full_items
        self.items2048 = self.full_items // 2
        self.dag_bytes = self.items512 * 64
        with torch.cuda.device(self.device):
            self.light = torch.empty(int(self.ctx.light_bytes), dtype=torch.uint8, device=self.device)
            runtime.hip().memcpy_htod(self.light.data_ptr(), self.ctx.light_cache_ptr(), int(self.ctx.light_bytes))
            self.l1 = torch.tensor(self.ctx.l1, dtype=torch.int64).to(torch.int32).to(self.device)
            if light_only:
                self._storage = None
                self.dag = None
            else:
                # padded to a whole number of equal shards so RCCL can all-gather in place
                self._storage = torch.empty(self.shard_bytes(world_size) * world_size, dtype=torch.uint8,
                                            device=self.device)
                self.dag = self._storage[:self.dag_bytes]
        self.built = False
        self._audit_init = None  # pinned {0, 0xFFFFFFFF, 0, 0}: an audit's four words before it runs
        self.last_repaired = 0
        self._seal_pending = None
        self.seal_table: torch.Tensor | None = None  # per-chunk digests of the whole DAG, on the host (seal())

    # ------------------------------------------------------------------
    def shard_items(self, world: int) -> int:
        return (self.items512 + world - 1) // world

    def shard_bytes(self, world: int) -> int:
        return self.shard_items(world) * 64

    def dag_padded(self, world: int) -> torch.Tensor:
        n = self.shard_bytes(world) * world
        if n > self._storage.numel():
            raise ValueError("DeviceEpoch was allocated for a smaller world size")
        return self._storage[:n]

    def shard_range(self, rank: int, world: int) -> tuple[int, int]:
        """[first, first+count) 512-bit items owned by `rank` (equal contiguous slices)."""
        per = self.shard_items(world)
        first = min(rank * per, self.items512)
        return first, min(per, self.items512 - first)

    @traced("ethash.dag_build")
    def build(self, shard: tuple[int, int] | None = None, stream: int | None = None) -> None:
        if self.dag is None:
            raise ValueError("light-only DeviceEpoch has no DAG to build")
        h = runtime.hip()
        with torch.cuda.device(self.device):
            k = runtime.static_kernel("ethash_dag", "ethash_dag_build")
            s = runtime.current_stream_handle() if stream is None else stream
            first, count = (0, self.items512) if shard is None else self.shard_range(*shard)
            end = first + count
            pos = first
            while pos < end:
                n = min(_DAG_CHUNK, end - pos)
                h.launch_ethash_dag_build(k, self.light.data_ptr(), int(self.ctx.light_items), self.dag.data_ptr(),
                                          pos, n, s)
                pos += n
        if shard is None:
            self.built = True

    def build_checked(self, stream: int | None = None):
        """`build()` followed by a sampled audit and `seal()`, all queued without a host wait on the
        current stream. Returns the parallel.dag.DagCheck to `finish()` after a synchronisation."""
        from ..parallel import dag as pdag

        if stream is not None:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device)):
                return pdag.build_solo_checked(self)
        return pdag.build_solo_checked(self)

    def mark_built(self) -> None:
        self.built = True

    def l1_matches(self) -> bool:
        """The first 16 KiB of the device DAG equals the host-computed KawPow L1."""
        dev = self.dag[:16384].cpu().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        ref = torch.tensor(self.ctx.l1, dtype=torch.int64)
        return bool(torch.equal(dev, ref))

    # ------------------------------------------------------------------ integrity
    @property
    def chunks(self) -> int:
        return (self.items512 + DAG_CHUNK_ITEMS - 1) // DAG_CHUNK_ITEMS

    def _range(self, first: int, count: int | None) -> tuple[int, int]:
        if self.dag is None:
            raise ValueError("light-only DeviceEpoch has no DAG to check")
        first = int(first)
        count = self.items512 - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.items512:
            raise ValueError(f"items [{first}, {first + count}) are outside the DAG of {self.items512}")
        return first, count

    def digest(self, first: int = 0, count: int | None = None, stream: int | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
        """Per-chunk digests (`_core.dag_digest`'s definition) of items [first, first + count), as a
        device int64 tensor with one entry per chunk of the global grid that the range touches.
        Queued on the stream, no host wait. `out`: write into this int64 tensor's leading entries
        (it is returned whole) instead of a new one."""
        first, count = self._range(first, count)
        n = chunk_span(first, count)[1]
        with torch.cuda.device(self.device):
            k = runtime.static_kernel("ethash_dag_check", "ethash_dag_digest")
            table = torch.empty(n, dtype=torch.int64, device=self.device) if out is None else out
            if table.dtype != torch.int64 or table.numel() < n:
                raise ValueError("digest table must be int64 with one entry per chunk touched")
            s = runtime.current_stream_handle() if stream is None else stream
            runtime.hip().launch_ethash_dag_digest(k, self.dag.data_ptr(), self.items512, first, count,
                                                   DAG_CHUNK_ITEMS, table.data_ptr(), table.numel(), s)
        return table

    def audit(self, first: int = 0, count: int | None = None, stride: int = 1, repair: bool = False,
              stream: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Recompute items first + k * stride (k < count; default: as many as fit) from the light
        cache and compare them with the resident ones; with `repair`, rewrite the 16-byte pieces
        that differ. Returns the device int32 tensor of four words (AuditResult.parse), queued on
        the stream with no host wait. `out`: accumulate into this tensor (already initialised)."""
        stride = int(stride)
        if stride < 1:
            raise ValueError("audit stride must be positive")
        first, _ = self._range(first, 0)
        fit = (self.items512 - first + stride - 1) // stride
        count = fit if count is None else int(count)
        if count < 0 or count > fit:
            raise ValueError("audit range is outside the DAG")
        with torch.cuda.device(self.device):
            k = runtime.static_kernel("ethash_dag_check", "ethash_dag_audit")
            s = runtime.current_stream_handle() if stream is None else stream
            h = runtime.hip()
            if out is None:
                if self._audit_init is None:
                    self._audit_init = torch.tensor([0, -1, 0, 0], dtype=torch.int32).pin_memory()
                out = torch.empty(4, dtype=torch.int32, device=self.device)
                h.memcpy_async(out.data_ptr(), self._audit_init.data_ptr(), 16, s, "htod")
            pos = 0
            while pos < count:
                n = min(_DAG_CHUNK, count - pos)
                h.launch_ethash_dag_audit(k, self.light.data_ptr(), int(self.ctx.light_items), self.dag.data_ptr(),
                                          self.items512, first + pos * stride, stride, n, bool(repair),
                                          out.data_ptr(), s)
                pos += n
        return out

    def _host(self, t: torch.Tensor, stream: int | None) -> torch.Tensor:
        if stream is not None:  # a raw stream handle: torch's copy below runs on its own current stream
            runtime.hip().stream_synchronize(stream)
        return t.cpu()

    def audit_result(self, first: int = 0, count: int | None = None, stride: int = 1, repair: bool = False,
                     stream: int | None = None) -> AuditResult:
        """`audit`, waited for and parsed."""
        return AuditResult.parse(self._host(self.audit(first, count, stride, repair, stream), stream))

    def copy_to_pinned(self, t: torch.Tensor, stream: int | None = None) -> torch.Tensor:
        """Queue a copy of device tensor `t` to new pinned host memory; valid once the stream got there."""
        host = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        with torch.cuda.device(self.device):
            s = runtime.current_stream_handle() if stream is None else stream
            runtime.hip().memcpy_async(host.data_ptr(), t.data_ptr(), t.numel() * t.element_size(), s, "dtoh")
        host._nx_src = t  # the device tensor lives until the copy has been consumed
        return host

    def seal(self, stream: int | None = None, wait: bool = True) -> torch.Tensor | None:
        """Digest the whole DAG and keep the table (host int64) as `seal_table`: what `check_seal`
        compares later digests with. `wait=False` only queues the digest and its copy to pinned
        memory; `finish_seal()` adopts it once the stream has been synchronised."""
        self._seal_pending = self.copy_to_pinned(self.digest(stream=stream), stream)
        if not wait:
            return None
        with torch.cuda.device(self.device):
            runtime.hip().stream_synchronize(runtime.current_stream_handle() if stream is None else stream)
        return self.finish_seal()

    def finish_seal(self) -> torch.Tensor:
        self.seal_table = self._seal_pending.clone()
        self._seal_pending = None
        return self.seal_table

    def check_seal(self, stream: int | None = None) -> list[int]:
        """The chunks whose digest differs from the seal now."""
        if self.seal_table is None:
            raise RuntimeError("the DAG has no seal")
        return self.chunks_differing(self._host(self.digest(stream=stream), stream))

    def chunks_differing(self, table: torch.Tensor) -> list[int]:
        """Chunks at which a whole-DAG digest table (host) differs from the seal."""
        return torch.nonzero(table != self.seal_table).flatten().tolist()

    def repair_chunks(self, chunks, stream: int | None = None) -> list[int]:
        """Audit the listed chunks with repair, digest them again and return those that still differ
        from the seal (a damaged light cache, or a seal taken of a damaged DAG). The repaired item
        count of the call is left in `last_repaired`."""
        if self.seal_table is None:
            raise RuntimeError("the DAG has no seal")
        chunks = sorted({int(c) for c in chunks})
        words = None
        with torch.cuda.device(self.device):
            table = torch.empty(len(chunks), dtype=torch.int64, device=self.device)
        for i, c in enumerate(chunks):
            if not 0 <= c < self.chunks:
                raise ValueError(f"chunk {c} is outside the DAG")
            first = c * DAG_CHUNK_ITEMS
            n = min(DAG_CHUNK_ITEMS, self.items512 - first)
            words = self.audit(first, n, repair=True, stream=stream, out=words)
            self.digest(first, n, stream=stream, out=table[i:i + 1])
        if not chunks:
            self.last_repaired = 0
            return []
        now = self._host(table, stream)
        self.last_repaired = AuditResult.parse(words.cpu()).repaired
        return [c for c, d in zip(chunks, now.tolist()) if d != int(self.seal_table[c])]

    def item512(self, index: int) -> bytes:
        return bytes(self.dag[index * 64:(index + 1) * 64].cpu().numpy().tobytes())

    def hashimoto_batch(self, header_hashes: list[bytes], nonces: list[int], stream: int | None = None
                        ) -> list[tuple[bytes, bytes]]:
        """Classic Ethash (final_hash, mix_hash) of each (header hash, nonce) over this resident
        DAG (hip/kernels/ethash_hashimoto.hip; ethash::hash, src/crypto/ethash/lib/ethash/
        ethash.cpp:416-440), as `_core.ethash_hash` computes them on the host."""
        import struct

        if not self.built or self.dag is None:
            raise RuntimeError("hashimoto_batch needs the built DAG")
        n = len(nonces)
        if n != len(header_hashes):
            raise ValueError("one nonce per header hash")
        if n == 0:
            return []
        job = struct.Struct("<8IQII")
        buf = bytearray(job.size * n)
        for i, (hh, nonce) in enumerate(zip(header_hashes, nonces)):
            if len(hh) != 32:
                raise ValueError("header hashes are 32 bytes")
            job.pack_into(buf, i * job.size, *struct.unpack("<8I", hh), int(nonce), 0, 0)
        h = runtime.hip()
        ks = [runtime.static_kernel("ethash_hashimoto", f"ethash_{x}_batch") for x in ("seed", "mix", "final")]
        with torch.cuda.device(self.device):
            jobs = torch.frombuffer(buf, dtype=torch.uint8).to(self.device)
            out = torch.empty(n * 16, dtype=torch.int32, device=self.device)
            seeds = torch.empty(n * 16, dtype=torch.int32, device=self.device)
            s = runtime.current_stream_handle() if stream is None else stream
            h.launch_ethash_hash_batch(*ks, self.dag.data_ptr(), self.full_items, jobs.data_ptr(), n, out.data_ptr(),
                                       seeds.data_ptr(), s, EH_HASHES)
            raw = out.cpu().numpy().tobytes()
        return [(raw[i * 64 + 32:i * 64 + 64], raw[i * 64:i * 64 + 32]) for i in range(n)]

    def ethash_search(self, header_hash: bytes, boundary: bytes, start_nonce: int, iterations: int,
                      window: int = 1 << 22, max_hits: int = ETHASH_MAX_HITS) -> tuple[int, bytes, bytes] | None:
        """ethash::search (src/crypto/ethash/lib/ethash/ethash.cpp:326-350): the first nonce in
        [start_nonce, start_nonce + iterations) whose classic Ethash final hash is <= boundary, as
        (nonce, final_hash, mix_hash), or None. Nonces run on the device in windows of `window`
        (job i = start + i, no host-side job list); the final kernel appends each hit and the
        lowest one of the first window that has any is the answer. The hit list holds `max_hits`
        indices; of a window with more hits every final hash is read back and compared on the host."""
        if not self.built or self.dag is None:
            raise RuntimeError("ethash_search needs the built DAG")
        if len(header_hash) != 32 or len(boundary) != 32:
            raise ValueError("32-byte header hash and boundary")
        h = runtime.hip()
        ks = [runtime.static_kernel("ethash_hashimoto", f"ethash_{x}_batch") for x in ("seed", "mix", "final")]
        max_hits = int(max_hits)
        if max_hits < 1:
            raise ValueError("the hit list needs at least one entry")
        with torch.cuda.device(self.device):
            w = max(1, min(int(window), int(iterations)))
            out = torch.empty(w * 16, dtype=torch.int32, device=self.device)
            seeds = torch.empty(w * 16, dtype=torch.int32, device=self.device)
            hits = torch.zeros(1 + max_hits, dtype=torch.int32, device=self.device)
            s = runtime.current_stream_handle()
            done = 0
            while done < iterations:
                n = min(w, iterations - done)
                start = (int(start_nonce) + done) & 0xFFFFFFFFFFFFFFFF
                hits.zero_()
                h.launch_ethash_hash_batch(*ks, self.dag.data_ptr(), self.full_items, 0, n, out.data_ptr(),
                                           seeds.data_ptr(), s, EH_HASHES, bytes(header_hash), start, bytes(boundary),
                                           hits.data_ptr(), max_hits)
                got = hits.cpu().numpy().view("<u4")
                cnt = int(got[0])
                if cnt:
                    i = int(got[1:1 + min(cnt, max_hits)].min())
                    if cnt > max_hits:  # the ring overflowed: the lowest hit may be past it
                        raw = out[:n * 16].cpu().numpy().tobytes()
                        i = next(j for j in range(n) if raw[j * 64 + 32:j * 64 + 64] <= boundary)
                    row = out[i * 16:(i + 1) * 16].cpu().numpy().tobytes()
                    return (start + i) & 0xFFFFFFFFFFFFFFFF, row[32:], row[:32]
                done += n
        return None
