"""Sharded DAG generation + RCCL all-gather (SURVEY §5 "DAG sharding").

Every GPU needs the whole DAG (each hash does 64 random 256-byte gathers, far
too fine-grained to serve over xGMI), but generating it is embarrassingly
parallel: rank r computes the r-th contiguous 1/world slice in place, then
one in-place `all_gather_into_tensor` replicates the slices. For a 4 GiB DAG
on 8 GPUs each rank ships 512 MiB, which RCCL moves over the xGMI mesh in tens
of milliseconds — small next to the generation it saves (8x less per GPU).
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import world as W


def allgather_shards(full: torch.Tensor, per: int) -> None:
    """In place: rank r's bytes [r*per, (r+1)*per) of `full` are replicated to every rank."""
    w = W.get()
    if not w.collective:
        return
    if full.numel() != per * w.world_size:
        raise ValueError("buffer must hold exactly world_size shards")
    mine = full[w.rank * per:(w.rank + 1) * per]
    if w.backend == "nccl":
        dist.all_gather_into_tensor(full, mine, group=w.group)
    else:  # gloo: no in-place all_gather_into_tensor, go through views of the same buffer
        parts = list(full.view(w.world_size, per).unbind(0))
        dist.all_gather(parts, mine.clone(), group=w.group)


def build_dag(epoch_dev) -> None:
    """Build `epoch_dev` (ops.ethash.DeviceEpoch): 1/world per rank, then all-gather."""
    w = W.get()
    if not w.collective:
        epoch_dev.build()
        return
    epoch_dev.build(shard=(w.rank, w.world_size))
    allgather_shards(epoch_dev.dag_padded(w.world_size), epoch_dev.shard_bytes(w.world_size))
    epoch_dev.mark_built()  # later kernels on this stream are ordered after the gather


# ---------------------------------------------------------------------------------------------
# Checked builds: every shard is digested by its owner and again by each rank that received it, a
# sample of the whole DAG is recomputed from the light cache, and the result is sealed. Two phases,
# so that a prebuild on a side stream never waits for the host: the queue phase only issues device
# work and asynchronous copies, `finish` reads them after the caller's stream synchronisation.

CHUNK_ITEMS = 16384  # ops/ethash.DAG_CHUNK_ITEMS (kept apart: this module must import without a GPU)
ITEM_BYTES = 64
SAMPLE_STRIDE = 256  # sampled audit of a fresh build: one item in 256


def table_len(shard_items: int) -> int:
    """Entries of a rank's padded digest table: a shard of n items touches at most ceil(n / chunk) + 1
    chunks of the global grid (both ends may be partial)."""
    return (shard_items + CHUNK_ITEMS - 1) // CHUNK_ITEMS + 1


def shard_of(rank: int, shard_items: int, items: int) -> tuple[int, int]:
    first = min(rank * shard_items, items)
    return first, min(shard_items, items - first)


def _chunks_of(first: int, count: int) -> int:
    return 0 if count <= 0 else (first + count - 1) // CHUNK_ITEMS - first // CHUNK_ITEMS + 1


class GatherCheck:
    """The digest tables of one checked all-gather: `owner[r]` is what rank r computed over its own
    shard before sending it, `got[r]` what this rank computed over the bytes it received. Tables are
    padded to `table_len`; entry j of rank r's row is global chunk first_r // CHUNK_ITEMS + j."""

    def __init__(self, rank: int, world_size: int, shard_items: int, items: int, owner: torch.Tensor,
                 got: torch.Tensor):
        self.rank, self.world_size, self.shard_items, self.items = rank, world_size, shard_items, items
        self.owner, self.got = owner, got  # (world, table_len) int64; the host copies by the time of finish()
        self.reported: list[tuple[int, int]] = []
        self.repaired_items = 0

    def differing(self) -> list[tuple[int, int]]:
        """(owner, global chunk) pairs whose received bytes do not digest to what the owner sent."""
        out = []
        for r in range(self.world_size):
            if r == self.rank:
                continue
            first, count = shard_of(r, self.shard_items, self.items)
            n = _chunks_of(first, count)
            bad = torch.nonzero(self.owner[r, :n] != self.got[r, :n]).flatten().tolist()
            out += [(r, first // CHUNK_ITEMS + j) for j in bad]
        return out

    def finish(self, digest_fn, repair_fn) -> list[tuple[int, int]]:
        """Repair every differing (owner, chunk) locally, digest it again and require the owner's
        value. Returns the pairs that differed; raises RuntimeError if one still does."""
        self.reported = self.differing()
        for r, chunk in self.reported:
            first, count = shard_of(r, self.shard_items, self.items)
            lo = max(first, chunk * CHUNK_ITEMS)
            hi = min(first + count, (chunk + 1) * CHUNK_ITEMS)
            n = repair_fn(lo, hi - lo)
            self.repaired_items += int(n or 0)
            now = int(digest_fn(lo, hi - lo).cpu()[0])
            if now != int(self.owner[r, chunk - first // CHUNK_ITEMS]):
                raise RuntimeError(f"rank {self.rank}: chunk {chunk} of rank {r}'s DAG shard still differs from its "
                                   f"owner's digest after a repair")
        return self.reported


def gather_queue(full: torch.Tensor, per: int, digest_fn, items: int | None = None) -> GatherCheck:
    """The device side of a checked gather, no host reads: digest this rank's shard, all-gather the
    shards and the (padded) tables, digest every other rank's shard as received.
    `digest_fn(first_item, count)` returns the per-chunk int64 digests of those items of `full` on
    `full`'s device (ops.ethash.DeviceEpoch.digest, or `_core.dag_digest` over a CPU tensor)."""
    w = W.get()
    ws, rank = (w.world_size, w.rank) if w.collective else (1, 0)
    if per % ITEM_BYTES:
        raise ValueError("a shard is a whole number of 64-byte items")
    si = per // ITEM_BYTES
    items = full.numel() // ITEM_BYTES if items is None else int(items)
    n = table_len(si)
    owner = torch.zeros((ws, n), dtype=torch.int64, device=full.device)
    got = torch.zeros((ws, n), dtype=torch.int64, device=full.device)
    first, count = shard_of(rank, si, items)
    if count:
        mine = digest_fn(first, count)
        owner[rank, :mine.numel()] = mine
    allgather_shards(full, per)
    allgather_shards(owner.view(-1).view(torch.uint8), n * 8)
    for r in range(ws):
        first, count = shard_of(r, si, items)
        if r != rank and count:
            theirs = digest_fn(first, count)
            got[r, :theirs.numel()] = theirs
    return GatherCheck(rank, ws, si, items, owner, got)


def gather_checked(full: torch.Tensor, per: int, digest_fn, repair_fn, items: int | None = None
                   ) -> list[tuple[int, int]]:
    """All-gather the shards of `full` in place and verify what arrived against each owner's digest;
    `repair_fn(first_item, count)` restores those items locally (from the light cache) and may return
    how many it rewrote. Returns the (owner, chunk) pairs that had to be repaired; raises
    RuntimeError when a repair does not bring a chunk to its owner's digest."""
    check = gather_queue(full, per, digest_fn, items)
    check.owner, check.got = check.owner.cpu(), check.got.cpu()
    return check.finish(digest_fn, repair_fn)


class DagCheck:
    """A checked DAG build in flight (`build_dag_checked`, `ops.ethash.DeviceEpoch.build_checked`).
    `finish()` is for after the build's stream has been synchronised: it compares the tables, repairs
    what differs and raises RuntimeError if the DAG cannot be made right."""

    def __init__(self, epoch_dev, gather: GatherCheck | None, sample_host: torch.Tensor, sample: tuple[int, int]):
        self.epoch_dev = epoch_dev
        self.gather = gather
        self.sample_host = sample_host  # pinned: the sampled audit's four words
        self.sample = sample            # (first item, stride)
        self.bad_chunks = 0             # (owner, chunk) pairs that arrived damaged
        self.repaired_items = 0
        self.done = False

    @property
    def events(self) -> int:
        """Findings of this build: damaged chunks received plus items the audits had to rewrite."""
        return self.bad_chunks + self.repaired_items

    def finish(self) -> "DagCheck":
        from ..ops.ethash import AuditResult

        e = self.epoch_dev
        e.finish_seal()
        reseal = False
        if self.gather is not None:
            def repair(first, count):
                return e.audit_result(first, count, repair=True).repaired

            bad = self.gather.finish(e.digest, repair)
            self.bad_chunks = len(bad)
            self.repaired_items += self.gather.repaired_items
            reseal = bool(bad)
        sampled = AuditResult.parse(self.sample_host)
        if sampled.mismatches:
            full = e.audit_result(repair=True)
            self.repaired_items += full.repaired
            again = e.audit_result()
            if again.mismatches:
                raise RuntimeError(f"epoch {e.epoch} DAG: {again.mismatches} items still differ from the light cache "
                                   f"after a full repair (first {again.first_bad})")
            reseal = True
        if reseal:
            e.seal()
        self.done = True
        return self


def sample_offset(epoch: int) -> int:
    """Where the sampled audit of epoch's build starts: another residue class of items each epoch."""
    return (int(epoch) * 97) % SAMPLE_STRIDE


def _queue_tail(epoch_dev, gather: GatherCheck | None) -> DagCheck:
    first = sample_offset(epoch_dev.epoch)
    words = epoch_dev.audit(first, stride=SAMPLE_STRIDE)
    epoch_dev.seal(wait=False)
    if gather is not None:
        gather.owner = epoch_dev.copy_to_pinned(gather.owner)
        gather.got = epoch_dev.copy_to_pinned(gather.got)
    return DagCheck(epoch_dev, gather, epoch_dev.copy_to_pinned(words), (first, SAMPLE_STRIDE))


def build_solo_checked(epoch_dev) -> DagCheck:
    """Build the whole DAG on this rank, audit a sample, seal: all queued on the current stream."""
    epoch_dev.build()
    return _queue_tail(epoch_dev, None)


def build_dag_checked(epoch_dev) -> DagCheck:
    """`build_dag` with the checks: queues, on the current stream, this rank's shard build and its
    digest, the all-gathers of shards and digest tables, a digest of every received shard, a sampled
    audit of the whole DAG, the seal, and the copies of all results to pinned memory. No host wait."""
    w = W.get()
    if not w.collective:
        return build_solo_checked(epoch_dev)
    epoch_dev.build(shard=(w.rank, w.world_size))
    gather = gather_queue(epoch_dev.dag_padded(w.world_size), epoch_dev.shard_bytes(w.world_size), epoch_dev.digest,
                          items=epoch_dev.items512)
    epoch_dev.mark_built()  # later kernels on this stream are ordered after the gather
    return _queue_tail(epoch_dev, gather)
