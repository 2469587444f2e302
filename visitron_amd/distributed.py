"""Data-parallel plumbing: one process per GPU, ``torch.distributed`` (backend "nccl" = RCCL over
xGMI on ROCm; "gloo" in the CPU tests).  The reference's only parallelism is DDP with bucketed
gradient all-reduce (tasks/viewpoint_select/pretrain.py:96-102,191) plus seven scalar all-reduces
for logged metrics (:169-189); here the gradients already live in ONE flat slab, so a bucket is a
slice of it -- no flatten/unflatten copies -- and the seven scalars travel as one 7-float message.
"""
import torch
import torch.distributed as dist


def bucket_ranges(n, bucket_elems):
    """[start, end) slices covering n elements, each <= bucket_elems (last one may be short)."""
    if bucket_elems <= 0:
        raise ValueError("bucket_elems must be positive")
    return [(s, min(n, s + bucket_elems)) for s in range(0, n, bucket_elems)]


def all_reduce_flat(flat, bucket_elems, group=None, async_handles=None):
    """In-place SUM all-reduce of a flat tensor in fixed-size buckets (several collectives in flight:
    on xGMI a ring is bound per link, so a few large messages keep every link busy)."""
    works = []
    for s, e in bucket_ranges(flat.numel(), bucket_elems):
        works.append(dist.all_reduce(flat[s:e], op=dist.ReduceOp.SUM, group=group, async_op=True))
    if async_handles is not None:
        async_handles.extend(works)
        return
    for w in works:
        w.wait()


def all_reduce_ranges(flat, ranges, bucket_elems, group=None, async_handles=None):
    """all_reduce_flat over a list of [start, end) element ranges of `flat` (e.g. the gradient slab
    regions of the encoder layers whose backward has just been enqueued)."""
    for s, e in ranges:
        if e > s:
            all_reduce_flat(flat[s:e], bucket_elems, group=group, async_handles=async_handles)


def complement_ranges(n, ranges):
    """[0, n) minus the given disjoint ranges, as a sorted list of ranges."""
    out, cur = [], 0
    for s, e in sorted(ranges):
        if s > cur:
            out.append((cur, s))
        cur = max(cur, e)
    if cur < n:
        out.append((cur, n))
    return out


def all_reduce_metrics(values, group=None):
    """The reference's 7x (x /= world; all_reduce(SUM)) of pretrain.py:169-189 as one message."""
    world = dist.get_world_size(group)
    t = torch.stack([v if torch.is_tensor(v) else torch.tensor(float(v), device=values[0].device) for v in values])
    t = t.to(torch.float32) / world
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return tuple(t.unbind(0))


def shard_batch(batch, rank, world):
    """Rank's contiguous slice of a global batch (what DistributedSampler amounts to for one step)."""
    out = {}
    for k, v in batch.items():
        n = v.shape[0]
        assert n % world == 0, "global batch must divide by world size"
        per = n // world
        out[k] = v[rank * per:(rank + 1) * per]
    return out


# ---- the optimizer sharded over the ranks: reduce-scatter, update, all-gather ------------------------------------------------
# An all-reduce is a reduce-scatter plus an all-gather; with AdamW between the two halves each rank updates 1 / world of the
# slab and keeps 1 / world of the moments, and the bytes on the wire stay what they were.  WHO owns WHAT is a static plan.
SHARD_WORLDS = (2, 4, 8)   # the divisors (> 1) of ALIGN / 8: every atom then cuts into whole pieces of 8 elements


class ShardLaunch(object):
    """What one launched list of ranges means under a plan: its buckets as (start, end, has_bf16, has_fp32), this rank's
    segments as (start, end, decay, fp32, moment_offset) and everybody else's as (start, end, fp32)."""

    def __init__(self, ranges, buckets, own, others):
        self.ranges, self.buckets, self.own, self.others = ranges, buckets, own, others
        self.own_elems = sum(e - s for s, e, _, _, _ in own)


class ShardPlan(object):
    """Static ownership of a flat slab of `total` elements by `world` ranks.

    atoms: disjoint [start, end) ranges covering the slab, each a multiple of ALIGN long -- the ranges the backward hands over
    one layer at a time; a range launched with several layers per chunk is a union of atoms, so the plan never depends on
    it.  Each atom is cut into buckets of at most bucket_elems elements (rounded down to a multiple of 8 * world), each
    bucket into `world` equal contiguous pieces, rank r owning the r-th: a piece is a multiple of 8 elements (16 bytes of
    bf16, 32 of fp32) and one contiguous in-place operand of reduce_scatter_tensor / all_gather_into_tensor.  A piece is cut
    into segments at n_decay (weight decay changes there) and at the edges of fp32_spans (the elements whose updated values
    travel back as fp32; all others travel back as bf16).  The moments of the owned pieces are stored back to back in slab
    order; a segment carries its place in that shard-sized storage."""

    def __init__(self, total, n_decay, atoms, fp32_spans, world, rank, bucket_elems):
        if world not in SHARD_WORLDS:
            raise ValueError("the sharded optimizer serves world sizes %s (the divisors of ALIGN / 8 = 8: every bucket must "
                             "cut into `world` pieces of whole 8-element groups), not %d" % (SHARD_WORLDS, world))
        if not 0 <= rank < world:
            raise ValueError("rank %d outside world %d" % (rank, world))
        self.total, self.n_decay, self.world, self.rank = int(total), int(n_decay), int(world), int(rank)
        self.bucket = int(bucket_elems) // (8 * world) * (8 * world)
        if self.bucket <= 0:
            raise ValueError("bucket_elems must hold at least 8 * world elements")
        self.atoms = sorted((int(s), int(e)) for s, e in atoms if e > s)
        cur = 0
        for s, e in self.atoms:
            if s != cur or (e - s) % (8 * world):
                raise ValueError("the atoms must cover the slab without gaps in multiples of 8 * world elements")
            cur = e
        if cur != self.total:
            raise ValueError("the atoms must cover the slab")
        self.fp32_spans = sorted((int(s), int(e)) for s, e in fp32_spans if e > s)
        self._cuts = sorted({self.n_decay} | {x for sp in self.fp32_spans for x in sp})
        # buckets per atom, and the shard-local moment offset of every owned piece (slab order)
        self._atom_buckets, self._moff, off = {}, {}, 0
        for s, e in self.atoms:
            bs = bucket_ranges(e - s, self.bucket)
            self._atom_buckets[(s, e)] = [(s + a, s + b) for a, b in bs]
            for a, b in self._atom_buckets[(s, e)]:
                ps, pe = self.piece(a, b, self.rank)
                self._moff[ps] = off
                off += pe - ps
        self.owned = off
        assert self.owned * world == self.total
        self._launches = {}

    def piece(self, bs, be, r):
        """Rank r's piece of the bucket [bs, be)."""
        n = (be - bs) // self.world
        return bs + r * n, bs + (r + 1) * n

    def is_fp32(self, x):
        """Travel class of element x."""
        return any(s <= x < e for s, e in self.fp32_spans)

    def segments(self, ps, pe):
        """[ps, pe) cut at n_decay and at the travel-class edges: (start, end, decay, fp32)."""
        pts = [ps] + [c for c in self._cuts if ps < c < pe] + [pe]
        return [(a, b, a < self.n_decay, self.is_fp32(a)) for a, b in zip(pts[:-1], pts[1:])]

    def buckets_of(self, ranges):
        """The buckets of the atoms that make up the given ranges (each range must be a union of atoms)."""
        out = []
        for s, e in ranges:
            if e <= s:
                continue
            inside = [a for a in self.atoms if s <= a[0] and a[1] <= e]
            if sum(b - a for a, b in inside) != e - s:
                raise ValueError("range [%d, %d) is not a union of the plan's atoms" % (s, e))
            for a in inside:
                out.extend(self._atom_buckets[a])
        return out

    def launch(self, ranges):
        key = tuple((int(s), int(e)) for s, e in ranges)
        got = self._launches.get(key)
        if got is None:
            buckets, own, others = [], [], []
            for bs, be in self.buckets_of(key):
                whole = self.segments(bs, be)
                buckets.append((bs, be, any(not f for _, _, _, f in whole), any(f for _, _, _, f in whole)))
                for r in range(self.world):
                    ps, pe = self.piece(bs, be, r)
                    for a, b, dec, f32 in self.segments(ps, pe):
                        if r == self.rank:
                            own.append((a, b, dec, f32, self._moff[ps] + (a - ps)))
                        else:
                            others.append((a, b, f32))
            got = self._launches[key] = ShardLaunch(list(key), buckets, own, others)
        return got

    def everything(self):
        """The whole plan as one launch."""
        return self.launch(self.atoms)


def reduce_scatter_buckets(flat, launch, plan, all_reduce_bucket_elems, group=None, async_handles=None):
    """SUM of `flat` over the ranks, delivered at least on each bucket's owner piece.  Backend nccl: one in-place
    reduce_scatter_tensor per bucket (the output is the rank's own piece of the input).  Any other backend has no
    reduce-scatter: the launched ranges go through the bucketed all-reduce the replicated step uses -- every piece, the
    owner's included, then holds the sum."""
    works = []
    if dist.get_backend(group) == "nccl":
        for bs, be, _, _ in launch.buckets:
            ps, pe = plan.piece(bs, be, plan.rank)
            works.append(dist.reduce_scatter_tensor(flat[ps:pe], flat[bs:be], op=dist.ReduceOp.SUM, group=group, async_op=True))
    else:
        all_reduce_ranges(flat, launch.ranges, all_reduce_bucket_elems, group=group, async_handles=works)
    if async_handles is not None:
        async_handles.extend(works)
        return
    for w in works:
        w.wait()


class _ListGather(object):
    """An all_gather in list form in flight: wait() puts the other ranks' pieces where they belong (plain copies: every bit,
    the sign of a zero included, arrives as it was sent)."""

    def __init__(self, work, parts, dests):
        self.work, self.parts, self.dests = work, parts, dests

    def wait(self):
        self.work.wait()
        for part, dest in zip(self.parts, self.dests):
            if dest is not None:
                dest.copy_(part)


def all_gather_buckets(flat, buckets, plan, group=None, async_handles=None):
    """Every rank's piece of each bucket [bs, be) of `flat` to every rank, in place.  Backend nccl: all_gather_into_tensor
    whose input is the rank's own piece of the output.  Any other backend: the list form into temporaries plus copies."""
    works = []
    nccl = dist.get_backend(group) == "nccl"
    for b in buckets:
        bs, be = b[0], b[1]
        ps, pe = plan.piece(bs, be, plan.rank)
        if nccl:
            works.append(dist.all_gather_into_tensor(flat[bs:be], flat[ps:pe], group=group, async_op=True))
        else:
            parts = [torch.empty_like(flat[ps:pe]) for _ in range(plan.world)]
            w = dist.all_gather(parts, flat[ps:pe], group=group, async_op=True)
            dests = [None if r == plan.rank else flat[slice(*plan.piece(bs, be, r))] for r in range(plan.world)]
            works.append(_ListGather(w, parts, dests))
    if async_handles is not None:
        async_handles.extend(works)
        return
    for w in works:
        w.wait()
