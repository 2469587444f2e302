"""CPU, gloo, world 2 and 4: the collective wrappers of the sharded optimizer (visitron_amd.distributed) on a ragged plan --
after reduce_scatter_buckets every rank's own pieces hold exactly the all-reduce's values, after all_gather_buckets every
rank holds every owner's bits (the sign of a zero included), and the async-handle forms deliver on wait()."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from visitron_amd.distributed import ShardPlan, all_gather_buckets, all_reduce_ranges, reduce_scatter_buckets

# a ragged plan: atoms of 3, 1 and 5 granules of 64, a bucket of 176 elements (rounded down per world), fp32 class in the middle
TOTAL, N_DECAY = 9 * 64, 4 * 64
ATOMS = [(0, 192), (192, 256), (256, 576)]
FP32 = [(128, 320)]
BUCKET = 176


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _values(rank, dtype):
    g = torch.Generator().manual_seed(77 + rank)
    return torch.randn(TOTAL, generator=g).to(dtype)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        plan = ShardPlan(TOTAL, N_DECAY, ATOMS, FP32, world, rank, BUCKET)
        every = plan.everything()
        assert len(every.buckets) > len(ATOMS) and len({b[1] - b[0] for b in every.buckets}) > 1   # ragged
        launches = [plan.launch([ATOMS[2]]), plan.launch([ATOMS[0], ATOMS[1]])]                     # two ranges in one launch
        for dtype in (torch.float32, torch.bfloat16):
            # the yardstick: the bucketed all-reduce of the same ranges
            want = _values(rank, dtype)
            for la in launches:
                all_reduce_ranges(want, la.ranges, 100)
            # 1) reduce-scatter, blocking and with handles: the own pieces hold the all-reduce's bits
            for use_handles in (False, True):
                flat = _values(rank, dtype)
                handles = [] if use_handles else None
                for la in launches:
                    reduce_scatter_buckets(flat, la, plan, 100, async_handles=handles)
                if use_handles:
                    assert handles
                    for h in handles:
                        h.wait()
                for s, e, _, _, _ in every.own:
                    assert torch.equal(flat[s:e].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                       want[s:e].view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
            # 2) all-gather: each rank contributes its own pieces (everything else poisoned); afterwards every rank holds
            #    the owners' bits.  The owner's values carry -0.0 and infinities.
            bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
            owner_vals = []
            for r in range(world):
                v = _values(100 + r, dtype)
                v[::7] = -0.0
                v[3::11] = float("inf")
                owner_vals.append(v)
            full = torch.empty(TOTAL, dtype=dtype)
            for r in range(world):
                for s, e, _, _, _ in ShardPlan(TOTAL, N_DECAY, ATOMS, FP32, world, r, BUCKET).everything().own:
                    full[s:e] = owner_vals[r][s:e]
            assert bool((full == 0).any()) and bool((full.view(bits)[full == 0] < 0).all())   # the zeros are negative zeros
            for use_handles in (False, True):
                flat = torch.full((TOTAL,), 123.0, dtype=dtype)
                for s, e, _, _, _ in every.own:
                    flat[s:e] = owner_vals[rank][s:e]
                handles = [] if use_handles else None
                for la in launches:
                    all_gather_buckets(flat, la.buckets, plan, async_handles=handles)
                if use_handles:
                    mine = flat.clone()
                    for s, e, _ in every.others:     # nothing has been delivered before wait()
                        assert bool((mine[s:e] == 123.0).all())
                    for h in handles:
                        h.wait()
                assert torch.equal(flat.view(bits), full.view(bits))
        open(os.path.join(out_dir, "ok%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", (2, 4))
def test_shard_collectives_gloo(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert sorted(os.listdir(tmp_path)) == ["ok%d" % r for r in range(world)]
