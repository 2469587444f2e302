"""One rank of tests/test_gpu_shard_optimizer.py's multi-rank tests (launched by torch.distributed.run): the optimizer sharded
over the data-parallel ranks (PretrainEngine(shard_optimizer=True)) against the replicated engine on the same data, bit for
bit.  backend "gloo": every rank on cuda:0 (a rehearsal on one device); backend "nccl": rank r on cuda:r.

Two model instances with the same initial weights, one engine each.  The replicated engine takes every step with the SAME
layers_per_chunk as the sharded one: under gloo the reduce-scatter is emulated by the replicated step's own bucketed
all-reduce of the launched ranges, so the two engines then issue the same collectives over the same buffers and the sums
agree whatever order a backend adds four ranks in."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def main():
    backend = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend=backend)
    from visitron_amd import ops
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict, make_batch
    from visitron_amd.training import PretrainEngine

    ops.set_deterministic(True)
    ops.force_gemm_variant(1)             # one kernel variant everywhere: the comparison is then order-exact
    ops.set_wgrad_kernel(-8)
    cfg = mini_config(num_hidden_layers=4, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)

    def model():
        m = PreTrainOscar(cfg)
        m.load_state_dict(deterministic_state_dict(m, seed=5))
        m.tie_weights()
        return m.to(dev).train()

    def engine(m, shard, comm_dtype):
        e = PretrainEngine(m, lr=1e-3, weight_decay=0.05, schedule="constant", warmup_steps=0, bucket_mb=0.05,
                           grad_comm_dtype=comm_dtype, shard_optimizer=shard)
        e.compact_min_rows = 0
        return e

    batches = [{k: v.to(dev) for k, v in make_batch(cfg, 3, text_len=20, region_len=10, seed=100 + 10 * i + rank).items()}
               for i in range(5)]

    def step_pair(sh, rep, i, **kw):
        """One step of each engine on batch i with the same dropout seed; the two 7-tuples."""
        rep.fb_count = sh.fb_count
        a = sh.train_step(batches[i], **kw)
        b = rep.train_step(batches[i], **kw)
        torch.cuda.synchronize()
        as_t = lambda out: torch.stack([v.float() if torch.is_tensor(v) else torch.tensor(float(v), device=dev) for v in out])
        return as_t(a), as_t(b)

    def check_params(sh, rep, tag):
        """(ii): fp32-class parameters exact; bf16-class exact on owned pieces, float(mirror) elsewhere; mirror exact."""
        f, plan = sh.flat, sh.plan
        assert same(f.mirror, rep.flat.mirror), tag + ": mirror"
        every = plan.everything()
        assert sum(e - s for s, e, _, _, _ in every.own) * world == f.total
        for s, e, _, f32, _ in every.own:
            assert same(f.p[s:e], rep.flat.p[s:e]), (tag, "own", s, e, f32)
        for s, e, f32 in every.others:
            want = rep.flat.p[s:e] if f32 else f.mirror[s:e].float()
            assert same(f.p[s:e], want), (tag, "other", s, e, f32)
        # the model's parameters ARE the slab, and a mirror refreshed from them is the same mirror
        assert sh.flat.owns_params()
        assert same(f.p.to(torch.bfloat16), f.mirror), tag + ": refresh_mirror would not be idempotent"

    def check_state(sd_a, sd_b, tag):
        assert set(sd_a["state"]) == set(sd_b["state"])
        for n in sd_a["state"]:
            for k in ("exp_avg", "exp_avg_sq"):
                assert same(sd_a["state"][n][k], sd_b["state"][n][k]), (tag, n, k)
        for k in ("step_count", "sched_step", "fb_count"):
            assert sd_a[k] == sd_b[k], (tag, k)

    # precision="fp32" serves one rank, with or without the flag
    for shard in (False, True):
        try:
            PretrainEngine(model(), precision="fp32", shard_optimizer=shard)
            raise AssertionError("precision='fp32' under several ranks did not raise")
        except NotImplementedError as exc:
            assert "one rank" in str(exc)

    for comm_dtype in ("bf16", "fp32"):
        m_sh, m_rep = model(), model()
        sh, rep = engine(m_sh, True, comm_dtype), engine(m_rep, False, comm_dtype)
        rep.drop_seed_base = sh.drop_seed_base
        assert sh.shard and sh.world == world and sh.flat.m is None and sh.flat.v is None
        assert sh.m_sh.numel() * world == sh.flat.total == rep.flat.m.numel()
        assert (sh.g16 is not None) == (comm_dtype == "bf16")
        # (i) three overlapped steps, layers_per_chunk 1, 2, 3
        for i, per_chunk in enumerate((1, 2, 3)):
            a, b = step_pair(sh, rep, i, overlap=True, layers_per_chunk=per_chunk)
            assert same(a, b), (comm_dtype, "7-tuple", i, a.tolist(), b.tolist())
            assert bool(torch.isfinite(a[:4]).all())
            check_params(sh, rep, "%s step %d" % (comm_dtype, i))               # (ii)
        assert sh.step_count == rep.step_count == 3
        # (vi)
        try:
            sh.all_reduce_grads()
            raise AssertionError("all_reduce_grads() did not raise")
        except RuntimeError as exc:
            assert "optimizer_step()" in str(exc)
        # (iii) consolidate: p exact everywhere and equal across ranks; the optimizer state in the replicated format
        sh.consolidate()
        torch.cuda.synchronize()
        assert same(sh.flat.p, rep.flat.p), comm_dtype + ": consolidate"
        gathered = [torch.empty_like(sh.flat.p) for _ in range(world)] if backend == "gloo" else None
        if gathered is not None:
            dist.all_gather(gathered, sh.flat.p)
            assert all(same(g_, sh.flat.p) for g_ in gathered)
        sd_sh, sd_rep = sh.state_dict(), rep.state_dict()
        check_state(sd_sh, sd_rep, comm_dtype + ": state_dict")
        assert sd_sh["hyper"]["shard_optimizer"] is True and sd_rep["hyper"]["shard_optimizer"] is False
        # (iv) interchange: sharded state -> fresh replicated engine, replicated state -> fresh sharded engine, one more step
        m_sh2, m_rep2 = model(), model()
        m_sh2.load_state_dict(m_rep.state_dict())
        m_rep2.load_state_dict(m_sh.state_dict())     # (after consolidate: exact)
        sh2, rep2 = engine(m_sh2, True, comm_dtype), engine(m_rep2, False, comm_dtype)
        sh2.load_state_dict(sd_rep)
        rep2.load_state_dict(sd_sh)
        assert same(sh2.flat.p, rep2.flat.p) and same(sh2.flat.mirror, rep2.flat.mirror)
        a, b = step_pair(sh2, rep2, 3, overlap=True, layers_per_chunk=2)
        assert same(a, b), (comm_dtype, "7-tuple after interchange")
        check_params(sh2, rep2, comm_dtype + " interchange")
        sh2.consolidate()
        assert same(sh2.flat.p, rep2.flat.p)
        check_state(sh2.state_dict(), rep2.state_dict(), comm_dtype + ": interchange")
        # (v) overlap=False and forward_backward + optimizer_step(): the bits of the overlapped step (one layer per chunk: the
        # launches the un-overlapped path reduces)
        base_w, base_sd = {k: v.clone() for k, v in m_rep2.state_dict().items()}, rep2.state_dict()
        results = []
        for mode in ("overlap", "plain", "manual"):
            m3 = model()
            m3.load_state_dict(base_w)
            e3 = engine(m3, True, comm_dtype)
            e3.load_state_dict(base_sd)
            if mode == "overlap":
                e3.train_step(batches[4], overlap=True, layers_per_chunk=1)
            elif mode == "plain":
                e3.train_step(batches[4], overlap=False)
            else:
                e3.forward_backward(batches[4], grad_scale=1.0 / world)
                e3.optimizer_step(grad_scale=1.0 / world)
            torch.cuda.synchronize()
            assert e3.step_count == base_sd["step_count"] + 1 and e3.sched_step == base_sd["sched_step"] + 1
            results.append((e3.flat.p.clone(), e3.flat.mirror.clone(), e3.m_sh.clone(), e3.v_sh.clone()))
            last = e3
        for other in results[1:]:
            for x, y in zip(results[0], other):
                assert same(x, y), comm_dtype + ": un-overlapped step"
        # (vii) _force_comm with a no-op: the same kernels on the rank's own gradients, no collective issued
        calls = {"n": 0}
        real = (dist.all_reduce, dist.all_gather, dist.reduce_scatter_tensor, dist.all_gather_into_tensor)

        def counted(fn):
            def wrapper(*a_, **k_):
                calls["n"] += 1
                return fn(*a_, **k_)
            return wrapper

        dist.all_reduce, dist.all_gather, dist.reduce_scatter_tensor, dist.all_gather_into_tensor = map(counted, real)
        try:
            noop_ranges = []
            last.train_step(batches[0], _force_comm=lambda rng: noop_ranges.append(list(rng)))
            torch.cuda.synchronize()
        finally:
            dist.all_reduce, dist.all_gather, dist.reduce_scatter_tensor, dist.all_gather_into_tensor = real
        assert calls["n"] == 0 and len(noop_ranges) == 2 + 2   # heads, two chunks of (at most) three layers, tail
        assert bool(torch.isfinite(last.m_sh).all()) and bool(torch.isfinite(last.v_sh).all())
        assert bool(torch.isfinite(last.flat.p).all())
        del sh, rep, sh2, rep2, last
    dist.barrier()
    print("rank %d ok" % rank)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
