"""What one rank of the sharded optimizer launches per step, on one device: the base model's slab (113 M parameters), the
ownership plan at 64 MB buckets, rank 0's segments of an emulated world of 2, 4 and 8.  Alternating in one process:
  - adamw_flat over the whole slab (decay / no-decay: the two launches of the replicated step) -- the yardstick;
  - per world: the sharded AdamW launch set (one vt_shard_adamw per arrived range at three layers per chunk: heads, four
    layer chunks, tail) on rank 0's 1 / world of the slab, moments in shard-sized storage;
  - per world: the settle launch over the (world - 1) / world of the slab that rank 0 does not own.
Gradients are the bf16 communication copy (the default).  Bytes are what each kernel needs, counted from the plan: 28 per
updated element (p, m, v read and written, bf16 g read, bf16 mirror written), 6 per settled element.  No collective runs:
the time of the step on several devices is NOT measured here.
   python tools/shard_optim_bench.py [--rounds 7] [--window-ms 250]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--config", default="base", choices=("base", "mini"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "shard_optim_bench needs a HIP device"

    from visitron_amd import ops
    from visitron_amd.config import BertConfig, mini_config
    from visitron_amd.distributed import complement_ranges
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.training import ALIGN, PretrainEngine

    dev = torch.device("cuda:0")
    cfg = BertConfig() if args.config == "base" else mini_config(num_hidden_layers=4)
    model = PreTrainOscar(cfg)
    model.tie_weights()
    eng = PretrainEngine(model.to(dev), bucket_mb=64)
    f = eng.flat
    gen = torch.Generator(device=dev).manual_seed(1)
    f.g.copy_(torch.randn(f.total, device=dev, generator=gen) * 0.01)
    g16 = f.g.to(torch.bfloat16)
    hyper = (5e-5, 4.9e-5, 0.9, 0.999, 1e-8)

    def launch_ranges(per_chunk):   # what train_step launches: heads, layer chunks last first, the rest
        L = cfg.num_hidden_layers
        out, hi = [eng._param_ranges(eng._head_params())], L
        while hi > 0:
            lo = max(0, hi - per_chunk)
            out.append([(eng.layer_ranges[lo][k][0], min(ops.round_up(eng.layer_ranges[hi - 1][k][1], ALIGN), f.total)) for k in (0, 1)])
            hi = lo
        out.append(complement_ranges(f.total, [r for rng in out for r in rng]))
        return out

    def yardstick():
        for lo, hi, wd in ((0, f.n_decay, 0.05), (f.n_decay, f.total, 0.0)):
            ops.adamw_flat(f.p[lo:hi], g16[lo:hi], f.m[lo:hi], f.v[lo:hi], f.mirror[lo:hi], hyper[0], hyper[1], hyper[2], hyper[3],
                           hyper[4], wd, 0.5)

    variants = {"adamw_flat, whole slab (yardstick)": (28.0 * f.total, 2, 0, yardstick)}
    for world in (2, 4, 8):
        plan = eng.shard_plan(world, 0)
        m_sh, v_sh = (torch.zeros(plan.owned, device=dev) for _ in range(2))
        tabs = [ops.shard_adamw_table(f.p, g16, m_sh, v_sh, f.mirror, [(s, e, d, mo) for s, e, d, _, mo in plan.launch(r).own])
                for r in launch_ranges(3)]
        assert sum(t.numel for t in tabs) == plan.owned
        settle = ops.shard_settle_table(f.p, f.mirror, [(s, e, int(c)) for s, e, c in plan.everything().others])
        assert settle.numel == f.total - plan.owned

        def update(tabs=tabs):
            for t in tabs:
                ops.shard_adamw(t, True, hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], 0.05, 0.5)

        variants["shard_adamw, world %d, rank 0's launch set" % world] = (28.0 * plan.owned, len(tabs), sum(t.n_chunks for t in tabs), update)
        variants["shard_settle, world %d, not rank 0's" % world] = (6.0 * settle.numel, 1, settle.n_chunks, lambda s=settle: ops.shard_settle(s))

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    iters = {}
    for name, (_, _, _, fn) in variants.items():     # warm-up, and the repetitions that fill the window
        timed(fn, 3)
        iters[name] = max(10, int(args.window_ms / max(timed(fn, 10), 1e-3)))
    ms = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, (_, _, _, fn) in variants.items():
            ms[name].append(timed(fn, iters[name]))

    print("config %s: slab %d elements (%.1f MB fp32), n_decay %d; %d rounds, windows of ~%.0f ms; bf16 gradients"
          % (args.config, f.total, 4e-6 * f.total, f.n_decay, args.rounds, args.window_ms))
    print("%-46s %8s %8s %7s %9s %9s %9s %8s %7s %9s" % ("variant", "launches", "chunks", "iters", "us median", "min", "max", "MB", "TB/s",
                                                      "yard/this"))
    med = {}
    for name, (nbytes, launches, chunks, _) in variants.items():
        xs = sorted(ms[name])
        med[name] = xs[len(xs) // 2]
        y = med["adamw_flat, whole slab (yardstick)"]
        print("%-46s %8d %8d %7d %9.1f %9.1f %9.1f %8.1f %7.2f %9.2f" % (name, launches, chunks, iters[name], 1e3 * med[name], 1e3 * xs[0],
                                                                        1e3 * xs[-1], nbytes / 1e6, nbytes / med[name] / 1e9, y / med[name]))
    ys = sorted(ms["adamw_flat, whole slab (yardstick)"])
    print("yardstick spread over the rounds of this run: (max - min) / median = %.1f %%" % (100 * (ys[-1] - ys[0]) / ys[len(ys) // 2]))


if __name__ == "__main__":
    main()
