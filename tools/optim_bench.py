"""The step between backward() and the next forward of the reference's loops, over the base model's parameter list with
random gradients: one iteration = clip_grad_norm_ + optimizer.step().  Four variants alternate in one process:
  (a) the pytorch-transformers AdamW as a torch loop (oracle.optim.AdamW) + torch.nn.utils.clip_grad_norm_
  (b) torch.optim.Adam + torch.nn.utils.clip_grad_norm_
  (c) visitron_amd.optim.AdamW + visitron_amd.optim.clip_grad_norm_
  (d) visitron_amd.optim.AdamW(max_grad_norm=...): the clip fused into the step
and the engine's ops.adamw_flat over one flat slab of the same size is the yardstick (update only, 28 B per parameter).
Bytes are what the algorithm needs: 28 per parameter for the update (p, m, v read and written, g read), 4 for the norm,
8 for the in-place scale.
   python tools/optim_bench.py [--config base|mini] [--rounds 5] [--iters 10]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29      # MI355X: HBM3E spec peak; measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="base", choices=("base", "mini"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-norm", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bench needs a HIP device"

    from oracle.optim import AdamW as TorchLoopAdamW
    from visitron_amd import ops, optim
    from visitron_amd.config import BertConfig, mini_config
    from visitron_amd.modeling import PreTrainOscar

    dev = torch.device("cuda:0")
    cfg = BertConfig() if args.config == "base" else mini_config()
    named = [(n, tuple(p.shape)) for n, p in PreTrainOscar(cfg).named_parameters()]
    no_decay = ("bias", "LayerNorm.weight")
    n_params = sum(int(torch.Size(s).numel()) for _, s in named)
    print("config %s: %d tensors, %d parameters (%.1f MB fp32); %d rounds x %d iterations, max_norm %g"
          % (args.config, len(named), n_params, 4e-6 * n_params, args.rounds, args.iters, args.max_norm))

    def groups(seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        ps = []
        for _, shape in named:
            p = torch.nn.Parameter(torch.randn(shape, device=dev, generator=gen) * 0.05)
            p.grad = torch.randn(shape, device=dev, generator=gen) * 0.01
            ps.append(p)
        decay = [p for (n, _), p in zip(named, ps) if not any(nd in n for nd in no_decay)]
        rest = [p for (n, _), p in zip(named, ps) if any(nd in n for nd in no_decay)]
        return ps, [{"params": decay, "weight_decay": 0.05}, {"params": rest, "weight_decay": 0.0}]

    variants = {}

    def add(name, nbytes, make):
        ps, gr = groups(len(variants))
        variants[name] = (nbytes, make(ps, gr))

    def torch_clip(ps, opt):
        def it():
            torch.nn.utils.clip_grad_norm_(ps, args.max_norm)
            opt.step()
        return it

    def hip_clip(ps, opt):
        def it():
            optim.clip_grad_norm_(ps, args.max_norm)
            opt.step()
        return it

    add("(a) torch-loop AdamW + torch clip", 40.0, lambda ps, gr: torch_clip(ps, TorchLoopAdamW(gr, lr=5e-5, eps=1e-8)))
    add("(b) torch.optim.Adam + torch clip", 40.0, lambda ps, gr: torch_clip(ps, torch.optim.Adam(ps, lr=5e-5)))
    add("(c) optim.AdamW + optim.clip_grad_norm_", 40.0, lambda ps, gr: hip_clip(ps, optim.AdamW(gr, lr=5e-5, eps=1e-8)))
    add("(d) optim.AdamW(max_grad_norm)", 32.0,
        lambda ps, gr: optim.AdamW(gr, lr=5e-5, eps=1e-8, max_grad_norm=args.max_norm).step)
    n_flat = n_params // 4 * 4
    flat = [torch.randn(n_flat, device=dev) * s for s in (0.05, 0.01)] + [torch.zeros(n_flat, device=dev) for _ in range(2)]
    variants["adamw_flat yardstick (update only)"] = (
        28.0, lambda: ops.adamw_flat(flat[0], flat[1], flat[2], flat[3], None, 5e-5, 5e-5, 0.9, 0.999, 1e-8, 0.05, 1.0))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    for _, fn in variants.values():      # warm-up: code objects, optimizer state, chunk tables
        for _ in range(3):
            fn()
    ms = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, (_, fn) in variants.items():
            ms[name].append(timed(fn))

    print("%-44s %9s %9s %9s %8s %7s %9s %9s" % ("variant", "ms median", "min", "max", "GB", "TB/s", "of 8.0", "of 6.29"))
    med = {}
    for name, (per_param, _) in variants.items():
        xs = sorted(ms[name])
        med[name] = xs[len(xs) // 2]
        gb = per_param * n_params / 1e9
        tbs = gb / med[name]
        print("%-44s %9.3f %9.3f %9.3f %8.2f %7.2f %8.1f%% %8.1f%%"
              % (name, med[name], xs[0], xs[-1], gb, tbs, 100 * tbs / HBM_SPEC_TBS, 100 * tbs / HBM_COPY_TBS))
    a, b, c, d, y = (med[k] for k in variants)
    print("ratios of the medians: (c)/(a) %.3f  (c)/(b) %.3f  (d)/(a) %.3f  (d)/(b) %.3f  (speed-up = 1 / ratio)"
          % (c / a, c / b, d / a, d / b))

    # the kernels of (c) and (d) alone (device events around each launch), beside the yardstick's
    ops.profile_begin()
    for _ in range(args.iters):
        variants["(c) optim.AdamW + optim.clip_grad_norm_"][1]()
        variants["adamw_flat yardstick (update only)"][1]()
    prof = ops.profile_end()
    print("per launch, events around each one (%d launches each):" % args.iters)
    for k in ("multi_sumsq", "norm_finish", "multi_scale", "multi_adam", "adamw_flat"):
        r = prof[k]
        print("  %-12s %8.3f ms  %6.2f TB/s" % (k, r["ms"] / r["n"], r["bytes"] / r["n"] / (r["ms"] / r["n"]) / 1e9))
    rate = lambda k: prof[k]["bytes"] / prof[k]["ms"]
    print("multi_adam runs at %.2f of adamw_flat's bytes/s in this run" % (rate("multi_adam") / rate("adamw_flat")))


if __name__ == "__main__":
    main()
