#!/usr/bin/env python
"""What visitron_amd.set_deterministic(True) costs: the two modes ALTERNATED in one process (drift of the clock or of a
neighbour's load hits both alike), on

  * the attention backward alone, S = 656 and S = 767 (three key blocks: atomics against planes + ordered sum);
  * the persistent weight-gradient kernel alone: an encoder layer's group at 14 592 rows (two row ranges per tile: ticket
    order against row-range order), and -- the launches that take fp32 atomics by default -- single 768 x 768 and
    768 x 3072 matrices at 2 x 767 rows, which the switch hands to the one-tile-per-workgroup kernel (timed under both
    hooks: 8 = the library's own routing, 128 = that kernel asked for by name);
  * the whole training step at 2 x 767 and at 8 x (511 + 256).

    python tools/deterministic_ab.py [--alternations 5] [--reps 20] [--out profiles/r08/deterministic_ab.txt]

Each figure is the median over the alternations of (HIP-event time of `reps` calls) / reps, with the smallest and largest
alternation beside it; "on/off" is the ratio of the medians.  The GEMM kernels are taken from the committed table in both
modes (VT_AUTOTUNE=0 unless it is set already), so that the step times differ by the two kernels only."""
import argparse
import os
import sys

os.environ.setdefault("VT_AUTOTUNE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

BF16 = torch.bfloat16


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps   # us per call


def alternate(ops, variants, alternations, reps):
    """variants: [(label, deterministic flag, callable)].  Warm each once, then `alternations` rounds in the given order."""
    times = {label: [] for label, _, _ in variants}
    for label, flag, fn in variants:
        ops.set_deterministic(flag)
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(alternations):
        for label, flag, fn in variants:
            ops.set_deterministic(flag)
            times[label].append(timed(fn, reps))
    ops.set_deterministic(False)
    return times


def report(out, title, times, base):
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out.append(title)
    for k, v in times.items():
        out.append("    %-34s median %10.1f us   min %10.1f   max %10.1f   x %.3f of %s" % (
            k, med[k], min(v), max(v), med[k] / med[base], base))
    print("\n".join(out[-(len(times) + 1):]), flush=True)


def attention_case(ops, dev, B, S, nh, drop):
    g = torch.Generator(device=dev).manual_seed(S)
    H = nh * 64
    qkv = torch.randn(B * S, 3 * H, generator=g, device=dev).to(BF16)
    dctx = (torch.randn(B * S, H, generator=g, device=dev) * 0.7).to(BF16)
    lse = torch.empty((B, nh, S), dtype=torch.float32, device=dev)
    dr = (0.1, 99, ops.site_attn(1)) if drop else ops.NO_DROP
    words = torch.zeros(ops.keep_words(B, nh, S), dtype=torch.int32, device=dev) if drop else None
    ctx = ops.attention_fwd(qkv, B, S, nh, lse=lse, drop=dr, keep_bits=words)
    out = torch.empty((B * S, 3 * H), dtype=BF16, device=dev)
    delta = torch.empty((B, nh, S), dtype=torch.float32, device=dev)
    ws = torch.empty(((S + 255) // 256) * B * S * H, dtype=torch.float32, device=dev)   # large enough for both modes
    return lambda: ops.attention_bwd(qkv, dctx, ctx, lse, B, S, nh, out=out, delta_ws=delta, dq32_ws=ws, drop=dr, keep_bits=words)


def wgrad_case(ops, dev, M, specs, mode):
    g = torch.Generator(device=dev).manual_seed(M)
    probs = []
    for N, K in specs:
        probs.append(dict(dy=(torch.randn(M, N, generator=g, device=dev) * 0.5).to(BF16),
                          x=torch.randn(M, K, generator=g, device=dev).to(BF16),
                          dw=torch.zeros(N, K, device=dev), db=torch.zeros(N, device=dev), accumulate=True))

    def run():
        ops.set_wgrad_kernel(mode)
        try:
            ops.wgrad(probs, M)
        finally:
            ops.set_wgrad_kernel(0)
    return run


def step_case(dev, B, T, R):
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch
    from visitron_amd.training import PretrainEngine

    cfg = BertConfig(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(0)
    model = PreTrainOscar(cfg).to(dev).train()
    eng = PretrainEngine(model, lr=5e-5, weight_decay=0.05, eps=1e-8, schedule="linear", warmup_steps=0, t_total=20000)
    batch = make_batch(cfg, B, T, R, seed=1234, device=dev, with_labels=True)
    return lambda: eng.train_step(batch)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--skip-step", action="store_true", help="kernels only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("deterministic_ab.py measures on the GPU: no HIP device here")
    from visitron_amd import ops

    dev = torch.device("cuda:0")
    out = ["# tools/deterministic_ab.py --alternations %d --reps %d --step-reps %d   (%s; VT_AUTOTUNE=%s)" % (
        a.alternations, a.reps, a.step_reps, torch.cuda.get_device_name(0), os.environ["VT_AUTOTUNE"])]
    layer = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
    try:
        for B, S in ((36, 656), (8, 767), (2, 767)):
            fn = attention_case(ops, dev, B, S, 12, True)
            report(out, "attention backward  B=%d S=%d nh=12 p=0.1 (keep words)" % (B, S),
                   alternate(ops, [("off (fp32 atomics)", False, fn), ("on (planes, ordered sum)", True, fn)], a.alternations, a.reps), "off (fp32 atomics)")
        fn = wgrad_case(ops, dev, 14592, layer, 0)
        report(out, "persistent wgrad  encoder layer group, M=14592 (two row ranges per tile)",
               alternate(ops, [("off (ticket order)", False, fn), ("on (row-range order)", True, fn)], a.alternations, a.reps), "off (ticket order)")
        for spec in ([(768, 768)], [(768, 3072)]):
            p8, p128 = wgrad_case(ops, dev, 2 * 767, spec, 8), wgrad_case(ops, dev, 2 * 767, spec, 128)
            report(out, "wgrad  %d x %d alone, M=2*767 (hook 8: three row ranges, fp32 atomics, by default)" % spec[0],
                   alternate(ops, [("off persistent (atomics)", False, p8), ("on (hook 8: handed to one-tile)", True, p8),
                                   ("on one-tile kernel", True, p128)], a.alternations, a.reps), "off persistent (atomics)")
        if not a.skip_step:
            for B, T, R in ((2, 511, 256), (8, 511, 256)):
                fn = step_case(dev, B, T, R)
                report(out, "training step  %d x (%d + %d), dropout 0.1" % (B, T, R),
                       alternate(ops, [("off", False, fn), ("on", True, fn)], a.alternations, a.step_reps), "off")
                del fn
                torch.cuda.empty_cache()
        out.append("wgrad turn timeouts: %d" % ops.wgrad_turn_timeouts())
        print(out[-1])
    finally:
        ops.set_deterministic(False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
