#!/usr/bin/env python
"""What each inference precision costs and delivers: set_precision(model, "fp32" | "bf16x3" | "bf16") ALTERNATED in rounds
in one process (drift of the clock or of a neighbour's load hits all three alike) on the trunk forward of the base config at
BASELINE configs[1]'s shape (B = 64, 128 text + 100 region tokens) and at B = 2.

    python tools/precision_ab.py [--rounds 7] [--reps 5] [--out profiles/r07/bf16x3.txt]

Per shape it prints
  * per mode the median over the rounds of (HIP-event time of `reps` forwards) / reps, the smallest and largest round, and
    the ratio of the medians to "fp32" -- a difference counts only where it exceeds the spread of the rounds;
  * the time of the two GEMM kernels inside one forward of the two fp32-route modes (ops.profile_begin / profile_end:
    gemm_* = the nn.Linear products, bmm_* = the two attention products), so that the ratio of the products alone stands
    beside the ratio of the forward (the derived ceiling of three bf16 MFMAs against sixteen fp32 issue slots is 16/3 = 5.3);
  * the max-abs difference of each mode's sequence_output to that of "fp32".

The bf16 GEMM kernels are taken from the committed table (VT_AUTOTUNE=0 unless it is set already): nothing is timed to choose
a kernel while the modes are being timed."""
import argparse
import os
import sys

os.environ.setdefault("VT_AUTOTUNE", "0")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

MODES = ("fp32", "bf16x3", "bf16")
TRUNK_KEYS = ("input_ids", "attention_mask", "img_feats", "img_location_embeddings")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps   # ms per call


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 2])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("precision_ab.py measures on the GPU: no HIP device here")
    from visitron_amd import ops, set_precision
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict, make_batch

    dev = torch.device("cuda:0")
    cfg = BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = PreTrainOscar(cfg).eval()
    model.load_state_dict(deterministic_state_dict(model, seed=0, weight_std=0.03))
    model.tie_weights()
    model = model.to(dev)
    out = ["# tools/precision_ab.py --rounds %d --reps %d   (%s; VT_AUTOTUNE=%s)" % (
        a.rounds, a.reps, torch.cuda.get_device_name(0), os.environ["VT_AUTOTUNE"])]

    def say(line):
        out.append(line)
        print(line, flush=True)

    for B in a.batches:
        batch = make_batch(cfg, B, seed=1234, device=dev)
        inputs = {k: batch[k] for k in TRUNK_KEYS}

        def forward():
            with torch.no_grad():
                return model.bert(**inputs)[0]

        say("trunk forward  base config, B=%d, 128 + 100 tokens (%d rows)" % (B, B * 228))
        seq, kern = {}, {}
        for mode in MODES:               # warm every mode's kernels and caches; keep its output; one profiled forward
            set_precision(model, mode)
            forward()
            seq[mode] = forward().float().clone()
            ops.profile_begin()
            forward()
            kern[mode] = ops.profile_end()
        times = {m: [] for m in MODES}
        for _ in range(a.rounds):
            for mode in MODES:
                set_precision(model, mode)
                times[mode].append(timed(forward, a.reps))
        med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
        for m in MODES:
            v = times[m]
            say("    %-8s median %9.3f ms   min %9.3f   max %9.3f   spread %4.1f %%   fp32 / this = %6.2f" % (
                m, med[m], min(v), max(v), 100.0 * (max(v) - min(v)) / med[m], med["fp32"] / med[m]))
        for m in ("fp32", "bf16x3"):
            for name in sorted(kern[m]):
                if name.startswith(("gemm_f32", "bmm_f32", "gemm_bf16x3", "bmm_bf16x3")):
                    k = kern[m][name]
                    say("    %-8s kernel %-12s %4d launches %9.3f ms   %7.1f TFLOP/s algorithmic" % (
                        m, name, k["n"], k["ms"], k["flops"] / (k["ms"] * 1e-3) / 1e12 if k["ms"] > 0 else 0.0))
        for a_name, b_name in (("gemm_f32", "gemm_bf16x3"), ("bmm_f32", "bmm_bf16x3")):
            if a_name in kern["fp32"] and b_name in kern["bf16x3"]:
                say("    products alone: %s / %s = %.2f   (ceiling 16/3 = 5.33)" % (
                    a_name, b_name, kern["fp32"][a_name]["ms"] / kern["bf16x3"][b_name]["ms"]))
        for m in MODES:
            say("    %-8s sequence_output max-abs difference to fp32: %.3e" % (m, float((seq[m] - seq["fp32"]).abs().max())))
        del seq, batch, inputs
        torch.cuda.empty_cache()
    set_precision(model, "bf16")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
