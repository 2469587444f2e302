"""Gradient drift of the bf16 training step against the fp32 one, at the shapes that are actually trained.

One batch, one dropout seed, three engines over the same weights: bf16 on the compacted rows (the default step), bf16 on the
padded rows (compact_rows = False) and fp32 (PretrainEngine(..., precision="fp32"): every operand, activation and gradient in
fp32 -- the reference's arithmetic).  Prints, per bf16 engine, each parameter's relative L2 against the fp32 gradient (worst
and median; --all: every parameter) and the wall time of one forward + backward of each engine.

The fp32 engine draws the bf16 engine's dropout decisions on the PADDED layout; the compacted step indexes its row sites by
compact row, so with --dropout > 0 only the padded bf16 engine sees the same masks (the compacted one then differs by its
masks, not by its arithmetic).  Default: dropout 0.

    python tools/grad_drift.py --batch 36 --text 128 --regions 100
    python tools/grad_drift.py --batch 256 --text 128 --regions 100
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _rel(a, b):
    a, b = a.double(), b.double()
    floor = 2e-3 * (b.numel() ** 0.5)   # tests/test_gpu_train.py's floor (exactly-zero true gradients: key biases)
    return float((a - b).norm() / (b.norm() + floor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=36)
    ap.add_argument("--text", type=int, default=128)
    ap.add_argument("--regions", type=int, default=100)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()

    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch
    from visitron_amd.training import PretrainEngine

    dev = torch.device("cuda:0")
    cfg = BertConfig(hidden_dropout_prob=a.dropout, attention_probs_dropout_prob=a.dropout)
    torch.manual_seed(0)
    state = PreTrainOscar(cfg).state_dict()
    batch = make_batch(cfg, a.batch, a.text, a.regions, seed=1234, device=dev, with_labels=True)

    def run(precision, compact):
        model = PreTrainOscar(cfg)
        model.load_state_dict(state)
        model = model.to(dev).train()
        eng = PretrainEngine(model, precision=precision)
        eng.compact_rows = compact
        times = []
        for _ in range(2):   # the first call tunes / allocates; the second is timed
            eng.drop_seed_base, eng.fb_count = a.seed, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.forward_backward(batch)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        peak = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        del eng, model
        torch.cuda.empty_cache()
        return grads, float(out[0]), times[-1] * 1e3, peak

    ref, loss32, ms32, mem32 = run("fp32", False)
    rows = [dict(engine="fp32", loss=loss32, step_ms=round(ms32, 2), peak_gib=round(mem32, 1))]
    for name, compact in (("bf16 compacted", True), ("bf16 padded", False)):
        torch.cuda.reset_peak_memory_stats(dev)
        g, loss, ms, mem = run("bf16", compact)
        errs = sorted(((_rel(g[n], ref[n]), n) for n in ref), reverse=True)
        med = errs[len(errs) // 2][0]
        rows.append(dict(engine=name, loss=loss, step_ms=round(ms, 2), peak_gib=round(mem, 1), worst_rel_l2=errs[0][0],
                         worst_param=errs[0][1], median_rel_l2=med))
        if a.all:
            for e, n in errs:
                print("%-16s %-70s %.3e" % (name, n, e))
        del g
    print(json.dumps(dict(batch=a.batch, text=a.text, regions=a.regions, dropout=a.dropout, engines=rows)))


if __name__ == "__main__":
    main()
