#!/usr/bin/env python
"""What freezing part of the model saves, and that an all-trainable step costs what it did: the base configuration at
36 x (128 + 100) and 256 x (128 + 100) through PretrainEngine.train_step, and 8 x 511 text-only through OscarEncoder
(forward + loss.backward(): the trunk node of the autograd bridge; no optimizer in the timed window).

    python tools/partial_training_bench.py [--old ab_old] [--rounds 3] [--reps 10] [--out profiles/r18/partial_training.txt]

  * all-trainable, this build against another build of the project (--old: a tree of the parent commit, built; left out
    when the directory is missing): child processes ALTERNATED old, new, new, old, old, new, ... -- each child imports one tree, runs
    the three cases and prints one figure per case; the report gives both builds' medians and their own run-to-run spreads;
  * frozen patterns against this build's all-trainable step, alternated IN one process (requires_grad is read at every
    step, so the same engine serves every pattern): the word table; the bottom six layers + embedding block + region
    group; the heads only (everything under `bert.` but the pooler frozen; not defined for the encoder case, whose trunk
    has no heads -- a fully frozen trunk takes the inference path);
  * the launch census of one step per pattern at 36 x (128 + 100) (ops.profile_begin / profile_end: the unrolled path).

Each figure is (HIP-event time of `reps` steps) / reps after two warm-up steps; medians over the rounds, smallest and largest
round beside them.  The GEMM kernels come from the committed table (VT_AUTOTUNE=0 unless it is set already)."""
import argparse
import json
import os
import subprocess
import sys

os.environ.setdefault("VT_AUTOTUNE", "0")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = (("train 36 x (128 + 100)", 36, 128, 100), ("train 256 x (128 + 100)", 256, 128, 100), ("encoder 8 x 511 text", 8, 511, 0))
EMB_REGION = ("bert.embeddings.", "bert.img_embedding.", "bert.location_embeds.")
PATTERNS = {
    "all trainable": lambda n: False,
    "word table": lambda n: n == "bert.embeddings.word_embeddings.weight",
    "bottom six + embeddings + region": lambda n: n.startswith(EMB_REGION + tuple("bert.encoder.layer.%d." % l for l in range(6))),
    "heads only": lambda n: n.startswith("bert.") and not n.startswith("bert.pooler."),
}


def timed(fn, reps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps   # ms per step


def build_case(dev, B, T, R):
    """-> (step callable, the module whose named_parameters carry the patterns' names, name prefix)."""
    import torch

    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import BertImgModelwithLocationEmbeds, PreTrainOscar
    from visitron_amd.synth import make_batch

    cfg = BertConfig(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    torch.manual_seed(0)
    if R > 0:
        from visitron_amd.training import PretrainEngine

        model = PreTrainOscar(cfg).to(dev).train()
        eng = PretrainEngine(model, lr=5e-5, weight_decay=0.05, eps=1e-8, schedule="linear", warmup_steps=0, t_total=20000)
        batch = make_batch(cfg, B, T, R, seed=1234, device=dev, with_labels=True)
        return (lambda: eng.train_step(batch)), model, ""
    from visitron_amd.rollout import OscarEncoder

    trunk = BertImgModelwithLocationEmbeds(cfg)
    enc = OscarEncoder(None, trunk, 512, 512, 0.0).to(dev).train()
    g = torch.Generator().manual_seed(7)
    lens = sorted((int(x) for x in torch.randint(T // 2, T + 1, (B,), generator=g)), reverse=True)
    lens[0] = T
    ids = torch.randint(1000, cfg.vocab_size, (B, T), generator=g)
    pad = torch.zeros(B, T, dtype=torch.bool)
    for i, n in enumerate(lens):
        pad[i, n:] = True
        ids[i, n:] = 0
    ids, pad = ids.to(dev), pad.to(dev)

    def step():
        enc.zero_grad(set_to_none=True)
        ctx, h_t, c_t = enc(ids, lens, pad)
        (ctx.float().square().mean() + h_t.sum() + c_t.sum()).backward()

    return step, trunk, "bert."


def set_pattern(module, prefix, frozen):
    for n, p in module.named_parameters():
        p.requires_grad = not frozen(prefix + n)


def worker(a):
    """One child: --tree's package, the cases, --mode build (all-trainable only) or patterns; one JSON line per figure."""
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    if not torch.cuda.is_available():
        sys.exit("partial_training_bench.py measures on the GPU: no HIP device here")
    from visitron_amd import ops

    dev = torch.device("cuda:0")
    for name, B, T, R in CASES:
        reps = max(2, a.reps // 2) if B >= 128 else a.reps
        step, module, prefix = build_case(dev, B, T, R)
        pats = ["all trainable"] if a.mode == "build" else [p for p in PATTERNS if not (R == 0 and p == "heads only")]
        for rnd in range(a.rounds if a.mode == "patterns" else 1):
            for pat in pats:
                set_pattern(module, prefix, PATTERNS[pat])
                step()
                step()
                torch.cuda.synchronize()
                print("FIGURE " + json.dumps(dict(case=name, pattern=pat, ms=timed(step, reps))), flush=True)
        if a.mode == "patterns" and R > 0 and B < 128:
            for pat in pats:
                set_pattern(module, prefix, PATTERNS[pat])
                step()
                ops.profile_begin()
                step()
                census = {k: v["n"] for k, v in sorted(ops.profile_end().items())}
                print("CENSUS " + json.dumps(dict(case=name, pattern=pat, launches=census)), flush=True)
        del step, module
        torch.cuda.empty_cache()


def child(tree, mode, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--mode", mode, "--rounds", str(a.rounds),
           "--reps", str(a.reps)]
    env = dict(os.environ, PYTHONPATH=os.path.abspath(tree))
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("the child on %s (%s) failed:\n%s\n%s" % (tree, mode, r.stdout[-2000:], r.stderr[-4000:]))
    figs = [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("FIGURE ")]
    cens = [json.loads(ln[7:]) for ln in r.stdout.splitlines() if ln.startswith("CENSUS ")]
    return figs, cens


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", default=os.path.join(HERE, "ab_old"), help="a built tree of the commit to compare with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="patterns", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    out = ["# tools/partial_training_bench.py --rounds %d --reps %d   (VT_AUTOTUNE=%s)" % (a.rounds, a.reps, os.environ["VT_AUTOTUNE"])]

    def say(line):
        out.append(line)
        print(line, flush=True)

    # ---- all-trainable: this build against the other one, children alternated
    if os.path.isdir(os.path.join(a.old, "visitron_amd", "lib")):
        times = {}
        for rnd in range(a.rounds):
            pair = (("old", a.old), ("new", HERE))
            for label, tree in (pair if rnd % 2 == 0 else pair[::-1]):   # (who goes first changes from round to round)
                for f in child(tree, "build", a)[0]:
                    times.setdefault((f["case"], label), []).append(f["ms"])
        say("all-trainable step, this build (new) against %s (old), %d alternated processes each [ms per step]" % (
            os.path.relpath(a.old, HERE), a.rounds))
        for name, _, _, _ in CASES:
            (mo, lo_o, hi_o), (mn, lo_n, hi_n) = stats(times[(name, "old")]), stats(times[(name, "new")])
            say("    %-26s old median %8.3f (%8.3f .. %8.3f)   new median %8.3f (%8.3f .. %8.3f)   new/old %.4f   %s" % (
                name, mo, lo_o, hi_o, mn, lo_n, hi_n, mn / mo,
                "inside old's spread" if lo_o <= mn <= hi_o else ("below old's spread" if mn < lo_o else "ABOVE old's spread")))
    else:
        say("all-trainable against another build: not measured (%s holds no built tree)" % a.old)
    # ---- frozen patterns against this build's all-trainable step, alternated in one process
    figs, cens = child(HERE, "patterns", a)
    say("frozen patterns, this build, %d rounds alternated in one process [ms per step]" % a.rounds)
    for name, _, _, _ in CASES:
        base = stats([f["ms"] for f in figs if f["case"] == name and f["pattern"] == "all trainable"])
        for pat in PATTERNS:
            v = [f["ms"] for f in figs if f["case"] == name and f["pattern"] == pat]
            if v:
                med, lo, hi = stats(v)
                say("    %-26s %-34s median %8.3f (%8.3f .. %8.3f)   x %.4f of all trainable   %s" % (
                    name, pat, med, lo, hi, med / base[0], "" if pat == "all trainable" else ("faster" if hi < base[1] else "NOT clearly faster")))
    say("launch census of one step (unrolled path: the C loop issues the same launches from one call)")
    for c in cens:
        say("    %-26s %-34s %s" % (c["case"], c["pattern"], "  ".join("%s %d" % kv for kv in c["launches"].items())))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
