"""Which library calls the training engine issues, and what it computes, as comparable hashes -- for checking that a change
to the Python that drives the step (visitron_amd/training.py, training_f32.py) moved neither.

    python tools/engine_trace.py [--package-root DIR] [--mode deterministic|default] [--only CASE ...] [--log-dir DIR]

--package-root DIR is put in front of sys.path, so another tree's `visitron_amd` (say, the parent commit's Python files)
can run against the same built library (VT_HIP_LIB).  Only names both trees have are used.  What _lib.load() returns is
replaced by a recording proxy: per library call the function name, every scalar argument and, for every pointer argument,
only whether it is null (no addresses).  Per case one line:

    <case> calls=<n> log=<sha256 of the call log> out=<sha256 over the returned tuples, flat.g / p / m / v / mirror, d_history>

deterministic (default): under ops.set_deterministic(True) the GEMM choices come from the committed table (no timing
launches) and sums have a fixed order: two trees that do the same work print the same lines.  A differing `out` with an
equal `log` means a tensor was released while a launch still read it."""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--package-root", default=ROOT)
ap.add_argument("--mode", choices=("deterministic", "default"), default="deterministic")
ap.add_argument("--only", nargs="*", default=None)
ap.add_argument("--log-dir", default=None, help="also write each case's call log to DIR/<case>.log (to diff two runs)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

import torch  # noqa: E402
from visitron_amd import _lib, ops  # noqa: E402
from visitron_amd.config import mini_config  # noqa: E402
from visitron_amd.modeling import PreTrainOscar  # noqa: E402
from visitron_amd.synth import deterministic_state_dict, make_batch  # noqa: E402
from visitron_amd.training import PretrainEngine  # noqa: E402

DEV = "cuda:0"
B, T, R = 3, 20, 17           # the shapes of tests/test_gpu_train.py: 111 token rows, some of them padding


class _Recorder(object):
    """Stands in for the loaded library: forwards every call, logs name, scalars and the nullness of pointers."""

    def __init__(self, lib):
        self._lib_, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib_, name)
        types = fn.argtypes or ()

        def call(*a):
            items = []
            for i, v in enumerate(a):
                t = types[i] if i < len(types) else None
                scalar = t is not None and issubclass(t, ctypes._SimpleCData) and t not in (ctypes.c_void_p, ctypes.c_char_p)
                if scalar:
                    items.append(repr(v.value if isinstance(v, ctypes._SimpleCData) else v))
                else:
                    null = v is None or v == 0 or (isinstance(v, ctypes.c_void_p) and not v.value)
                    items.append("null" if null else "ptr")
            self.log.append("%s(%s)" % (name, ", ".join(items)))
            return fn(*a)

        return call


REC = _Recorder(_lib.load())
_lib.load = lambda: REC


def _bytes(x):
    if torch.is_tensor(x):
        x = x.detach()
        return (x.view(torch.int16) if x.dtype == torch.bfloat16 else x).contiguous().cpu().numpy().tobytes()
    if isinstance(x, (list, tuple)):
        return b"[" + b",".join(_bytes(v) for v in x) + b"]"
    return repr(x).encode()


def _engine(cfg=None, untied=False, dropout=True, **kw):
    cfg = cfg or mini_config()
    if dropout:
        cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    torch.manual_seed(0)
    model = PreTrainOscar(cfg)
    if untied:
        model.resize_embeddings({"word_embeddings": cfg.vocab_size + 3})
    model.load_state_dict(deterministic_state_dict(model, seed=3))
    model = model.to(DEV).train()
    eng = PretrainEngine(model, **kw)
    eng.compact_min_rows = 0      # the small batches take the real-rows-only path too
    return cfg, model, eng


def _batch(cfg, seed=11, b=B, t=T, r=R, **kw):
    return {k: v.to(DEV) for k, v in make_batch(cfg, batch=b, text_len=t, region_len=r, seed=seed, **kw).items()}


def _trunk_batch(batch):
    return {k: v for k, v in batch.items() if k in ("input_ids", "attention_mask", "img_feats", "img_location_embeddings")}


def _slabs(eng):
    f = eng.flat
    return [f.g, f.p, f.m, f.v, f.mirror]


# ---- the cases: each returns what goes into the output hash --------------------------------------------------------------
def _steps(compact):
    cfg, _, eng = _engine()
    eng.compact_rows = compact
    return [eng.train_step(_batch(cfg, seed=11 + i)) for i in range(3)] + _slabs(eng)


def case_train_step_compact():
    return _steps(True)


def case_train_step_padded():
    return _steps(False)


def case_train_step_long():   # 260 keys: the attention backward runs over two key blocks, dQ through the fp32 workspace
    cfg, _, eng = _engine()
    return [eng.train_step(_batch(cfg, b=2, t=60, r=200)) for _ in range(2)] + _slabs(eng)


def case_accumulate_then_step():
    cfg, _, eng = _engine()
    out = [eng.forward_backward(_batch(cfg, seed=11)), eng.forward_backward(_batch(cfg, seed=12), accumulate=True)]
    eng.optimizer_step()
    return out + _slabs(eng)


def case_head_mask():
    cfg, _, eng = _engine()
    hm = torch.tensor([[1.0, 0.0], [0.5, 1.0]], device=DEV)
    return [eng.forward_backward(_batch(cfg), head_mask=hm)] + _slabs(eng)


def case_mask_3d():
    cfg, _, eng = _engine()
    batch = _batch(cfg)
    m = batch["attention_mask"].float()
    batch["attention_mask"] = m[:, None, :].expand(B, T + R, T + R).contiguous()
    return [eng.forward_backward(batch)] + _slabs(eng)


def _unsupervised(change):
    cfg, _, eng = _engine()
    out = [eng.forward_backward(_batch(cfg, seed=11))]       # gradients everywhere first: the second pass must clear its share
    batch = _batch(cfg, seed=12)
    change(batch)
    return out + [eng.forward_backward(batch)] + _slabs(eng)


def case_no_mlm_row():
    return _unsupervised(lambda b: b["labels"].fill_(-1))


def case_no_token_row():
    return _unsupervised(lambda b: b["token_labels"].fill_(-1))


def case_no_next_action():
    return _unsupervised(lambda b: b.pop("next_action"))


def case_img_layernorm():
    cfg = mini_config()
    cfg.use_img_layernorm, cfg.img_layer_norm_eps = 1, 1e-12
    cfg, _, eng = _engine(cfg)
    return [eng.train_step(_batch(cfg, seed=11 + i)) for i in range(2)] + _slabs(eng)


def case_untied_decoder():
    cfg, _, eng = _engine(untied=True)
    out = [eng.train_step(_batch(cfg, seed=11 + i)) for i in range(2)]
    batch = _batch(cfg, seed=13)
    batch["labels"].fill_(-1)
    return out + [eng.forward_backward(batch)] + _slabs(eng)


def case_forced_comm_chunks():
    cfg, _, eng = _engine()
    return [eng.train_step(_batch(cfg, seed=11 + i), _force_comm=lambda rng: None, layers_per_chunk=1) for i in range(2)] + _slabs(eng)


def case_overlap_adamw():
    cfg, _, eng = _engine()
    eng.overlap_adamw = True
    return [eng.train_step(_batch(cfg, seed=11 + i)) for i in range(3)] + _slabs(eng)


def case_overlap_wgrad():
    cfg, _, eng = _engine()
    eng.overlap_wgrad = True
    out = [eng.train_step(_batch(cfg, seed=11 + i)) for i in range(2)]
    eng.compact_rows = False
    return out + [eng.train_step(_batch(cfg, seed=13 + i)) for i in range(2)] + _slabs(eng)


def case_fp32():
    cfg, _, eng = _engine(precision="fp32")
    batch = _batch(cfg)
    out = [eng.forward_backward(batch)]
    seq, pooled, st = eng.trunk_forward(_trunk_batch(batch))
    g = torch.Generator(device="cpu").manual_seed(5)
    d_seq, d_pooled = torch.randn(seq.shape, generator=g).to(DEV), torch.randn(pooled.shape, generator=g).to(DEV)
    eng.trunk_backward(st, d_seq, d_pooled)
    return out + [seq, pooled] + _slabs(eng)


def case_trunk_variants():
    cfg, _, eng = _engine()
    batch, out = _trunk_batch(_batch(cfg)), []
    g = torch.Generator(device="cpu").manual_seed(7)
    rnd = lambda like: torch.randn(like.shape, generator=g).to(DEV)
    seq, pooled, st = eng.trunk_forward(batch, unmasked_only=True)
    eng.trunk_backward(st, rnd(seq) * (seq != 0), rnd(pooled))
    out += [seq, pooled, eng.flat.g.clone()]
    seq, pooled, st, hidden = eng.trunk_forward(batch, want_hidden=True)
    eng.trunk_backward(st, rnd(seq), None, d_hidden=[rnd(h) for h in hidden])
    out += [seq, pooled, hidden, eng.flat.g.clone()]
    seq, pooled, st, _, attn = eng.trunk_forward(batch, want_attn=True)
    eng.trunk_backward(st, rnd(seq), rnd(pooled), accumulate=True)
    out += [seq, pooled, attn, eng.flat.g.clone()]
    # history states (text only): layer 1's requires grad
    Sh = 5
    text = dict(input_ids=batch["input_ids"], attention_mask=torch.cat(
        [torch.ones((B, Sh), device=DEV, dtype=batch["attention_mask"].dtype), batch["attention_mask"][:, :T]], 1))
    hist = [rnd(torch.empty(B, Sh, cfg.hidden_size)) * 0.3 for _ in range(cfg.num_hidden_layers)]
    hist[1].requires_grad_(True)
    seq, pooled, st, _, attn = eng.trunk_forward(text, history=hist, want_attn=True)
    eng.trunk_backward(st, rnd(seq), rnd(pooled))
    return out + [seq, pooled, attn, st.d_history] + _slabs(eng)


def case_autograd_entries():
    cfg, model, _ = _engine()
    batch, out = _batch(cfg), []
    grads = lambda mod: [None if p.grad is None else p.grad.clone() for p in mod.parameters()]
    res = model(**batch)                                   # training.autograd_forward
    res[0].backward()
    out += [res, grads(model)]
    model.zero_grad()
    model.eval()
    res = model(**batch)                                   # training.lazy_autograd_loss
    res[0].backward()
    out += [res, grads(model), _slabs(model._vt_engine)]
    cfg, model, _ = _engine()
    trunk, tb = model.bert, _trunk_batch(batch)
    seq, pooled = trunk(**tb)[:2]                          # training.autograd_trunk_forward
    (seq.sum() + 2.0 * pooled.sum()).backward()
    out += [seq, pooled, grads(trunk)]
    trunk.zero_grad()
    trunk.eval()
    seq, pooled = trunk(**tb)[:2]                          # training.lazy_autograd_trunk
    (seq * seq).sum().backward()
    return out + [seq, pooled, grads(trunk), _slabs(trunk._vt_engine)]


def main():
    ops.set_deterministic(args.mode == "deterministic")
    cases = [(n[5:], f) for n, f in globals().items() if n.startswith("case_")]
    for name, fn in cases:
        if args.only and name not in args.only:
            continue
        del REC.log[:]
        out = fn()
        torch.cuda.synchronize()
        if args.log_dir:
            os.makedirs(args.log_dir, exist_ok=True)
            with open(os.path.join(args.log_dir, name + ".log"), "w") as fh:
                fh.write("\n".join(REC.log) + "\n")
        print("%-22s calls=%-5d log=%s out=%s" % (name, len(REC.log), hashlib.sha256("\n".join(REC.log).encode()).hexdigest()[:32],
                                                   hashlib.sha256(_bytes(out)).hexdigest()[:32]), flush=True)


if __name__ == "__main__":
    main()
