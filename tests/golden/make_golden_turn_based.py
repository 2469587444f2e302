"""Writes tests/golden/ref_turn_based.npz from the reference's turn-based agent models (build container only).

The reference's source runs where it lies: tasks/turn_based/agent_models.py and tasks/viewpoint_select/agent_models.py are
imported from /root/reference by path (asserted below), nothing of their text is copied.  What is recorded:

  sd.<name>            the AttnDecoderLSTM state dict (hidden 128, embedding 8, feature 70, 8 input / 6 output actions); the
                       values are multiples of 1/512 in [-1/8, 1/8], stored as float16 (exact)
  attn.*               SoftDotAttention(128) on h [5, 128], ctx [5, 9, 128] without and with a uint8 mask
  step.*               two chained eval steps (h_1, c_1 fed back as the rollout loop does, agent.py:311-313)
  train.*, grad.<name> a two-step teacher-forced loss under train() at dropout 0: CrossEntropyLoss(ignore_index=-100) of the
                       logits with the `forward` entry of some rows set to -inf (agent.py:316-323), rows with target -100
                       included; gradients of every parameter and of ctx, h_0, c_0.  A gradient g is stored as float16 of
                       g / gscale.<name> with gscale a power of two >= max|g| (relative rounding 2^-11, far inside the 2e-2
                       relative-L2 tolerance it is read at)
  oscar_encoder_same   1 when the two tasks' OscarEncoder classes give bit-identical outputs for one state dict and input
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
HS, E, F, A_IN, A_OUT, B, L = 128, 8, 70, 8, 6, 5, 9
FORWARD, IGNORE = 1, -100


def _load(name, rel):
    path = os.path.join(REF, rel)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.realpath(mod.__file__).startswith(REF + os.sep), mod.__file__
    return mod


def _grid(gen, *shape):
    return torch.randint(-64, 65, shape, generator=gen).float() / 512.0


class _Bert(torch.nn.Module):
    """Stand-in trunk for the OscarEncoder comparison: [B, S] ids -> ([B, S, 768],)."""

    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(50, 768)

    def forward(self, inputs, token_type_ids=None, attention_mask=None, position_ids=None):
        return (self.emb(inputs) * attention_mask.bool()[:, :, None].float(),)


class _Args(object):
    device = "cpu"


def _encoder_same(tb, vp, gen):
    torch.manual_seed(5)
    a = tb.OscarEncoder(_Args(), _Bert(), 128, 96, 0.5).eval()
    b = vp.OscarEncoder(_Args(), _Bert(), 128, 96, 0.5).eval()
    if list(a.state_dict()) != list(b.state_dict()):
        return 0
    b.load_state_dict(a.state_dict())
    ids = torch.randint(1, 50, (3, 7), generator=gen)
    lengths = torch.tensor([7, 5, 2])
    mask = (torch.arange(7)[None, :] >= lengths[:, None])
    with torch.no_grad():
        oa, ob = a(ids, lengths, mask), b(ids, lengths, mask)
    return int(all(torch.equal(x, y) for x, y in zip(oa, ob)))


def main():
    tb = _load("ref_turn_based_agent_models", "tasks/turn_based/agent_models.py")
    vp = _load("ref_viewpoint_agent_models", "tasks/viewpoint_select/agent_models.py")
    gen = torch.Generator().manual_seed(1234)
    out = {}

    dec = tb.AttnDecoderLSTM(A_IN, A_OUT, E, HS, 0.0, feature_size=F)
    sd = {k: _grid(gen, *v.shape) for k, v in dec.state_dict().items()}
    dec.load_state_dict(sd)
    for k, v in sd.items():
        assert torch.equal(v.half().float(), v)
        out["sd." + k] = v.half().numpy()

    ctx = torch.randn(B, L, HS, generator=gen) * 0.5
    lens = [9, 7, 7, 4, 1]
    mask = (torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]).to(torch.uint8)
    h0, c0 = torch.randn(B, HS, generator=gen) * 0.5, torch.randn(B, HS, generator=gen) * 0.5
    out.update({"ctx": ctx.numpy(), "mask": mask.numpy(), "h0": h0.numpy(), "c0": c0.numpy()})

    att = dec.attention_layer.eval()
    with torch.no_grad():
        for tag, m in (("nomask", None), ("mask", mask)):
            ht, al = att(h0, ctx, m)
            out["attn.%s.h_tilde" % tag], out["attn.%s.attn" % tag] = ht.numpy(), al.numpy()

    feats = [torch.randn(B, F, generator=gen).abs() for _ in range(2)]   # image features are non-negative (post-ReLU pool)
    acts = [torch.randint(0, A_IN, (B, 1), generator=gen) for _ in range(2)]
    for i in range(2):
        out["feature%d" % i], out["action%d" % i] = feats[i].numpy(), acts[i].numpy()
    dec.eval()
    with torch.no_grad():
        h, c = h0, c0
        for i in range(2):
            h, c, alpha, logit = dec(acts[i], feats[i], h, c, ctx, mask)
            for n, t in (("h_1", h), ("c_1", c), ("alpha", alpha), ("logit", logit)):
                out["step.%d.%s" % (i, n)] = t.numpy()

    # two teacher-forced training steps at dropout 0
    dec.train()
    targets = [torch.tensor([2, FORWARD, IGNORE, 4, 0]), torch.tensor([IGNORE, 3, 5, FORWARD, 2])]
    blocked = [torch.zeros(B, A_OUT, dtype=torch.uint8) for _ in range(2)]
    blocked[0][0, FORWARD] = 1
    blocked[0][2, FORWARD] = 1       # an ignored row may be blocked too
    blocked[1][2, FORWARD] = 1
    blocked[1][4, FORWARD] = 1
    ctx_g, h_g, c_g = ctx.clone().requires_grad_(), h0.clone().requires_grad_(), c0.clone().requires_grad_()
    crit = torch.nn.CrossEntropyLoss(ignore_index=IGNORE)
    a_t = acts[0]
    loss = torch.zeros(())
    h, c = h_g, c_g
    for i in range(2):
        h, c, alpha, logit = dec(a_t.view(-1, 1), feats[i], h, c, ctx_g, mask)
        for r in range(B):
            if blocked[i][r, FORWARD]:
                logit[r, FORWARD] = -float("inf")
        step_loss = crit(logit, targets[i])
        out["train.loss%d" % i] = step_loss.detach().numpy()
        loss = loss + step_loss
        # teacher forcing: the next input is the target; an ignored row (an ended episode) keeps feeding action 0
        a_t = torch.where(targets[i] == IGNORE, torch.zeros_like(targets[i]), targets[i])
        out["train.target%d" % i], out["train.blocked%d" % i] = targets[i].numpy(), blocked[i].numpy()
    loss.backward()
    out["train.loss"] = loss.detach().numpy()
    grads = {k: p.grad for k, p in dec.named_parameters()}
    grads.update({"ctx": ctx_g.grad, "h0": h_g.grad, "c0": c_g.grad})
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
        s = 2.0 ** np.ceil(np.log2(float(g.abs().max())))
        out["grad." + k], out["gscale." + k] = (g / s).half().numpy(), np.float32(s)

    out["oscar_encoder_same"] = np.int64(_encoder_same(tb, vp, gen))
    assert out["oscar_encoder_same"] == 1
    path = os.path.join(HERE, "ref_turn_based.npz")
    np.savez_compressed(path, **out)
    print("ref_turn_based.npz written: %d bytes, %d arrays" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    sys.exit(main())
