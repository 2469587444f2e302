"""Rectangular attention (csrc/attention_rect.hip: Sq queries over Sk = Sh + Sq keys): the case table, the backward comparison
and a CPU model of the kernels' data movement with its mutants.

The fp64 reference, the rounding models and the forward bounds are those of tests/helpers_attention.py, which take
q [B, nh, Sq, 64] against k, v [B, nh, Sk, 64] as they are.  Only the backward comparison is restated (backward_ratios there
applies one row selection to dq and to dk / dv), with the SAME yardstick and no new constant: per tensor and (batch, head), with
e_m the error of attention_bwd_ref64(round_model=True) and F the fp32 floor of BackwardTerms,
    ||e||_2 <= 2 ||e_m||_2 + ||F||_2     and     max|e| <= 3 max|e_m| + max|F|,
under either of DS_FORMS.

Packed layout (include/visitron_hip.h, vt_attention_rect_fwd_bf16): qkv [B*Sk, 3 nh 64], sequence b owns rows b Sk .. b Sk + Sk - 1,
its Sh history rows first, its queries the last Sq rows; ctx / dctx [B*Sq, nh 64]; lse [B, nh, Sq]; dqkv [B*Sk, 3 nh 64] with the
dq columns of history rows exactly zero; keep words one per (batch, head, 32-query block, key), key pitch Sk rounded up to 32."""
import math

import torch

import helpers_attention as ha

F64 = ha.F64
BF16 = torch.bfloat16

# (B, nh, Sh, Sq): the smallest shapes at which each mechanism can go wrong
SHAPES = ((2, 2, 0, 16),      # the square problem
          (2, 2, 1, 1), (2, 3, 7, 1), (2, 2, 64, 1), (2, 2, 37, 5),
          (1, 2, 255, 2),     # straddles 256 keys
          (2, 2, 250, 17),    # partial query tile and partial key tile
          (1, 2, 300, 33),    # second keep-word group
          (1, 1, 511, 1),
          (1, 2, 539, 228),   # the shipped 767
          (1, 1, 768, 256), (1, 1, 1023, 1))
BIAS_FORMS = ("none", "0/1", "-10000", "-inf", "finfo.min", "causal")
MUTANTS = ("history_keys_left_out", "queries_from_first_rows", "bias_square_pitch", "dkv_history_not_written",
           "dq_leaks_into_history", "keep_pitch_sq", "last_query_dropped", "dq_block_crossing_256_not_added")


def inputs(B, nh, Sh, Sq, seed=None, std=1.0):
    """qkv [B*Sk, 3 nh 64], dctx [B*Sq, nh 64]: fp32 holding bf16-exact values."""
    Sk, H = Sh + Sq, nh * 64
    g = torch.Generator().manual_seed(7919 * Sk + Sq if seed is None else seed)
    qkv = (torch.randn((B * Sk, 3 * H), generator=g) * std).to(BF16).float()
    dctx = (torch.randn((B * Sq, H), generator=g) * 0.7).to(BF16).float()
    return qkv, dctx


def split_rect(qkv, B, Sq, Sk, nh, q_rows_from=None):
    """packed [B*Sk, 3 nh 64] -> q [B, nh, Sq, 64] (a sequence's LAST Sq rows), k, v [B, nh, Sk, 64], float64."""
    q, k, v = ha.split_qkv(qkv, B, Sk, nh)
    r0 = Sk - Sq if q_rows_from is None else q_rows_from
    return q[:, :, r0:r0 + Sq].contiguous(), k, v


def bias_form(form, B, Sh, Sq, seed=0):
    """(mask for the kernel or None, mask_additive, float64 bias [B, Sk] or [B, Sq, Sk]).  Every row keeps its last key; one
    history key (the second, where there is one) is always masked, as is a padded tail of the new positions in sequence 0."""
    Sk = Sh + Sq
    if form == "none":
        return None, False, torch.zeros(B, Sk, dtype=F64)
    g = torch.Generator().manual_seed(4000 + 31 * Sk + Sq + seed)
    raw = (torch.rand(B, Sk, generator=g) > 0.25).float()
    raw[:, -1] = 1
    if Sh > 1:
        raw[:, 1] = 0
    if Sq > 2:
        raw[0, Sh + Sq // 2:Sk - 1] = 0
    if form == "0/1":
        return raw, False, ((1.0 - raw) * -10000.0).to(F64)
    if form == "causal":   # per query: the history as `raw` says, new position i sees the new positions j <= i
        vis = raw[:, None, :].expand(B, Sq, Sk).clone()
        vis[:, :, Sh:] = torch.tril(torch.ones(Sq, Sq))[None]
        add = ((1.0 - vis) * -10000.0).contiguous()
        return add, True, add.to(F64)
    add = torch.stack([ha.form_bias(raw[b], form) for b in range(B)])
    return add, True, ha.canonical_bias(add)


def pack_keep_words(keep):
    """bool [B, nh, Sq, Sk] -> int32 [B nh nqb kpitch], the forward's layout."""
    B, nh, Sq, Sk = keep.shape
    nqb, kp = (Sq + 31) // 32, (Sk + 31) // 32 * 32
    full = torch.zeros(B, nh, nqb * 32, kp, dtype=torch.int64)
    full[:, :, :Sq, :Sk] = keep.to(torch.int64)
    w = (full.view(B, nh, nqb, 32, kp) << torch.arange(32).view(1, 1, 1, 32, 1)).sum(3)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).reshape(-1)


def unpack_keep_words(words, B, nh, Sq, Sk, kpitch=None):
    """int32 words -> bool [B, nh, Sq, Sk]; kpitch: the key pitch read with (default: Sk rounded up to 32)."""
    nqb = (Sq + 31) // 32
    kp = (Sk + 31) // 32 * 32 if kpitch is None else kpitch
    blk = torch.arange(B * nh * nqb).view(B, nh, nqb, 1, 1)
    idx = blk * kp + torch.arange(Sk).view(1, 1, 1, 1, Sk)
    w = words.to(torch.int64)[idx.expand(B, nh, nqb, 1, Sk)]
    bits = (w >> torch.arange(32).view(1, 1, 1, 32, 1)) & 1
    return bits.reshape(B, nh, nqb * 32, Sk)[:, :, :Sq].bool()


class Case(object):
    """One problem in the packed layout with its fp64 terms (built once, shared by every judgement of the case)."""

    def __init__(self, B, nh, Sh, Sq, form="none", keep=None, p_eff=0.0, head_scale=None, qkv=None, dctx=None, seed=None, std=1.0):
        self.B, self.nh, self.Sh, self.Sq, self.Sk, self.H = B, nh, Sh, Sq, Sh + Sq, nh * 64
        self.form = form
        a, b = inputs(B, nh, Sh, Sq, seed, std)
        self.qkv, self.dctx = (a if qkv is None else qkv), (b if dctx is None else dctx)
        self.mask, self.mask_additive, self.bias = bias_form(form, B, Sh, Sq)
        self.keep, self.p_eff, self.head_scale = keep, p_eff, head_scale
        self.q, self.k, self.v = split_rect(self.qkv, B, Sq, self.Sk, nh)
        self.d64 = ha.heads(self.dctx, B, Sq, nh)
        self._fterms = self._bterms = None

    def label(self):
        return "B%d nh%d Sh%d Sq%d %s%s" % (self.B, self.nh, self.Sh, self.Sq, self.form, " drop" if self.keep is not None else "")

    def fterms(self):
        if self._fterms is None:
            self._fterms = ha.ForwardTerms(self.q, self.k, self.v, self.bias, self.keep, self.p_eff, self.head_scale)
        return self._fterms

    def bterms(self, ctx_given):
        """The backward's terms, delta formed from `ctx_given` [B, nh, Sq, 64] (the context the backward under test was handed);
        built at the first call and kept."""
        if self._bterms is None:
            self._bterms = ha.BackwardTerms(self.q, self.k, self.v, self.bias, self.d64, ctx_given, self.keep, self.p_eff)
        return self._bterms


def backward_ratios(terms, got, ds_form="folded"):
    """{check: measured / bound} of dq [B, nh, Sq, 64], dk, dv [B, nh, Sk, 64]: helpers_attention.backward_ratios' yardstick
    (module docstring) with every row of every tensor compared."""
    out = {}
    for name, g, w, m, F in zip(("dq", "dk", "dv"), got, terms.want, terms.models[ds_form], terms.F):
        g = g.to(F64)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert bool(torch.isfinite(g).all()), "non-finite %s" % name
        ek, em = (g - w).flatten(2), (m - w).flatten(2)
        Ff = F.flatten(2)
        l2 = ek.norm(dim=-1) / (2.0 * em.norm(dim=-1) + Ff.norm(dim=-1))
        mx = ek.abs().amax(-1) / (3.0 * em.abs().amax(-1) + Ff.abs().amax(-1))
        zero = ek.abs().amax(-1) == 0
        out[name + " l2 err/bound"] = float(torch.where(zero, torch.zeros_like(l2), l2).max())
        out[name + " max err/bound"] = float(torch.where(zero, torch.zeros_like(mx), mx).max())
    return out


def unpack_grads(dqkv, B, Sq, Sk, nh):
    """packed dqkv [B*Sk, 3 nh 64] -> dq of the history rows [B, nh, Sh, 64], dq [B, nh, Sq, 64], dk, dv [B, nh, Sk, 64]."""
    H = nh * 64
    x = dqkv.detach().cpu().to(F64)
    dq, dk, dv = (ha.heads(x[:, i * H:(i + 1) * H], B, Sk, nh) for i in range(3))
    return dq[:, :, :Sk - Sq], dq[:, :, Sk - Sq:].contiguous(), dk, dv


def judge_forward(case, ctx, lse):
    """ctx [B*Sq, nh 64], lse [B, nh, Sq] -> {check: ratio}."""
    return ha.forward_ratios(case.fterms(), ha.heads(ctx, case.B, case.Sq, case.nh), None if lse is None else lse.detach().cpu())


def judge_backward(case, ctx_given, dqkv):
    """dqkv [B*Sk, 3 nh 64] (any float dtype), ctx_given [B*Sq, nh 64] -> {check: ratio}, under both DS_FORMS; the history rows' dq
    must be exactly zero (ratio inf otherwise)."""
    hist, dq, dk, dv = unpack_grads(dqkv, case.B, case.Sq, case.Sk, case.nh)
    terms = case.bterms(ha.heads(ctx_given, case.B, case.Sq, case.nh))
    out = {"dq of history rows == 0": 0.0 if bool((hist == 0).all()) else math.inf}
    for form in ha.DS_FORMS if case.keep is not None else ha.DS_FORMS[:1]:
        for key, val in backward_ratios(terms, (dq, dk, dv), form).items():
            out["%s (%s)" % (key, form)] = val
    return out


# ---- the CPU model of the kernels' data movement --------------------------------------------------------------------------
def packed_model(case, mutant=None):
    """What the kernels do, on the CPU: the minimal bf16 arithmetic of helpers_attention (forward_model,
    attention_bwd_ref64(round_model=True)) between the packed layouts of the module docstring.  Returns ctx [B*Sq, nh 64],
    lse [B, nh, Sq], dqkv [B*Sk, 3 nh 64] (float64; the backward takes no head scale and is None for a case that has one).
    mutant: one way of moving the data wrongly (MUTANTS)."""
    B, nh, Sh, Sq, Sk = case.B, case.nh, case.Sh, case.Sq, case.Sk
    q, k, v = split_rect(case.qkv, B, Sq, Sk, nh, q_rows_from=0 if mutant == "queries_from_first_rows" else None)
    bias = case.bias
    if mutant == "bias_square_pitch" and bias.dim() == 3:     # element (q, key) read at q * Sq + key of the sequence's block
        idx = torch.arange(Sq)[:, None] * Sq + torch.arange(Sk)[None, :]
        bias = bias.reshape(B, -1)[:, idx]
    if mutant == "history_keys_left_out" and Sh > 0:
        gone = torch.zeros(Sk, dtype=F64)
        gone[:Sh] = -math.inf
        bias = bias + gone
    ctx, lse, _ = ha.forward_model(q, k, v, bias, case.keep, case.p_eff, case.head_scale)
    if mutant == "last_query_dropped":
        ctx = ctx.clone()
        ctx[:, :, -1] = 0
    ctx_rows = ctx.permute(0, 2, 1, 3).reshape(B * Sq, nh * 64)
    if case.head_scale is not None:
        return ctx_rows, lse, None
    keep = case.keep
    if mutant == "keep_pitch_sq" and keep is not None:
        keep = unpack_keep_words(pack_keep_words(keep), B, nh, Sq, Sk, kpitch=(Sq + 31) // 32 * 32)
    bmut = {"last_query_dropped": "last_query_ignored", "dq_block_crossing_256_not_added": "dq_second_key_block_not_added"}.get(mutant)
    dq, dk, dv = ha.attention_bwd_ref64(q, k, v, bias, case.d64, ctx, keep, case.p_eff, round_model=True, mutant=bmut)
    out = torch.zeros(B, Sk, 3, nh, 64, dtype=F64)
    out[:, Sh:, 0] = dq.permute(0, 2, 1, 3)
    out[:, :, 1] = dk.permute(0, 2, 1, 3)
    out[:, :, 2] = dv.permute(0, 2, 1, 3)
    if mutant == "dkv_history_not_written":
        out[:, :Sh, 1:] = 0
    if mutant == "dq_leaks_into_history":
        n = min(Sh, Sq)
        out[:, :n, 0] = dq.permute(0, 2, 1, 3)[:, :n]
    return ctx_rows, lse, out.reshape(B * Sk, 3 * nh * 64)


def random_keep(B, nh, Sq, Sk, p, seed=5):
    g = torch.Generator().manual_seed(seed + Sk)
    return torch.rand(B, nh, Sq, Sk, generator=g) >= p
