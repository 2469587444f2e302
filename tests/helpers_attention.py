"""fp64 reference, CPU rounding models and derived error bounds for the fused attention kernels (head size 64).

Everything here is plain torch on the CPU in float64.  tests/test_host_attention_reference.py proves, without a GPU, that
the bounds accept the minimal bf16 implementation and reject a table of subtly wrong ones; tests/test_gpu_attention_conformance.py
holds the HIP kernels to the same bounds.  No bound below was chosen by looking at a kernel's output.

Tensors: q, k, v [B, nh, S, 64] float64 (from bf16-rounded inputs), bias [B, S] (per key) or [B, S, S] (per query, key) float64,
-inf legal where a row keeps one finite key; keep [B, nh, S, S] 0/1 or None; lens [B] = rows of each sequence (a compacted batch is
compared in the padded geometry with bias = -inf for keys past a sequence's length and only its own query rows looked at).

FORWARD BOUND (forward_bound), per element, u = 2^-8 (bf16 unit round-off, round to nearest), A = sum_k p~_k |v_k| with p~ the
probability after dropout and |head scale|:

    |ctx_kernel - ctx_ref| <= u A + u |ctx_ref| + 2^-12 f A,      f = max(1, max_k |s_k| / 128, D / 16)

  u A       each un-normalised probability is rounded to bf16 once before P.V while the normaliser sums the unrounded values:
            sum_k |delta p_k| |v_k| <= u sum_k p_k |v_k|.
  u |ctx|   the stored output is rounded once.
  2^-12 A   everything done in fp32: the exponent's argument (|acc scale2| <= 2^7 => absolute 2^-17 on the argument, relative
            2^-17 on p), v_exp_f32 (1 ulp), the fp32 accumulation of up to 1 025 terms (<= n 2^-24 = 2^-14), the normaliser's
            own sum (the same), 1 / l and the final multiplies (a few 2^-24): about 2^-14, with a factor four to spare.
  f         the 2^-12 assumed |s| <= 128 and a score exact to fp32.  A 64-term fp32 dot product errs by at most
            64 2^-24 D with D = max_k sum_i |q_i k_i| / 8 (the absolute-value twin of the score), and a score of magnitude
            |s| is resolved to |s| 2^-24 by fp32 (the reference's own arithmetic): both enter p relatively, hence the scaling.

LSE BOUND  |lse_kernel - lse_ref| <= 2^-23 (4 (1 + max_k |s_k|) + 32 D): four fp32 roundings at the magnitude of the largest
score plus the dot product's 64 2^-24 D.

PROBABILITIES  relative <= 2^-23 (8 + 2 |s - lse| + 4 (1 + max|s|) + 64 D) where p_ref >= 2^-100, absolute <= 2^-100 below
(__expf's result and argument roundings, the lse bound carried through the exponent, the kernel's own dot product).  Rows sum
to the head scale within |head scale| (S 2^-23 f + the lse bound of the row): S 2^-23 is the sum of S independently rounded
probabilities; an error e of the saved lse -- allowed up to the lse bound -- moves EVERY probability of the row by the same
factor exp(-e), so it arrives in the row sum undiminished, and f is the forward bound's factor for scores outside |s| <= 128
(a sum bound below what the element bound and the lse bound permit would contradict them).

BACKWARD (backward_ratios)  The yardstick is the error e_m of the MINIMAL BF16 IMPLEMENTATION (attention_bwd_ref64 with
round_model=True: fp64 except ctx as handed in, P and dS rounded to bf16 once before their second product, dq / dk / dv rounded
once; under dropout dS is rounded either with or without the factor 1 / (1 - p): DS_FORMS below).
Per tensor and (batch, head):   ||e_k||_2 <= 2 ||e_m||_2 + ||F||_2   and   max|e_k| <= 3 max|e_m| + max|F|.
Any MFMA implementation has at least the model's roundings; a legitimate one may round one operand once more per product (a
transposed dS image, a pre-scaled Q): one more term of the same size in quadrature, sqrt 2, rounded up to 2; the maximum of a few
hundred thousand roundings fluctuates more than their norm: 3.  F is the element-wise fp32 floor: the gradient's product with every
factor replaced by its absolute value and (dP - delta) by (|dP| + |delta|), times 2^-18, plus a relative 2^-21 max(1, |s|) on every
P (fp32's resolution of the score).  Errors are compared as norms and never divided by ||want||.

SIGNED BIAS (signed_stat)  mean(err sign(ref) / bound) over N >= 1e5 elements of random data must lie within 6 / sqrt(N) of zero:
roundings to nearest are zero-mean and |err / bound| <= 1, so the mean has a standard deviation below 1 / sqrt(N).  A truncating
convert shrinks every output towards zero: its error follows the sign of the output and is invisible to any max-abs bound.
"""
import math

import torch

U = 2.0 ** -8
F64 = torch.float64


def bf16r(x):
    """Round to nearest even to bf16, back in float64."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def bf16_trunc(x):
    """Truncating bf16 convert (the mutant), back in float64."""
    return (x.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32).to(F64)


def split_qkv(qkv, B, S, nh):
    """packed [B*S, 3*nh*64] -> q, k, v [B, nh, S, 64] float64 of the bf16-rounded values."""
    t = qkv.detach().cpu().to(torch.bfloat16).to(F64).view(B, S, 3, nh, 64).permute(2, 0, 3, 1, 4)
    return t[0].contiguous(), t[1].contiguous(), t[2].contiguous()


def heads(x, B, S, nh):
    """[B*S, nh*64] -> [B, nh, S, 64] float64."""
    return x.detach().cpu().to(F64).view(B, S, nh, 64).permute(0, 2, 1, 3).contiguous()


def canonical_bias(bias):
    """float64 bias; anything at or below -1e30 (finfo(float32).min: the kernel's bias / scale overflows it) is -inf."""
    bias = bias.detach().cpu().to(F64)
    return torch.where(bias <= -1e30, torch.full_like(bias, -math.inf), bias)


def length_bias(lens, S):
    """[B, S]: 0 for a sequence's own keys, -inf past its length (a compacted batch in the padded geometry)."""
    keep = torch.arange(S)[None, :] < torch.as_tensor(lens)[:, None]
    return torch.where(keep, torch.zeros((), dtype=F64), torch.full((), -math.inf, dtype=F64))


def _bias4(bias):
    return bias[:, None, None, :] if bias.dim() == 2 else bias[:, None, :, :]


def scores64(q, k, bias):
    return q @ k.transpose(-1, -2) / 8.0 + _bias4(bias)


def _keep_scale(keep, p_eff):
    return None if keep is None else keep.to(F64) / (1.0 - p_eff)


def attention_ref64(q, k, v, bias, keep=None, p_eff=0.0, head_scale=None):
    """oscar/modeling_bert.py:52-68 in float64: s = q k^T / 8 + bias, softmax, * keep / (1 - p_eff), * head_scale, . v.
    Returns ctx [B, nh, S, 64], lse [B, nh, S], probs [B, nh, S, S] (the softmax itself, before dropout and head scale)."""
    s = scores64(q, k, bias)
    probs = torch.softmax(s, dim=-1)
    lse = torch.logsumexp(s, dim=-1)
    pt = probs
    km = _keep_scale(keep, p_eff)
    if km is not None:
        pt = pt * km
    if head_scale is not None:
        pt = pt * head_scale.to(F64).view(1, -1, 1, 1)
    return pt @ v, lse, probs


def attention_bwd_ref64(q, k, v, bias, dctx, ctx_given=None, keep=None, p_eff=0.0, round_model=False, mutant=None, lens=None,
                        pre=None, ds_prescale=1.0):
    """Closed form of the gradient of attention_ref64 (no head scale: the backward kernels take none):
    dV = P~^T dO, dP = dO V^T, dS = P o (keep / (1 - p) o dP - delta), dQ = dS K / 8, dK = dS^T Q / 8, with
    delta = rowsum(P~ o dP) = rowsum(dO o ctx); ctx_given: form delta from this ctx (the kernels' input) instead.
    round_model: the minimal bf16 implementation (module docstring).  mutant: a wrong backward for the host test's table.
    pre: (softmax(s), dO V^T) when the caller has them already.  ds_prescale: the factor dS carries when it is rounded (DS_FORMS)."""
    P, dP = pre if pre is not None else (torch.softmax(scores64(q, k, bias), dim=-1), dctx @ v.transpose(-1, -2))
    c = 1.0 / (1.0 - p_eff)
    kp = None if keep is None else keep.to(F64)
    if kp is not None:
        dP = dP * kp * c
    if ctx_given is None:
        delta = (P * dP).sum(-1, keepdim=True)
    else:
        delta = (dctx * ctx_given).sum(-1, keepdim=True)
    if mutant == "delta_without_dropout_scale":
        delta = delta * (1.0 - p_eff)
    dS = P * (dP - delta)
    Pk = P if kp is None else P * kp
    if round_model:
        Pk, dS = bf16r(Pk), bf16r(dS * ds_prescale) / ds_prescale
    Pt = Pk * c
    dSq = dS
    if mutant == "last_query_ignored":
        Pt, dS = Pt.clone(), dS.clone()
        for b in range(q.shape[0]):
            n = int(lens[b]) if lens is not None else q.shape[2]
            Pt[b, :, n - 1, :] = 0
            dS[b, :, n - 1, :] = 0
    dv = Pt.transpose(-1, -2) @ dctx
    dk = dS.transpose(-1, -2) @ q / 8.0
    if mutant == "dq_second_key_block_not_added":
        dq = dSq[..., :256] @ k[..., :256, :] / 8.0
    else:
        dq = dSq @ k / 8.0
    if round_model:
        dq, dk, dv = bf16r(dq), bf16r(dk), bf16r(dv)
    return dq, dk, dv


# ---- the forward's CPU rounding model and its mutants --------------------------------------------------------------------
FWD_MUTANTS = ("last_key_dropped", "first_key_of_second_chunk_dropped", "partial_tile_duplicates_last_row", "rescale_skipped_once",
               "p_truncated", "normaliser_from_rounded_p", "normaliser_after_dropout", "dropout_scale_from_requested_p",
               "dropout_pitch_unrounded", "lse_off_by_ln2_2^-10", "head_reads_next_heads_v")
BWD_MUTANTS = ("delta_without_dropout_scale", "last_query_ignored", "dq_second_key_block_not_added")


def forward_model(q, k, v, bias, keep=None, p_eff=0.0, head_scale=None, mutant=None, lens=None, p_requested=None,
                  keep_mutant=None):
    """The kernel's own roundings and nothing else: fp64 everywhere, the un-normalised P rounded to bf16 before P.V (the
    normaliser sums the unrounded values), the output rounded to bf16.  Returns ctx, lse, probs like attention_ref64.
    mutant: one of FWD_MUTANTS.  lens: the sequences' lengths (defaults to S).  p_requested / keep_mutant: what the mutants
    "dropout_scale_from_requested_p" / "dropout_pitch_unrounded" use instead of p_eff / keep."""
    B, nh, S, _ = q.shape
    lens = [S] * B if lens is None else [int(n) for n in lens]
    s = scores64(q, k, bias).clone()
    if mutant == "head_reads_next_heads_v":
        v = torch.roll(v, -1, dims=1)
    if mutant == "last_key_dropped":
        for b, n in enumerate(lens):
            if n > 1:
                s[b, :, :, n - 1] = -math.inf
    if mutant == "first_key_of_second_chunk_dropped":
        for b, n in enumerate(lens):
            if n > 256:
                s[b, :, :, 256] = -math.inf
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    if mutant == "partial_tile_duplicates_last_row":   # the clamped reads of keys n .. 32 ceil(n / 32) - 1 not cancelled
        p = p.clone()
        for b, n in enumerate(lens):
            p[b, :, :, n - 1] *= 1 + (-n) % 32
    if mutant == "rescale_skipped_once" and S > 32:    # tile 0's sums keep the scale of tile 0's maximum
        m0 = s[..., :32].amax(-1, keepdim=True)
        m1 = torch.maximum(m0, s[..., 32:64].amax(-1, keepdim=True))
        p = p.clone()
        p[..., :32] *= torch.exp(torch.where(torch.isfinite(m0), m1 - m0, torch.zeros_like(m0)))
    if mutant == "dropout_pitch_unrounded":
        keep = keep_mutant
    kp = None if keep is None else keep.to(F64)
    pk = p if kp is None else p * kp
    pb = bf16_trunc(pk) if mutant == "p_truncated" else bf16r(pk)
    if mutant == "normaliser_from_rounded_p":
        l = bf16r(p).sum(-1, keepdim=True)
    elif mutant == "normaliser_after_dropout":
        l = pk.sum(-1, keepdim=True)
    else:
        l = p.sum(-1, keepdim=True)
    scale = 1.0 / (1.0 - (p_requested if mutant == "dropout_scale_from_requested_p" else p_eff))
    o = (pb @ v) / l * scale
    if head_scale is not None:
        o = o * head_scale.to(F64).view(1, -1, 1, 1)
    lse = (m + torch.log(l)).squeeze(-1)
    if mutant == "lse_off_by_ln2_2^-10":
        lse = lse + math.log(2.0) * 2.0 ** -10
    return bf16r(o), lse, p / l


# ---- bounds --------------------------------------------------------------------------------------------------------------
class ForwardTerms(object):
    """The fp64 reference of one case and the magnitudes its bounds are made of."""

    def __init__(self, q, k, v, bias, keep=None, p_eff=0.0, head_scale=None):
        self.ctx, self.lse, self.probs = attention_ref64(q, k, v, bias, keep, p_eff, head_scale)
        s = scores64(q, k, bias)
        fin = torch.isfinite(s)
        zero = torch.zeros((), dtype=F64)
        self.s = s
        self.smax = torch.where(fin, s.abs(), zero).amax(-1)                                         # [B, nh, S]
        self.D = torch.where(fin, (q.abs() @ k.abs().transpose(-1, -2) / 8.0).expand_as(s), zero).amax(-1)
        pt = self.probs
        km = _keep_scale(keep, p_eff)
        if km is not None:
            pt = pt * km
        self.head_scale = None if head_scale is None else head_scale.to(F64).view(1, -1, 1, 1)
        if head_scale is not None:
            pt = pt * self.head_scale.abs()
        self.A = pt @ v.abs()
        self.has_key = fin.any(-1)                                                                    # [B, nh, S]

    def f32_factor(self):
        """max(1, max|s| / 128, D / 16) per row: where the scores leave the range the fp32 terms were derived for."""
        return torch.clamp(torch.maximum(self.smax / 128.0, self.D / 16.0), min=1.0)

    def forward_bound(self):
        return U * self.A + U * self.ctx.abs() + 2.0 ** -12 * self.f32_factor().unsqueeze(-1) * self.A

    def lse_bound(self):
        return 2.0 ** -23 * (4.0 * (1.0 + self.smax) + 32.0 * self.D)

    def probs_rel_bound(self):
        return 2.0 ** -23 * (8.0 + 2.0 * (self.s - self.lse.unsqueeze(-1)).abs()
                              + (4.0 * (1.0 + self.smax) + 64.0 * self.D).unsqueeze(-1))


def _ratio(err, bound):
    """max(err / bound); an element with bound 0 must be exact."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def row_select(terms, lens=None):
    """bool [B, nh, S]: the query rows that are compared: a sequence's own rows that keep one finite key."""
    sel = terms.has_key.clone()
    if lens is not None:
        S = sel.shape[-1]
        sel &= (torch.arange(S)[None, :] < torch.as_tensor(lens)[:, None])[:, None, :]
    return sel


def signed_stat(err, ref, bound):
    """(stat sqrt(N) / 6, N) for stat = mean(err sign(ref) / bound): must be within [-1, 1] (module docstring)."""
    ok = bound > 0
    n = int(ok.sum())
    if n == 0:
        return 0.0, 0
    stat = float((err[ok] * torch.sign(ref[ok]) / bound[ok]).mean())
    return stat * math.sqrt(n) / 6.0, n


def forward_ratios(terms, ctx, lse=None, probs=None, lens=None, signed=False):
    """{check: measured / bound} of a forward result (ctx [B, nh, S, 64], lse [B, nh, S], probs [B, nh, S, S] incl. head scale)
    against `terms`; every value must be <= 1 (the signed statistic: within [-1, 1])."""
    sel = row_select(terms, lens)
    out = {}
    ctx = ctx.to(F64)
    assert bool(torch.isfinite(ctx[sel]).all()), "non-finite context on a row with a finite key"
    err, bound = (ctx - terms.ctx)[sel], terms.forward_bound()[sel]
    out["ctx err/bound"] = _ratio(err.abs(), bound)
    if signed:
        out["ctx signed bias"], n = signed_stat(err, terms.ctx[sel], bound)
        assert n >= 100000, "the signed statistic wants N >= 1e5 (N = %d)" % n
    if lse is not None:
        lse = lse.to(F64)
        assert bool(torch.isfinite(lse[sel]).all()), "non-finite lse on a row with a finite key"
        out["lse err/bound"] = _ratio((lse - terms.lse)[sel].abs(), terms.lse_bound()[sel])
    if probs is not None:
        p, want = probs.to(F64)[sel], terms.probs[sel]
        hs = 1.0 if terms.head_scale is None else terms.head_scale.expand(sel.shape + (1,))[sel]
        assert bool(torch.isfinite(p).all()), "non-finite probability on a row with a finite key"
        e = (p - want * hs).abs()
        big = want >= 2.0 ** -100
        b = torch.where(big, terms.probs_rel_bound()[sel] * want * abs_(hs), torch.full_like(want, 2.0 ** -100) * abs_(hs)
                        + torch.zeros_like(want))
        out["probs err/bound"] = _ratio(e, b)
        S = want.shape[-1]
        rs = (S * 2.0 ** -23 * terms.f32_factor()[sel] + terms.lse_bound()[sel]).unsqueeze(-1)
        out["probs rowsum err/bound"] = _ratio((p.sum(-1, keepdim=True) - hs).abs(), abs_(hs) * rs)
    return out


def abs_(x):
    return abs(x) if isinstance(x, float) else x.abs()


class BackwardTerms(object):
    """want (fp64 closed form), the rounding model's error and the fp32 floor F of one backward case."""

    def __init__(self, q, k, v, bias, dctx, ctx_given, keep=None, p_eff=0.0, valid_b=None):
        B = q.shape[0]
        self.valid_b = torch.ones(B, dtype=torch.bool) if valid_b is None else valid_b
        s = scores64(q, k, bias)
        P = torch.softmax(s, dim=-1)
        pre = (P, dctx @ v.transpose(-1, -2))
        self.want = attention_bwd_ref64(q, k, v, bias, dctx, None, keep, p_eff, pre=pre)
        self.models = {"folded": attention_bwd_ref64(q, k, v, bias, dctx, ctx_given, keep, p_eff, round_model=True, pre=pre)}
        self.models["deferred"] = self.models["folded"] if not p_eff > 0 else attention_bwd_ref64(
            q, k, v, bias, dctx, ctx_given, keep, p_eff, round_model=True, pre=pre, ds_prescale=1.0 - p_eff)
        self.model = self.models["folded"]
        del pre
        km = _keep_scale(keep, p_eff)
        Pt = P if km is None else P * km
        dPa = dctx.abs() @ v.abs().transpose(-1, -2)
        if km is not None:
            dPa = dPa * km
        br = dPa + (P * dPa).sum(-1, keepdim=True)                                  # |dP| + |delta|
        rel = 2.0 ** -21 * torch.clamp(torch.where(torch.isfinite(s), s.abs(), torch.zeros((), dtype=F64)), min=1.0)
        dSa = P * br
        fS = (2.0 ** -18 + rel) * dSa
        self.F = (fS @ k.abs() / 8.0, fS.transpose(-1, -2) @ q.abs() / 8.0,
                  ((2.0 ** -18 + rel) * Pt).transpose(-1, -2) @ dctx.abs())
        self.A = (dSa @ k.abs() / 8.0, dSa.transpose(-1, -2) @ q.abs() / 8.0, Pt.transpose(-1, -2) @ dctx.abs())


# Where the dropout scale meets the rounding of dS (both are minimal: ONE rounding of dS; 1 - p is no power of two, so the two
# forms round the same dS to different bf16 values and their errors are different draws of the same size):
#   "folded"    dS / (8 (1 - p)) ... is rounded with every scale folded in: csrc/attention_bwd_keyblock.hip, the 4-wave kernel
#               (`sacc[i] = p * (dpv - del4[g4][e]) * ds_scale;  // dS' (scales folded in)`)
#   "deferred"  P (keep dP_raw - delta (1 - p)) = (1 - p) dS is rounded, and ds_scale = 1 / (8 (1 - p)) multiplies the fp32 dK / dQ
#               accumulators afterwards: the 8-wave kernel (the same file) and both 16-wave kernels (attention_bwd_w16.hip,
#               attention_bwd_w16p.hip) (`sacc[i] = p * (dpv - del4_g[e]);   // dS' up to ds_scale`,
#               `dsv[4 * t + j] = p * (dpv - e4[j]);`)
# Without dropout the two coincide.  Measured on an MI355X before the forms were told apart: every kernel's dV and the 4-wave
# kernel's dQ / dK reproduce the "folded" model's error exactly (max ratio 0.333 = 1 / 3), the other kernels' dQ / dK under
# dropout are the other draw (L2 within 1.12 x the model's; one element of 4 224 in one (batch, head) of a 256-sequence sweep one
# bf16 ulp from the model's value where the model happened to sit 0.09 ulp from fp64: max ratio 1.024; the CPU "folded" model
# judged against the "deferred" one on the same sweep: 1.07).
DS_FORMS = ("folded", "deferred")


def backward_ratios(terms, got, lens=None, signed=False, ds_form="folded"):
    """{check: measured / bound} of dq, dk, dv ([B, nh, S, 64] each) against the margins of the module docstring; ds_form: which
    of DS_FORMS the implementation under test is."""
    out = {}
    B, nh, S, _ = terms.want[0].shape
    rows = torch.ones(B, S, dtype=torch.bool) if lens is None else torch.arange(S)[None, :] < torch.as_tensor(lens)[:, None]
    rows = (rows & terms.valid_b[:, None])[:, None, :, None].to(F64)
    for name, g, w, m, F, A in zip(("dq", "dk", "dv"), got, terms.want, terms.models[ds_form], terms.F, terms.A):
        g = g.to(F64)
        vb = terms.valid_b
        assert bool(torch.isfinite(g[vb]).all()), "non-finite %s" % name
        ek, em, F = (g - w) * rows, (m - w) * rows, F * rows
        ek, em, F = ek[vb], em[vb], F[vb]
        l2 = ek.flatten(2).norm(dim=-1) / (2.0 * em.flatten(2).norm(dim=-1) + F.flatten(2).norm(dim=-1))
        mx = ek.flatten(2).abs().amax(-1) / (3.0 * em.flatten(2).abs().amax(-1) + F.flatten(2).abs().amax(-1))
        zero = ek.flatten(2).abs().amax(-1) == 0
        out[name + " l2 err/bound"] = float(torch.where(zero, torch.zeros_like(l2), l2).max())
        out[name + " max err/bound"] = float(torch.where(zero, torch.zeros_like(mx), mx).max())
        if signed:
            sc = (U * w.abs() + U * A)[vb] * rows[vb].expand_as(ek)
            out[name + " signed bias"], n = signed_stat(ek, w[vb], sc)
            assert n >= 100000, "the signed statistic wants N >= 1e5 (N = %d)" % n
    return out


def passes(ratios):
    return all((abs(r) <= 1.0) and r == r for r in ratios.values())


def assert_ratios(name, ratios):
    """Record every ratio through helpers.check_close (bound 1: it lands in the session's parity_measured.txt) and assert it."""
    from helpers import check_close

    for key in sorted(ratios):
        check_close("attn conformance %s: %s" % (name, key), ratios[key], 0.0, 1.0)


# ---- case builders shared by the host and the GPU file ----------------------------------------------------------------------
FORMS = ("-10000", "fractional", "-inf", "finfo.min")
SCORE_SHAPES = ("rising", "falling", "max in last tile", "max in second chunk", "shift +200")


def mask_patterns(S):
    """[6, S] raw masks, one pattern per sequence: random 25 % masked; only key 0 kept; nothing kept (softmax of the raw scores);
    the first min(64, S - 1) keys masked; the last partial tile masked (S > 32); alternating.  Every pattern but "nothing kept"
    keeps at least one key at every S."""
    g = torch.Generator().manual_seed(1000 + S)
    m = torch.ones(6, S)
    m[0] = (torch.rand(S, generator=g) > 0.25).float()
    m[0, 0] = 1
    m[1, 1:] = 0
    m[2] = 0
    m[3, :min(64, S - 1)] = 0
    if S > 32:
        m[4, ((S - 1) // 32) * 32:] = 0
    m[5, 1::2] = 0
    return m


def form_bias(raw, form):
    """[S] fp32 additive bias of one raw mask row in one of FORMS (fractional: a masked key 0.5 -> -5 000, a kept last key
    2.0 -> +10 000)."""
    if form == "-10000":
        return (1.0 - raw) * -10000.0
    if form == "fractional":
        frac = torch.where(raw == 0, 0.5, 1.0)
        frac[-1] = 2.0 if raw[-1] == 1 else 0.5
        return (1.0 - frac) * -10000.0
    fill = -math.inf if form == "-inf" else float(torch.finfo(torch.float32).min)
    return torch.where(raw == 1, 0.0, fill).float()


def score_ramp(what, S):
    """[S] fp32, added to every score of key k (q[0] = 8, k[0] = ramp): scores that rise from key tile to key tile (the online
    softmax's rescale taken at every tile), fall (taken once), peak in the last partial tile / the first tile of the second
    256-chunk, or all share +200 (shift invariance, no overflow)."""
    tile = (torch.arange(S) // 32).float()
    return {"rising": tile * 0.5, "falling": -tile * 0.5, "max in last tile": (tile == (S - 1) // 32).float() * 4.0,
            "max in second chunk": (tile == 8).float() * 4.0, "shift +200": torch.full((S,), 200.0)}[what]


# ---- exact constructions -------------------------------------------------------------------------------------------------
def bit_columns(S):
    """V [S, 64] of +-1: column j of key k = bit (j mod 11) of k.  With Q = 0 every context element of a sequence of n keys is
    (2 count - n) / n rounded once to bf16: any dropped, duplicated or out-of-range key changes a count."""
    kk = torch.arange(S)[:, None]
    jj = torch.arange(64)[None, :] % 11
    return (((kk >> jj) & 1) * 2 - 1).to(F64)


def bit_columns_expected(n):
    """(expected bf16 row [64] as float64, unique): unique = the bf16 rounding of (2 count - n) / n does not depend on an error of
    2^-22 relative (the fp32 product of the integer sum with 1 / n), or the value is computed exactly (n a power of two)."""
    x = bit_columns(n).sum(0) / n
    lo, hi = bf16r(x * (1 - 2.0 ** -22)), bf16r(x * (1 + 2.0 ** -22))
    pow2 = (n & (n - 1)) == 0
    return bf16r(x), bool(pow2 or torch.equal(lo, hi))


def permutation_case(S, nh, seed):
    """K[k] = random +-8 codes, Q[q] = K[pi(q)]: score(q, pi(q)) = 512, any other key at most 512 - 16 d / 8 ... lower by a
    margin that makes its probability < 2^-60, so ctx[q] == V[pi(q)] bit for bit.  Returns qkv [S, 3 nh 64] fp32 (bf16-exact),
    pi [nh, S]."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(S, 3, nh, 64)
    pis = []
    for h in range(nh):
        while True:
            K = (torch.randint(0, 2, (S, 64), generator=g) * 2 - 1).float() * 8.0
            if torch.unique(K, dim=0).shape[0] == S:
                break
        pi = torch.randperm(S, generator=g)
        qkv[:, 0, h], qkv[:, 1, h] = K[pi], K
        qkv[:, 2, h] = torch.randn(S, 64, generator=g).to(torch.bfloat16).float()
        pis.append(pi)
    return qkv.reshape(S, 3 * nh * 64), torch.stack(pis)
