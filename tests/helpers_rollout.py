"""float64 references, CPU models, float32 emulations, derived per-element bounds and the case table of the rollout caller's
kernels: csrc/rollout.hip (lstm_step_kernel, lstm_step_bwd_kernel, softdot_kernel, softdot_bwd_kernel<1|2>,
softdot_bwd_dots / softdot_bwd_apply<1|2>, skinny_linear_kernel<GRID>) and csrc/lstm_persistent.hip (lstm_persistent_kernel,
whose arithmetic per step is the step kernel's).

Everything here is plain numpy / torch on the CPU.  tests/test_host_rollout_reference.py proves, without a GPU, that the bounds
accept the minimal implementation (float64, every output rounded once) and float32 emulations in four summation orders with the
fast exponential and reciprocal pushed one ulp either way, never go vacuous outside the elements a case names, and reject a table
of subtly wrong implementations; tests/test_gpu_rollout_conformance.py holds the HIP kernels to the same bounds.  No bound below
was chosen by looking at a kernel's output; every quantity on the right of a bound is the float64 reference's own.

NOTATION  e = 2^-24 (fp32 unit round-off), u = 2^-8 (bf16).  x~ = the bf16 round-to-nearest-even of x.
  DOT PRODUCTS are helpers_gemm's F: products of two bf16 values are exact in fp32 and the MFMA's inner sum is not documented as
  round to nearest, so a K-term MFMA product carries dot(K, S) = (K + 8) 2^-23 S with S = sum |terms| (+ |bias|, |xproj|: the
  values added to it); an fp32 x fp32 product chain of the attention kernels (plain v_fma / v_add, round to nearest) carries
  (K + 8) e S: each product rounds once (e |term|), K - 1 additions in ANY order move the sum by at most (K - 1) e S.
  __expf(a) is helpers_attention's / helpers_loss's model: the log2(e) multiply and its rounding give a relative 2 |a| e, v_exp_f32
  one ulp: rexp(a) = (2 |a| + 4) e relative (helpers_loss's a_j, two to spare), and below a result of 2^-100 only an absolute floor.
  v_rcp_f32 is one ulp (2 e relative).

ACTIVATIONS (rollout.hip: sigmoidf_, tanhf_)
  sigmoid(x) = rcp(1 + E), E = __expf(-x).  d sigma / dE = -sigma^2 and sigma^2 E = sigma (1 - sigma):
      eps_sig(x) = sigma (1 - sigma) rexp(x) + 4 e sigma           (the sum 1 + E: e; rcp: 2 e; one to spare)
    For x >~ 17 E underflows against 1 and the result is exactly 1 where the reference is 1 - 6e-8: inside 4 e sigma.
  tanh(x)  = sign(x) (1 - E) rcp(1 + E), E = __expf(-2 |x|).  d t / dE = -2 / (1 + E)^2 and 4 E / (1 + E)^2 = 1 - t^2:
      eps_tanh(x) = (1 - t^2) / 2 rexp(2 x) + 5 e |t|               (1 - E, 1 + E: e each; rcp 2 e; the product e)
    For |x| -> 0, E -> 1 and 1 - E is formed exactly from an E that carries an ABSOLUTE error of about rexp(0) = 4 e: the first
    term tends to 2 e and does not shrink with |t|.  The error of tanhf_ is absolute there, a few e, not relative -- a kernel that
    switched to the series x - x^3 / 3 would be far more accurate at |x| < 2^-10 and 0.6 % off at |x| = 0.4 (mutant table).
  An error d of the argument enters through the derivative; over [x - d, x + d] the derivative of either activation grows by at
  most exp(2 d) <= 1 + 4 d (d < 1/2):  act_err(x, d) = min(1, act'(x) (1 + 4 d)) d + eps_act(x)  (sigmoid: min(1/4, ...)).

LSTM STEP (lstm_values; torch.nn.LSTM gate order i, f, g, o; K = hs)
  z_q = xproj_q + h~ . W_hh[q]^T,   S_q = |xproj_q| + sum_k |h~_k w_k|,   d_q = dot(hs, S_q)
  E_i, E_f, E_o = act_err_sig(z, d),  E_g = act_err_tanh(z_g, d_g)                        -> the saved gates' bounds
  c' = f c + i g:        E_c = |c| E_f + |g| E_i + i E_g + E_i E_g + 3 e (|f c| + |i g|)    (two products, one sum)
  h' = o tanh(c'):       E_t = act_err_tanh(c', E_c),  E_h = |tanh c'| E_o + o E_t + E_o E_t + e |h'|
  seq_out[t] = h'.  Exact contracts: an inactive row (t >= lengths[b]) passes h and c through bit for bit, writes an exact-zero
  output position and leaves its saves untouched; sv_c is the input c bit for bit; sv_h is torch's .to(bfloat16) of h_prev.

LSTM STEP, BACKWARD (lstm_bwd_values; K = 4 hs: the product runs over the four gates' gradients)
  inputs as they are: dg_next (bf16), W_hh^T (bf16), the saved activated gates i f g o and c_prev (fp32), dc, d_out, dh_final.
  dh  = [row active at t_next: dg_next . W_hh^T[hid] | else dh_final | 0] + d_out
        E_dh = dot(4 hs, sum |dg_next w|) [if the product is taken] + e |dh| [if d_out is added]
  c'  = f c_prev + i g from the SAVED values:  E_cn = 3 e (|f c| + |i g|),  tc = tanh(c'): E_tc = act_err_tanh(c', E_cn)
  q   = 1 - tc^2:        E_q = 2 |tc| E_tc + E_tc^2 + 2 e
  dc  = dc_in + dh o q:  E_dc = o (E_dh q + |dh| E_q + E_dh E_q) + 4 e |dh o q| + e |dc_in|
  di = dc g i (1 - i), df = dc c_prev f (1 - f):  E = E_dc |factor| + 5 e |value|          (1 - i: e; three products)
  dg = dc i (1 - g^2):   E = E_dc i (1 - g^2) + 2 e |dc i| + 3 e |dg|   (1 - g^2 CANCELS for |g| -> 1: absolute 2 e on it)
  do = dh tc o (1 - o):  E = o (1 - o) (E_dh |tc| + |dh| E_tc + E_dh E_tc) + 5 e |do|
  dc_out = dc f:         E = E_dc f + e |dc f|
  the fp32 gate gradients carry E; the bf16 ones u |x| + (1 + u) E.  An inactive row: exact-zero gate gradients, dc untouched.

SOFT-DOT ATTENTION (softdot_values; K = D + L).  Masked context rows never enter (the reference zeroes them first).
  s_l = c_l . t,  Sct_l = sum_d |c_ld t_d|,  E_s,l = (D + 8) e Sct_l;  a masked key's logit is exactly -inf.
  p_l = exp(s_l - m) / Z.  The error of a logit is relative in its exp, once through the key itself and once through the sum:
      rp_l = E_s,l + sum_j p_j E_s,j + rexp(s_l - m) + sum_j p_j rexp(s_j - m) + 2 E_s,max + (L + 6) e
      E_p,l = p_l expm1(rp_l)  where p_l >= 2^-100;  2^-100 (absolute, nothing else) below;  exactly 0 for a masked key.
    (2 E_s,max: the computed maximum may sit E_s away from the true one, which moves both arguments; (L + 6) e: the L - 1
    additions of positive terms in any order, the division and the product.)
  weighted_d = sum_l p_l c_ld:  E_w = sum_l E_p,l |c_ld| + (L + 8) e sum_l p_l |c_ld|.
  A batch row with every key masked is NaN in its probabilities and weighted sum (its logits are -inf); no other row is affected.

SOFT-DOT BACKWARD (the same function; one-workgroup and two-launch forms share the bound)
  dp_l = c_l . dW (+ dA_l, probabilities returned), 0 for a masked key:  E_dp = (D + 8) e sum_d |c dW| + e |dp|
  P = sum_l p_l dp_l:   E_P = sum_l (E_p |dp| + p E_dp) + (L + 8) e sum_l p |dp|
  dlog_l = p_l (dp_l - P) (+ dA_l, logits returned, unmasked keys only).  dp - P CANCELS: only an absolute bound in
  p (|dp| + sum p |dp|) can be promised:
      E_dl = E_p (|dp| + |P|) + p (E_dp + E_P) + 3 e p (|dp| + |P|) + e |dlog|
  d_target_d = sum_l dlog_l c_ld:  E = sum_l E_dl |c_ld| + (L + 8) e sum_l |dlog_l c_ld|
  d_context[l, d] = p_l dW_d + dlog_l t_d:  E = E_p |dW_d| + E_dl |t_d| + 3 e (|p dW| + |dlog t|); a masked key's row is exactly
  zero for finite dW; an all-masked batch row is NaN.

SKINNY LINEAR (skinny_values; K = K0 + K1)  z = [x0 | x1]~ . W^T + b,  S = sum |x~ w| + |b|,  d = dot(K, S);
  out = z: E = d;   out = tanh(z): E = act_err_tanh(z, d).

VACUITY (vacuity)  For every element a case does not name, bound <= (4 K + 256 + 4 A) e N_j, with K the total length of the
reductions feeding the element (hs; 4 hs for the backward step; D + L; K0 + K1), A the largest |argument| of an exp in the
element's formula and N_j the first-order magnitude of the element: |y_j| plus the sum over the float64 terms it is made of of
|dy_j / dterm| |term| -- the terms being the products and addends of every reduction and the factors of every product:
  gates            N = |act(z)| + act'(z) S
  c'               N = |f c| + |i g| + |c| N_f' + |g| N_i' + i N_g'     (N_q' = act'(z_q) S_q)
  h', seq_out      N = |h'| + |tanh c'| N_o' + o (1 - tanh^2 c') N_c
  gate gradients   the formulas of E above with E_dh -> sum |dg_next w| + |d_out| + |dh_final|, E_cn -> |f c| + |i g|, every
                   "k e |x|" -> |x|
  logits           N = Sct;  probabilities N = p (1 + Sct_l + sum_j p_j Sct_j);  weighted N = sum_l N_p,l |c_ld|
  dlog             N = N_p (|dp| + sum p |dp|) / p + p (Scw_l + sum_j p_j Scw_j + |dA_l| + sum p |dA|) + |dA_l|
  d_target         N = sum_l N_dl |c_ld|;  d_context N = N_p |dW_d| + N_dl |t_d|
  skinny_linear    N = |out| + act'(z) S
Named elements (held to their bound and to finiteness like every other, excused from the cap): the elements of an all-masked row
(NaN; at most one batch row per case); elements whose probability lies below 2^-100 (absolute floor only; only kind `peaked`, at
most half a row) together with the d_context rows of those keys; the absolute-error region of tanhf_ -- elements whose formula
takes a tanh at |x| < 2^-10 (only kind `tiny`).

WHICH CASE REACHES WHICH BRANCH (asserted by tests/test_host_rollout_reference.py from the kernels' own selection rules)
  softdot load width     vec: D in 4, 512, 1024, 2052, 4096 on 16-byte aligned views; vec2: D in 2, 6, 130, 2058 on even strides, base 8
                         bytes in; element: odd D (1, 3, 129, 1025, 2055), D = 512 one float into its buffer, D = 130 on an odd row stride
  softdot key parts      D = 4: 8 (L >= 8), 7 (L = 7), 1 (L = 1); D = 1024 vec: 4; D = 512 vec: 8; D = 2052, 4096, 1025, 2055: 1, and the
                         threads walk the column groups at 1025 / 2055; L = 1030 > 1024: more keys than threads in the softmax loops
  softdot backward       W = 2: the vec2 cases; W = 1: every other; one workgroup / two launches: every case in both
                         (ops.SOFTDOT_SPLIT_KEYS); L = 40, 128, 129, 159, 161 put the last chunk of the two-launch form at 8, 32, 1, 31
                         and 1 keys; D = 1028 (W = 1) and 2058 (W = 2) walk the columns with one part
  skinny_linear          form `grid`: skinny_linear_kernel<true>; `strided`, `off4`, `odd`: <false> (load4_cat by address: 8-byte, and
                         element loads); (5, 6, 32) and (130, 3, 160) put the x0 | x1 seam inside a 4-column group; (32, 0, 32) leaves
                         three waves without a K-step; (128, 128, 288) has Kpad beyond K
  lstm_step_kernel       hs = 128 and 256; B = 1, 15, 16, 17, 33 (one to three batch tiles, full and partial); with and without lengths
  lstm_step_bwd_kernel   dg_next given with t_next inside / outside a row's length and t_next = -1 (the MFMA product taken, discarded
                         for dh_final, not taken), d_out / dh_final / lengths absent, dc zero
  lstm_persistent_kernel (B, hs) = (21, 128): <KS = 1, NBT = 2>;  (5, 256): <KS = 2, NBT = 1>   (tests/test_gpu_rollout_conformance.py)

MUTANTS LEFT OUT  "the max taken over masked keys too" (softmax is invariant to the shift until it overflows) and "1 / Z as
v_rcp_f32 instead of a division" (one ulp, inside (L + 6) e) cannot be seen by a bound derived from fp32 arithmetic.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch

from helpers_attention import bf16_trunc, bf16r
from helpers_loss import expf as expf32          # the one float32 model of __expf (helpers_attention's, as code)

F64 = torch.float64
F32 = np.float32
E = 2.0 ** -24
U = 2.0 ** -8
FLOOR = 2.0 ** -100
TINY = 2.0 ** -10
INF = float("inf")
SENTINEL = -768.0      # exact in bf16 too
SD_THREADS, SDB_KEYS = 1024, 32


def dot_mfma(K, S):
    """helpers_gemm's F"""
    return (K + 8) * 2.0 ** -23 * S


def dot_f32(K, S):
    return (K + 8) * E * S


def rexp(a):
    return (2.0 * a.abs() + 4.0) * E


def eps_sig(x):
    s = torch.sigmoid(x)
    return s * (1 - s) * rexp(x) + 4 * E * s


def eps_tanh(x):
    t = torch.tanh(x)
    return (1 - t * t) / 2 * rexp(2 * x) + 5 * E * t.abs()


def err_sig(x, d):
    s = torch.sigmoid(x)
    return torch.clamp(s * (1 - s) * (1 + 4 * d), max=0.25) * d + eps_sig(x)


def err_tanh(x, d):
    t = torch.tanh(x)
    return torch.clamp((1 - t * t) * (1 + 4 * d), max=1.0) * d + eps_tanh(x)


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _gen(name):
    return torch.Generator().manual_seed(_seed(name))


def f32(x):
    return x.to(torch.float32)


class Out(object):
    """One output of one case: the float64 value y, its bound, its magnitude N, the largest exp argument A, the named elements."""

    def __init__(self, y, bound, N=None, A=None, named=None, u=0.0):
        self.y = y
        self.bound = (u * y.abs() + (1 + u) * bound) if u else bound
        self.E, self.N, self.A = bound, N, A
        self.named = torch.zeros(y.shape, dtype=torch.bool) if named is None else named.expand(y.shape).clone()


class Case(object):
    def __init__(self, name, op, kind="normal", **kw):
        self.name, self.op, self.kind = name, op, kind
        self.__dict__.update(kw)

    def __repr__(self):
        return "Case(%s)" % self.name


# =====================================================================================================================================
# LSTM step, forward
# =====================================================================================================================================
def _tanh_series(x):
    return x - x ** 3 / 3.0


def lstm_values(x, h, c, w, active=None, mut=None):
    """x [B, 4hs] fp32-exact float64, h / c [B, hs], w [4hs, hs] (bf16 values), active bool [B] or None -> dict of float64 values
    (h_out, c_out, seq_out, sv_g [B, 4hs], and the intermediates the bounds are made of).  Inactive rows: h, c passed through,
    seq_out 0; their saves are reported as NaN (untouched: the test compares them with the buffer's sentinel)."""
    B, hs = h.shape
    act = torch.ones(B, dtype=torch.bool) if active is None else active
    hq = bf16_trunc(h) if mut == "h_prev_truncated" else (h if mut == "h_prev_left_in_fp32" else bf16r(h))
    P = hq[:, None, :] * w[None, :, :]
    if mut == "k_quarter_dropped":
        P = P.clone()
        P[:, :, 2 * (hs // 4):3 * (hs // 4)] = 0
    z = x + P.sum(-1)
    S = x.abs() + P.abs().sum(-1)
    zs, Ss = list(z.split(hs, 1)), list(S.split(hs, 1))
    if mut == "gate_order_igfo":
        zs[1], zs[2] = zs[2], zs[1]
        Ss[1], Ss[2] = Ss[2], Ss[1]
    tanh = _tanh_series if mut == "tanh_small_argument_series" else torch.tanh
    i, f, g, o = torch.sigmoid(zs[0]), torch.sigmoid(zs[1]), tanh(zs[2]), torch.sigmoid(zs[3])
    cn = f * c + i * g
    if mut == "c_from_new_c":
        cn = f * cn + i * g
    tc = tanh(cn)
    hn = o * tc
    a2 = act[:, None]
    keep = torch.ones_like(a2) if mut == "inactive_state_updated" else a2
    V = dict(z=zs, S=Ss, i=i, f=f, g=g, o=o, cn=cn, tc=tc, hn=hn, act=act, c=c, h=h)
    V["h_out"] = torch.where(keep, hn, h)
    V["c_out"] = torch.where(keep, cn, c)
    V["seq_out"] = torch.where(a2, hn, h if mut == "inactive_output_nonzero" else torch.zeros_like(hn))
    V["sv_g"] = torch.cat([i, f, g, o], 1)
    return V


def lstm_terms(x, h, c, w, active=None, tiny=False):
    """-> {output: Out} for h_out, c_out, seq_out, sv_g (the module docstring's LSTM STEP)"""
    V = lstm_values(x, h, c, w, active)
    hs = h.shape[1]
    z, S = V["z"], V["S"]
    d = [dot_mfma(hs, s) for s in S]
    i, f, g, o, cn, tc, hn = V["i"], V["f"], V["g"], V["o"], V["cn"], V["tc"], V["hn"]
    Ei, Ef, Eo, Eg = err_sig(z[0], d[0]), err_sig(z[1], d[1]), err_sig(z[3], d[3]), err_tanh(z[2], d[2])
    Ec = c.abs() * Ef + g.abs() * Ei + i * Eg + Ei * Eg + 3 * E * ((f * c).abs() + (i * g).abs())
    Et = err_tanh(cn, Ec)
    Eh = tc.abs() * Eo + o * Et + Eo * Et + E * hn.abs()
    Ni, Nf, No, Ng = i * (1 - i) * S[0], f * (1 - f) * S[1], o * (1 - o) * S[3], (1 - g * g) * S[2]
    Nc = (f * c).abs() + (i * g).abs() + c.abs() * Nf + g.abs() * Ni + i * Ng
    Nh = hn.abs() + tc.abs() * No + o * (1 - tc * tc) * Nc
    A = torch.maximum(torch.maximum(z[0].abs(), z[1].abs()), torch.maximum(z[3].abs(), 2 * z[2].abs()))
    Ah = torch.maximum(A, 2 * cn.abs())
    tg = (z[2].abs() < TINY) if tiny else torch.zeros_like(g, dtype=torch.bool)
    th = (tg | (cn.abs() < TINY)) if tiny else tg
    a2 = V["act"][:, None]
    zero = torch.zeros_like(hn)
    out = {"c_out": Out(V["c_out"], torch.where(a2, Ec, zero), Nc, A, tg & a2),
           "h_out": Out(V["h_out"], torch.where(a2, Eh, zero), Nh, Ah, th & a2),
           "seq_out": Out(V["seq_out"], torch.where(a2, Eh, zero), Nh, Ah, th & a2)}
    Eg4 = torch.cat([Ei, Ef, Eg, Eo], 1)
    Ng4 = torch.cat([i + Ni, f + Nf, g.abs() + Ng, o + No], 1)
    A4 = torch.cat([z[0].abs(), z[1].abs(), 2 * z[2].abs(), z[3].abs()], 1)
    named4 = torch.cat([torch.zeros_like(tg), torch.zeros_like(tg), tg, torch.zeros_like(tg)], 1)
    out["sv_g"] = Out(V["sv_g"], Eg4, Ng4, A4, named4)
    return out, V


# =====================================================================================================================================
# LSTM step, backward
# =====================================================================================================================================
def lstm_bwd_values(I, mut=None):
    """I: dict(dgn [B, 4hs] | None, wt [hs, 4hs], dh_final | None, d_out | None, dc [B, hs], svg [B, 4hs], svc [B, hs],
    lens int [B] | None, t, t_next) in float64 -> dict(d [B, 4hs], dc_out [B, hs], intermediates)."""
    svg, cp, dc_in = I["svg"], I["svc"], I["dc"]
    B, hs = cp.shape
    lens = torch.full((B,), 2 ** 31 - 1, dtype=torch.int64) if I["lens"] is None else I["lens"].to(torch.int64)
    t, tn = I["t"], I["t_next"]
    act = (t < lens)[:, None]
    use = ((tn >= 0) & (tn < lens))[:, None] & (I["dgn"] is not None)
    zero = torch.zeros_like(cp)
    if I["dgn"] is not None:
        P = I["dgn"][:, None, :] * I["wt"][None, :, :]
        prod, Sp = P.sum(-1), P.abs().sum(-1)
    else:
        prod, Sp = zero, zero
    fin = zero if I["dh_final"] is None else I["dh_final"]
    if mut == "dh_final_where_dg_next_should_be":
        use = torch.zeros_like(use)
    dh0 = torch.where(use, prod, zero if mut == "dh_final_missing_at_a_rows_last_position" else fin)
    Sdh = torch.where(use, Sp, fin.abs())
    dout = zero if I["d_out"] is None else I["d_out"]
    dh = dh0 + dout
    i, f, g, o = svg.split(hs, 1)
    cn = f * cp + i * g
    tc = torch.tanh(cn)
    q = 1 - tc * tc
    T = dh * o * q
    dc = dc_in + T
    cf = cn if mut == "df_with_new_c" else cp
    d = [dc * g * i * (1 - i), dc * cf * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)]
    dc_out = dc if mut == "dc_not_multiplied_by_f" else dc * f
    V = dict(act=act, use=use, Sp=Sp, Sdh=Sdh + dout.abs(), dh=dh, i=i, f=f, g=g, o=o, cp=cp, cn=cn, tc=tc, q=q, T=T, dc=dc,
             dout=I["d_out"] is not None, dc_in=dc_in)
    V["d"] = torch.where(act, torch.cat(d, 1), torch.zeros_like(svg))
    V["dc_out"] = torch.where(act, dc_out, dc_in)
    return V


def lstm_bwd_terms(I):
    V = lstm_bwd_values(I)
    hs = I["svc"].shape[1]
    i, f, g, o, cp, cn, tc, q, T, dc, dh, dc_in = (V[k] for k in ("i", "f", "g", "o", "cp", "cn", "tc", "q", "T", "dc", "dh", "dc_in"))
    zero = torch.zeros_like(cp)

    def build(Edh, Ecn, k):     # k = 1: the bound; k = None: the magnitude N (every "k e |x|" -> |x|)
        r = (lambda n, x: n * E * x) if k else (lambda n, x: x)
        Etc = err_tanh(cn, Ecn) if k else (q * Ecn + tc.abs())
        Eq = (2 * tc.abs() * Etc + Etc * Etc + 2 * E) if k else (2 * tc.abs() * q * Ecn + q + tc * tc)
        Edc = o * (Edh * q + dh.abs() * Eq + (Edh * Eq if k else 0)) + r(4, T.abs()) + r(1, dc_in.abs())
        Ed = [Edc * (g * i * (1 - i)).abs() + r(5, (dc * g * i * (1 - i)).abs()),
              Edc * (cp * f * (1 - f)).abs() + r(5, (dc * cp * f * (1 - f)).abs()),
              Edc * i * (1 - g * g) + r(2, (dc * i).abs() * (1 if k else g * g + (1 - g * g))) + r(3, (dc * i * (1 - g * g)).abs()),
              o * (1 - o) * (Edh * tc.abs() + dh.abs() * Etc + (Edh * Etc if k else 0)) + r(5, (dh * tc * o * (1 - o)).abs())]
        return torch.cat(Ed, 1), Edc * f + r(1, (dc * f).abs())

    Edh = torch.where(V["use"], dot_mfma(4 * hs, V["Sp"]), zero) + (E * dh.abs() if V["dout"] else 0)
    Ed, Edco = build(Edh, 3 * E * ((f * cp).abs() + (i * g).abs()), 1)
    Nd, Ndco = build(V["Sdh"], (f * cp).abs() + (i * g).abs(), None)
    act4 = V["act"]
    A = (2 * cn.abs())
    Ed = torch.where(act4, Ed, torch.zeros_like(Ed))
    out = {"dg32": Out(V["d"], Ed, Nd, A.repeat(1, 4)), "dg16": Out(V["d"], Ed, Nd, A.repeat(1, 4), u=U),
           "dc": Out(V["dc_out"], torch.where(V["act"], Edco, zero), Ndco, A)}
    return out, V


# =====================================================================================================================================
# soft-dot attention, forward and backward
# =====================================================================================================================================
def sd_parts(G, L):
    """rollout.hip sd_parts: key parts of the weighted-sum / d_target phase for G column groups"""
    return max(1, min(8, L, SD_THREADS // min(G, SD_THREADS)))


def softdot_path(D, row_stride, batch_stride, offset_floats):
    """which load width softdot_kernel takes: rollout.hip sd_aligned (bases: offset_floats into a 256-byte aligned buffer)"""
    al = lambda w: row_stride % w == 0 and batch_stride % w == 0 and (4 * offset_floats) % (4 * w) == 0
    if D % 4 == 0 and al(4):
        return "vec"
    if D % 4 == 2 and al(2):
        return "vec2"
    return "element"


def softdot_values(c, t, mask, dw=None, da=None, prob=True, mut=None):
    """c [B, L, D], t [B, D], mask bool [B, L] | None, dw [B, D] | None, da [B, L] | None -> dict (logit, p, weighted; with a
    gradient: d_target, d_context, dlog).  A masked context row may hold anything: it is zeroed first."""
    B, L, D = c.shape
    mk = torch.zeros((B, L), dtype=torch.bool) if mask is None else mask
    cz = torch.where(mk[:, :, None], torch.zeros_like(c), c)
    cs, ts = cz, t
    if mut == "last_2_columns_of_a_D%4==2_row_dropped" and D % 4 == 2:
        cs = cz.clone()
        cs[:, :, D - 2:] = 0
    Pm = cs * ts[:, None, :]
    s0, Sct = Pm.sum(-1), Pm.abs().sum(-1)
    drop = mk.clone()
    if mut == "key_L-1_dropped_when_L%16!=0" and L % 16 != 0:
        drop[:, L - 1] = True
    if mut == "mask_applied_after_the_softmax":
        s = torch.where(drop & ~mk, torch.full_like(s0, -INF), s0)
    else:
        s = torch.where(drop, torch.full_like(s0, -INF), s0)
    m = s.amax(1, keepdim=True)
    ex = torch.exp(s - m)
    p = ex / ex.sum(1, keepdim=True)
    if mut == "mask_applied_after_the_softmax":
        p = torch.where(mk, torch.zeros_like(p), p)
    logit = torch.where(mk, torch.full_like(s0, -INF), s0)
    cw = c if mut == "masked_keys_inf_multiplied_in" else cs
    pw = p
    if mut == "last_key_part_dropped":
        parts = sd_parts((D + 3) // 4 if D % 2 == 0 else D, L)
        if parts > 1:
            pw = p.clone()
            pw[:, parts - 1::parts] = 0
    with np.errstate(invalid="ignore"):
        weighted = (pw[:, :, None] * cw).sum(1)
    V = dict(s=s, Sct=Sct, p=p, logit=logit, weighted=weighted, mk=mk, cz=cz, allmasked=mk.all(1))
    if dw is None and da is None:
        return V
    zl = torch.zeros((B, L), dtype=F64)
    q0 = zl if dw is None else (cz * dw[:, None, :]).sum(-1)
    Scw = zl if dw is None else (cz * dw[:, None, :]).abs().sum(-1)
    dA = zl if da is None else da
    in_dp = prob != (mut == "d_attn_on_the_wrong_side_of_the_softmax")
    dp = torch.where(mk, zl, q0 + (dA if in_dp else 0))
    dp_sum = torch.where(mk, zl, q0) if mut == "sum_p_dp_without_d_attn" else dp
    Pd = (p * dp_sum).sum(1, keepdim=True)
    dlog = p * (dp - Pd)
    if not in_dp:
        dlog = dlog + (dA if mut == "d_attn_given_to_masked_keys_in_logit_mode" else torch.where(mk, zl, dA))
    dlt = dlog
    if mut == "one_chunk_of_the_split_d_target_dropped" and L > SDB_KEYS:
        dlt = dlog.clone()
        dlt[:, SDB_KEYS:2 * SDB_KEYS] = 0
    d_target = (dlt[:, :, None] * cz).sum(1)
    dwz = torch.zeros((B, D), dtype=F64) if dw is None else dw
    d_context = p[:, :, None] * dwz[:, None, :] + dlog[:, :, None] * t[:, None, :]
    V.update(dp=dp, Scw=Scw, Pd=Pd, dlog=dlog, d_target=d_target, d_context=d_context, dA=dA, in_dp=in_dp, dwz=dwz)
    return V


def softdot_terms(c, t, mask, dw=None, da=None, prob=True, peaked=False):
    V = softdot_values(c, t, mask, dw, da, prob)
    B, L, D = c.shape
    p, s, Sct, mk, cz = V["p"], V["s"], V["Sct"], V["mk"], V["cz"]
    live = ~mk
    zl = torch.zeros((B, L), dtype=F64)
    m = s.amax(1, keepdim=True)
    arg = torch.where(live, s - m, zl)                      # exp arguments (<= 0), 0 for masked keys
    Es = dot_f32(D, Sct)
    Esmax = torch.where(live & (s == m), Es, zl).amax(1, keepdim=True)
    pz = torch.where(live, p, zl)
    rp = Es + (pz * Es).sum(1, keepdim=True) + rexp(arg) + (pz * rexp(arg)).sum(1, keepdim=True) + 2 * Esmax + (L + 6) * E
    small = live & (p < FLOOR)
    Ep = torch.where(small, torch.full_like(p, FLOOR), p * torch.expm1(rp))
    Ep = torch.where(mk, zl, Ep)
    Np = pz * (1 + Sct + (pz * Sct).sum(1, keepdim=True))
    A = arg.abs().amax(1, keepdim=True)
    dead = V["allmasked"][:, None]                                            # [B, 1]: NaN rows, named
    ca = cz.abs()
    Ew = (Ep[:, :, None] * ca).sum(1) + (L + 8) * E * (pz[:, :, None] * ca).sum(1)
    Nw = (Np[:, :, None] * ca).sum(1)
    out = {"logit": Out(V["logit"], torch.where(mk, zl, Es), Sct, zl),
           "p": Out(p, Ep, Np, A.expand(B, L), (small & peaked) | dead),
           "weighted": Out(V["weighted"], Ew, Nw, A.expand(B, D), dead)}
    if dw is None and da is None:
        return out, V
    dp, Pd, dlog, dA, Scw = V["dp"], V["Pd"], V["dlog"], V["dA"], V["Scw"]
    Edp = torch.where(mk, zl, dot_f32(D, Scw) + (E * dp.abs() if V["in_dp"] and da is not None else 0))
    Pabs = (pz * dp.abs()).sum(1, keepdim=True)
    EP = (Ep * dp.abs() + pz * Edp).sum(1, keepdim=True) + (L + 8) * E * Pabs
    Edl = Ep * (dp.abs() + Pd.abs()) + pz * (Edp + EP) + 3 * E * pz * (dp.abs() + Pd.abs()) + E * dlog.abs()
    Edl = torch.where(mk, zl, Edl)
    dAl = torch.where(mk, zl, dA.abs())
    Ndp = Scw + (dAl if V["in_dp"] else 0)
    Ndl = (1 + Sct + (pz * Sct).sum(1, keepdim=True)) * pz * (dp.abs() + Pabs) + pz * (Ndp + (pz * Ndp).sum(1, keepdim=True)) \
        + (0 if V["in_dp"] else dAl)
    Edt = (Edl[:, :, None] * ca).sum(1) + (L + 8) * E * (dlog[:, :, None] * cz).abs().sum(1)
    Ndt = (Ndl[:, :, None] * ca).sum(1)
    dwa, ta = V["dwz"].abs()[:, None, :], t.abs()[:, None, :]
    Edc = Ep[:, :, None] * dwa + Edl[:, :, None] * ta + 3 * E * (pz[:, :, None] * dwa + dlog.abs()[:, :, None] * ta)
    Ndc = Np[:, :, None] * dwa + Ndl[:, :, None] * ta
    out["d_target"] = Out(V["d_target"], Edt, Ndt, A.expand(B, D), dead)
    out["d_context"] = Out(V["d_context"], Edc, Ndc, A[:, :, None].expand(B, L, D), ((small & peaked) | dead)[:, :, None])
    return out, V


# =====================================================================================================================================
# skinny linear
# =====================================================================================================================================
def skinny_values(x0, x1, w, bias, act_tanh, mut=None):
    """x0 [M, K0], x1 [M, K1] | None, w [N, K] (bf16 values, K = K0 + K1), bias [N] | None"""
    x1u = x1
    if mut == "x0_x1_seam_off_by_one" and x1 is not None:
        x1u = torch.cat([x1[:, 1:], torch.zeros_like(x1[:, :1])], 1)
    x = x0 if x1 is None else torch.cat([x0, x1u], 1)
    xq = bf16_trunc(x) if mut == "h_prev_truncated" else (x if mut == "h_prev_left_in_fp32" else bf16r(x))
    P = xq[:, None, :] * w[None, :, :]
    N = w.shape[0]
    b = torch.zeros(N, dtype=F64) if bias is None else bias.clone()
    if mut == "bias_skipped_for_the_last_N%16_columns" and N % 16:
        b[N - N % 16:] = 0
    z = P.sum(-1) + b
    S = P.abs().sum(-1) + b.abs()
    tanh = _tanh_series if mut == "tanh_small_argument_series" else torch.tanh
    return dict(z=z, S=S, out=tanh(z) if act_tanh else z)


def skinny_terms(x0, x1, w, bias, act_tanh, tiny=False):
    V = skinny_values(x0, x1, w, bias, act_tanh)
    K = w.shape[1]
    z, S = V["z"], V["S"]
    d = dot_mfma(K, S)
    if act_tanh:
        t = V["out"]
        o = Out(t, err_tanh(z, d), t.abs() + (1 - t * t) * S, 2 * z.abs(), (z.abs() < TINY) if tiny else None)
    else:
        o = Out(z, d, S, torch.zeros_like(z))
    return {"out": o}, V


# =====================================================================================================================================
# judging
# =====================================================================================================================================
def _same_special(got, want):
    """NaN exactly where the reference is NaN, the same infinities"""
    g, w = got.to(F64), want
    return bool((torch.isnan(g) == torch.isnan(w)).all()) and bool((torch.isinf(g) == torch.isinf(w)).all()) and \
        bool((g[torch.isinf(w)] == w[torch.isinf(w)]).all())


def judge(outs, got, prefix=""):
    """{check: measured / bound} of `got` (name -> tensor) against `outs` (name -> Out); every value must be <= 1.  Elements whose
    bound is 0 must be equal (else the ratio is inf); NaN / inf must sit exactly where the reference has them."""
    rs = {}
    for k, g in got.items():
        O = outs[k]
        g = g.detach().cpu().to(F64).reshape(O.y.shape)
        fin = torch.isfinite(O.y)
        rs[prefix + k + " special values"] = 0.0 if _same_special(g, O.y) else INF
        err = (g - O.y)[fin].abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, INF), err)
        r = torch.where(err == 0, torch.zeros_like(err), err / O.bound[fin])
        rs[prefix + k + " err/bound"] = float(r.max()) if r.numel() else 0.0
    return rs


def passes(rs):
    return all(v <= 1.0 for v in rs.values())


def vacuity_of(outs, K):
    """max over the unnamed finite elements of bound / ((4 K + 256 + 4 A) e N); must be <= 1"""
    worst = 0.0
    for k, O in outs.items():
        sel = torch.isfinite(O.y) & ~O.named & (O.E > 0)
        if not bool(sel.any()):
            continue
        cap = (4 * K + 256 + 4 * O.A.expand(O.y.shape)[sel]) * E * O.N.expand(O.y.shape)[sel]
        worst = max(worst, float((O.E[sel] / cap).max()))
    return worst


# =====================================================================================================================================
# case table
# =====================================================================================================================================
LSTM_B = (1, 15, 16, 17, 33)
LSTM_SCALES = (1.0, 30.0, 2.0 ** -12)
GAIN = 1.5


def lstm_weights(hs, name="w_hh"):
    g = _gen("%s %d" % (name, hs))
    return (torch.randn(4 * hs, hs, generator=g) * (GAIN / math.sqrt(hs))).to(torch.bfloat16)


def lstm_cases():
    cs = []
    for B in LSTM_B:
        for scale in (LSTM_SCALES if B == 17 else (1.0,)):
            for ragged in ((False, True) if B in (17, 33) else (B % 2 == 1,)):
                kind = "tiny" if scale < 1e-3 else ("saturated" if scale > 1 else "normal")
                cs.append(Case("lstm B%d hs128 x%g%s" % (B, scale, " ragged" if ragged else ""), "lstm", kind, B=B, hs=128,
                               scale=scale, ragged=ragged))
    cs.append(Case("lstm B17 hs256 x1 ragged", "lstm", "normal", B=17, hs=256, scale=1.0, ragged=True))
    return cs


def lstm_inputs(case):
    """x [B, 4hs], h, c fp32, w bf16, lens int32 | None, t.  kind `tiny`: a zero recurrent input and a cell state of the input's size,
    so that both tanh arguments lie in the absolute-error region."""
    g = _gen(case.name)
    B, hs = case.B, case.hs
    x = torch.randn(B, 4 * hs, generator=g) * case.scale
    if case.kind == "saturated":        # every input projection AT +-30 (no further: a gate below 2^-100 would need a floor of its own)
        x = torch.sign(x) * case.scale
        # (input gate, forget gate) saturate as (1, 1), (1, 0) or (0, 1), never (0, 0), and |c| lies in [1/4, 3/4]: c' = f c + i g is
        # then c +- 1, +-1 or c and stays out of tanh's absolute-error region (only kind `tiny` may enter it)
        pat = torch.randint(0, 3, (B, hs), generator=g)
        x[:, :hs] = torch.where(pat == 2, -case.scale, case.scale)
        x[:, hs:2 * hs] = torch.where(pat == 1, -case.scale, case.scale)
    h = torch.randn(B, hs, generator=g) * 0.5
    c = torch.randn(B, hs, generator=g)
    if case.kind == "tiny":
        h = torch.zeros(B, hs)
        c = c * case.scale
    if case.kind == "saturated":
        c = torch.sign(c) * (0.25 + 0.5 * torch.rand(B, hs, generator=g))
    lens, t = None, 0
    if case.ragged:
        t = 2
        lens = torch.tensor([(5, 2, 3, 1, 6)[b % 5] for b in range(B)], dtype=torch.int32)     # rows 1, 3 (mod 5) are inactive at t = 2
    return dict(x=x, h=h, c=c, w=lstm_weights(hs), lens=lens, t=t)


def lstm_active(I):
    return None if I["lens"] is None else (I["t"] < I["lens"].to(torch.int64))


def lstm_bwd_cases():
    cs = []
    for B, hs in [(b, 128) for b in LSTM_B] + [(17, 256)]:
        full = B == 17 and hs == 128
        for tn in (("inside", "outside", "none") if B in (17, 33) else ("inside",)):
            for opt in (("all", "no_d_out", "no_dh_final", "dc_zero", "no_lens") if full else ("all",)):
                if opt == "no_lens" and tn == "outside":
                    continue
                cs.append(Case("lstm_bwd B%d hs%d t_next %s %s" % (B, hs, tn, opt), "lstm_bwd", "normal", B=B, hs=hs, tn=tn, opt=opt))
    return cs


def lstm_bwd_inputs(case):
    """Every input explicit.  lens cycle (5, 2, 3, 1, 6), t = 1 (rows of length 1 are inactive); t_next = 2 lies inside the rows of
    length >= 3 and outside those of length 2 (`inside`: both kinds of row in one call); `outside`: t_next = 7 >= every length;
    `none`: t_next = -1 with dg_next still handed in (it must not be used)."""
    g = _gen(case.name)
    B, hs = case.B, case.hs
    rn = lambda *s: torch.randn(*s, generator=g)
    gates = torch.cat([torch.sigmoid(rn(B, hs)), torch.sigmoid(rn(B, hs)), torch.tanh(rn(B, hs) * 1.5), torch.sigmoid(rn(B, hs))], 1)
    I = dict(dgn=(rn(B, 4 * hs) * 0.3).to(torch.bfloat16), wt=lstm_weights(hs).t().contiguous(), dh_final=rn(B, hs), d_out=rn(B, hs),
             dc=rn(B, hs), svg=gates, svc=rn(B, hs), t=1, t_next={"inside": 2, "outside": 7, "none": -1}[case.tn],
             lens=torch.tensor([(5, 2, 3, 1, 6)[b % 5] for b in range(B)], dtype=torch.int32))
    if case.opt == "no_d_out":
        I["d_out"] = None
    if case.opt == "no_dh_final":
        I["dh_final"] = None
    if case.opt == "dc_zero":
        I["dc"] = torch.zeros(B, hs)
    if case.opt == "no_lens":
        I["lens"] = None
    return I


def to64(I):
    return {k: (v.to(F64) if isinstance(v, torch.Tensor) and v.dtype in (torch.float32, torch.bfloat16) else v) for k, v in I.items()}


# ---- soft-dot ------------------------------------------------------------------------------------------------------------------------
SD_B = 3
MASKS = ("none", "scattered", "first2", "allbut1", "allrow", "poison")
# (path, D, L lengths, offset in floats into the buffer, row stride - D)
SD_SHAPES = (
    [("vec", D, (1, 7, 16, 17), 4, 4) for D in (4, 512, 1024, 2052, 4096)] + [("vec", 512, (80,), 0, 0), ("vec", 4, (1030,), 4, 8)]
    + [("vec2", D, (1, 7, 17), 2, 2) for D in (2, 6, 130, 2058)]
    + [("element", D, (1, 7, 17), 0, 1) for D in (1, 3, 129, 1025, 2055)]
    + [("element", 512, (1, 7, 17), 1, 4), ("element", 130, (1, 7, 17), 2, 1)])
BWD_L = (40, 128, 129, 159, 161)
BWD_MODES = [(prob, g) for prob in (True, False) for g in ("dw", "da", "both")]


def softdot_cases():
    cs = []
    for path, D, Ls, off, pad in SD_SHAPES:
        for L in Ls:
            full = (path, D) in (("vec", 512), ("vec2", 130), ("element", 129)) and L in (7, 17)
            for mk in (MASKS if full else (("scattered",) if L >= 7 and D not in (4096, 2055) else ("none",))):
                if mk in ("first2", "allbut1", "scattered", "poison") and L < 3:
                    continue
                cs.append(Case("softdot %s D%d L%d off%d %s" % (path, D, L, off, mk), "softdot", "normal", path=path, D=D, L=L, off=off,
                               pad=pad, mask=mk, bwd=[(True, "both")]))
    cs.append(Case("softdot vec D4 L17 peaked", "softdot", "peaked", path="vec", D=4, L=17, off=4, pad=4, mask="none", bwd=[(True, "both")]))
    cs.append(Case("softdot vec2 D6 L17 peaked scattered", "softdot", "peaked", path="vec2", D=6, L=17, off=2, pad=2, mask="scattered",
                   bwd=[(False, "both")]))
    # the backward's own shapes: the column walk with one part, and both forms at the chunk edges of the split form
    for path, D, off, pad in (("vec", 1028, 4, 4), ("vec2", 2058, 2, 2)):
        cs.append(Case("softdot %s D%d L40 bwd" % (path, D), "softdot", "normal", path=path, D=D, L=40, off=off, pad=pad, mask="scattered",
                       bwd=[(True, "both"), (False, "da")]))
    for L in BWD_L:
        for path, D, off, pad in (("vec2", 130, 2, 2), ("element", 129, 0, 1)):
            for mk in (("scattered", "allrow", "poison") if L in (129, 161) else ("scattered",)):
                cs.append(Case("softdot %s D%d L%d bwd %s" % (path, D, L, mk), "softdot", "normal", path=path, D=D, L=L, off=off, pad=pad,
                               mask=mk, bwd=BWD_MODES if mk == "scattered" else [(True, "both"), (False, "both")]))
    return cs


class Inputs(object):
    """the tensors of one case (CPU)"""


def softdot_inputs(case):
    """The context is a strided view [B, L, D] of a NaN-filled flat buffer: offset case.off floats, row stride D + case.pad, batch
    stride L row strides + 2 row strides (so: row stride > D and batch stride > L row strides wherever pad > 0)."""
    g = _gen(case.name)
    B, L, D = SD_B, case.L, case.D
    I = Inputs()
    I.rs = D + case.pad
    I.bs = (L + 2) * I.rs if case.pad else L * D
    I.buf = torch.full((case.off + B * I.bs + 8,), float("nan"))
    I.ctx = torch.as_strided(I.buf, (B, L, D), (I.bs, I.rs, 1), case.off)
    I.ctx.copy_(torch.randn(B, L, D, generator=g) * 0.5)
    t = torch.randn(B, D, generator=g) * min(1.0, 4.0 / math.sqrt(D))      # logits of a few units at every width
    if case.kind == "peaked":           # logits spread over about +-60: the smallest probabilities fall below 2^-100
        s = (I.ctx.double() * t.double()[:, None, :]).sum(-1)
        t = t * (60.0 / float(s.abs().max()))
        t = t * torch.tensor([1.0, 0.5, 0.25])[:, None]          # one row spans +-60 (floor elements), the others +-30 and +-15
    I.t = t.float().contiguous()
    mk = torch.zeros(B, L, dtype=torch.bool)
    if case.mask in ("scattered", "poison"):
        mk = torch.rand(B, L, generator=g) < 0.3
        mk[:, L // 2] = False                     # every row keeps a key
        mk[0, L - 1] = True                       # the last key of a row is masked
    elif case.mask == "first2":
        mk[:, :2] = True
    elif case.mask == "allbut1":
        mk[:] = True
        mk[0, 0] = mk[1, L - 1] = mk[2, L // 2] = False
    elif case.mask == "allrow":
        mk = torch.rand(B, L, generator=g) < 0.3
        mk[:, L // 2] = False
        mk[1] = True                              # one all-masked batch row
    I.mask = None if case.mask == "none" else mk
    if case.mask == "poison":
        poison = torch.tensor([INF, float("nan"), -INF])[torch.arange(L * D).view(L, D) % 3]
        I.ctx.copy_(torch.where(mk[:, :, None], poison[None], I.ctx))
    I.dw = torch.randn(B, D, generator=g)
    I.da = torch.randn(B, L, generator=g)
    return I


def softdot_expected_path(case, I):
    return softdot_path(case.D, I.rs, I.bs, case.off)


# ---- skinny linear -------------------------------------------------------------------------------------------------------------------
SK_M = (1, 16, 17)
SK_N = (1, 15, 16, 17, 33)
SK_K = ((32, 0, 32), (64, 64, 128), (5, 6, 32), (1, 0, 32), (130, 3, 160), (128, 128, 288))
SK_FORMS = ("grid", "strided", "off4", "odd")


def skinny_cases():
    cs = []
    n = j = 0
    for K0, K1, Kpad in SK_K:
        for form in SK_FORMS:
            if form == "grid" and (K0 % 4 or K1 % 4):
                continue
            for M in SK_M:
                for N in SK_N:
                    n += 1
                    if (M, N) not in ((17, 33), (1, 1), (16, 16)) and (n % 4):    # the full M x N grid on a quarter of the combinations
                        continue
                    j += 1
                    kind = ("normal", "saturated", "tiny")[j % 3] if (M, N) == (17, 33) else "normal"
                    cs.append(Case("skinny K%d+%d/%d %s M%d N%d %s" % (K0, K1, Kpad, form, M, N, kind), "skinny", kind, K0=K0, K1=K1,
                                   Kpad=Kpad, form=form, M=M, N=N, bias=bool(j % 2), tanh=bool((j // 2) % 2) or kind != "normal"))
    for kind in ("normal", "saturated", "tiny"):
        for form in ("grid", "odd"):
            cs.append(Case("skinny K64+64/128 %s M17 N33 %s tanh" % (form, kind), "skinny", kind, K0=64, K1=64, Kpad=128, form=form, M=17,
                           N=33, bias=kind != "tiny", tanh=True))
    cs.append(Case("skinny K2058+512/2592 strided M17 N33 normal", "skinny", "normal", K0=2058, K1=512, Kpad=2592, form="strided", M=17, N=33,
                   bias=True, tanh=True))
    return cs


def skinny_inputs(case):
    """x0 / x1 are views of NaN-filled buffers: grid: row stride K + 4, offset 4 floats; strided: K + 2 (even), offset 2; off4: offset 1;
    odd: stride K + 1 | 1.  NaN sits just outside [0, K) of every row.  w_pad bf16 [N, Kpad] zero past K0 + K1 with a row stride of
    Kpad + 8."""
    g = _gen(case.name)
    M, N, K0, K1, Kpad = case.M, case.N, case.K0, case.K1, case.Kpad
    scale = {"normal": 1.0, "saturated": 30.0, "tiny": 2.0 ** -12}[case.kind]
    I = Inputs()

    def view(K, salt):
        stride, off = {"grid": (K + 4, 4), "strided": (K + 2, 2), "off4": (K + 3, 1), "odd": ((K + 1) | 1, 3 + salt)}[case.form]
        buf = torch.full((off + M * stride + 8,), float("nan"))
        v = torch.as_strided(buf, (M, K), (stride, 1), off)
        r = torch.randn(M, K, generator=g).clamp(-3, 3)
        if K0 + K1 < 8 and case.kind != "tiny":     # a row of one or two products: keep |z| out of tanh's absolute-error region (only kind `tiny` may enter it)
            r = torch.sign(r) * (0.5 + r.abs())
        v.copy_((torch.sign(r) if case.kind == "saturated" else r) * scale)
        return buf, v

    I.buf0, I.x0 = view(K0, 0)
    I.buf1, I.x1 = view(K1, 1) if K1 else (None, None)
    K = K0 + K1
    wstd = 1.0 / math.sqrt(K) if case.kind != "tiny" else 0.25 / K      # tiny: |z| <= 9/4 2^-12 < 2^-10 in every element
    I.wbuf = torch.zeros((N, Kpad + 8), dtype=torch.bfloat16)
    wr = torch.randn(N, K, generator=g).clamp(-3, 3)
    if K < 8 and case.kind != "tiny":
        wr = torch.sign(wr) * (0.5 + wr.abs())
    I.wbuf[:, :K] = (wr * wstd).to(torch.bfloat16)
    I.w = I.wbuf[:, :Kpad]
    I.bias = (torch.randn(N, generator=g) * (scale if case.kind != "tiny" else 0.0)) if case.bias else None
    if case.kind == "tiny":
        I.bias = None
    return I


def skinny_is_grid(case):
    return case.form == "grid"


_CASES = {}


def cases(op):
    if op not in _CASES:
        _CASES[op] = {"lstm": lstm_cases, "lstm_bwd": lstm_bwd_cases, "softdot": softdot_cases, "skinny": skinny_cases}[op]()
    return _CASES[op]


def all_cases():
    return [c for op in ("lstm", "lstm_bwd", "softdot", "skinny") for c in cases(op)]


def reduction_length(case):
    """K of the vacuity cap"""
    if case.op == "lstm":
        return case.hs
    if case.op == "lstm_bwd":
        return 4 * case.hs
    if case.op == "softdot":
        return case.D + case.L
    return case.K0 + case.K1


_TERMS = {}


def case_terms(case, sub=None):
    """-> ({output: Out}, values) of a case's float64 reference.  softdot: sub = None (forward) or (prob, "dw" | "da" | "both")."""
    key = (case.name, sub)
    if key in _TERMS:
        return _TERMS[key]
    if case.op == "lstm":
        I = lstm_inputs(case)
        r = lstm_terms(I["x"].double(), I["h"].double(), I["c"].double(), I["w"].double(), lstm_active(I), tiny=case.kind == "tiny")
    elif case.op == "lstm_bwd":
        r = lstm_bwd_terms(to64(lstm_bwd_inputs(case)))
    elif case.op == "softdot":
        I = softdot_inputs(case)
        dw = da = None
        prob = True
        if sub is not None:
            prob, g = sub
            dw = I.dw.double() if g in ("dw", "both") else None
            da = I.da.double() if g in ("da", "both") else None
        r = softdot_terms(I.ctx.double(), I.t.double(), I.mask, dw, da, prob, peaked=case.kind == "peaked")
    else:
        I = skinny_inputs(case)
        K = case.K0 + case.K1
        r = skinny_terms(I.x0.double(), None if I.x1 is None else I.x1.double(), I.w[:, :K].double(),
                         None if I.bias is None else I.bias.double(), case.tanh, tiny=case.kind == "tiny")
    if len(_TERMS) > 64:
        _TERMS.clear()
    _TERMS[key] = r
    return r


def subs(case):
    return [None] + list(case.bwd) if case.op == "softdot" else [None]


def vacuity(case):
    """the largest bound / cap over the unnamed elements of every output (and every backward mode) of the case; must be <= 1"""
    return max(vacuity_of(case_terms(case, s)[0], reduction_length(case)) for s in subs(case))


# =====================================================================================================================================
# the minimal implementation and the mutants: float64, every output rounded once
# =====================================================================================================================================
MUTANTS = collections.OrderedDict([
    ("gate_order_igfo", ("lstm",)), ("h_prev_truncated", ("lstm", "skinny")), ("h_prev_left_in_fp32", ("lstm", "skinny")),
    ("k_quarter_dropped", ("lstm",)), ("c_from_new_c", ("lstm",)), ("inactive_state_updated", ("lstm",)),
    ("inactive_output_nonzero", ("lstm",)), ("tanh_small_argument_series", ("lstm", "skinny")),
    ("mask_applied_after_the_softmax", ("softdot",)), ("masked_keys_inf_multiplied_in", ("softdot",)),
    ("last_2_columns_of_a_D%4==2_row_dropped", ("softdot",)), ("last_key_part_dropped", ("softdot",)),
    ("key_L-1_dropped_when_L%16!=0", ("softdot",)), ("d_attn_on_the_wrong_side_of_the_softmax", ("softdot",)),
    ("d_attn_given_to_masked_keys_in_logit_mode", ("softdot",)), ("sum_p_dp_without_d_attn", ("softdot",)),
    ("one_chunk_of_the_split_d_target_dropped", ("softdot",)), ("x0_x1_seam_off_by_one", ("skinny",)),
    ("bias_skipped_for_the_last_N%16_columns", ("skinny",)), ("dh_final_where_dg_next_should_be", ("lstm_bwd",)),
    ("dh_final_missing_at_a_rows_last_position", ("lstm_bwd",)), ("df_with_new_c", ("lstm_bwd",)),
    ("dc_not_multiplied_by_f", ("lstm_bwd",))])


def r32(x):
    return x.to(torch.float32).to(F64)


def model(case, sub=None, mut=None):
    """{output: float64 tensor} of the minimal implementation (or a mutant of it): the reference's formulas, every output rounded once"""
    if case.op == "lstm":
        I = lstm_inputs(case)
        V = lstm_values(I["x"].double(), I["h"].double(), I["c"].double(), I["w"].double(), lstm_active(I), mut)
        return {k: r32(V[k]) for k in ("h_out", "c_out", "seq_out", "sv_g")}
    if case.op == "lstm_bwd":
        V = lstm_bwd_values(to64(lstm_bwd_inputs(case)), mut)
        return {"dg32": r32(V["d"]), "dg16": bf16r(V["d"]), "dc": r32(V["dc_out"])}
    if case.op == "softdot":
        I = softdot_inputs(case)
        if sub is None:
            V = softdot_values(I.ctx.double(), I.t.double(), I.mask, mut=mut)
            return {k: r32(V[k]) for k in ("logit", "p", "weighted")}
        prob, g = sub
        V = softdot_values(I.ctx.double(), I.t.double(), I.mask, I.dw.double() if g in ("dw", "both") else None,
                           I.da.double() if g in ("da", "both") else None, prob, mut)
        return {k: r32(V[k]) for k in ("d_target", "d_context")}
    I = skinny_inputs(case)
    K = case.K0 + case.K1
    V = skinny_values(I.x0.double(), None if I.x1 is None else I.x1.double(), I.w[:, :K].double(),
                      None if I.bias is None else I.bias.double(), case.tanh, mut)
    return {"out": r32(V["out"])}


# =====================================================================================================================================
# float32 emulations: four summation orders, __expf and rcp one ulp either way
# =====================================================================================================================================
ORDERS = ("sequential", "reverse", "pairwise", "kernel")


def _fold(t):
    """the 64-lane xor butterfly as lane 0 sees it: halves folded onto each other"""
    w = t.shape[-1]
    while w > 1:
        w //= 2
        t = (t[..., :w] + t[..., w:2 * w]).astype(F32)
    return t[..., 0]


def sum32(a, order, lanes=64, width=1, waves=1):
    """float32 sum over the last axis.  kernel: lane-strided partial sums (a lane owns `width` consecutive elements every lanes * width),
    the 64-lane butterfly (lanes > 64: one butterfly per wave of a lanes-thread workgroup, then the 16 or 4 wave partials in turn); waves > 1: the axis is first cut into `waves` contiguous quarters (the MFMA kernels' K split), each
    summed in sequence, and the quarters are added in turn."""
    a = np.ascontiguousarray(a, dtype=F32)
    n = a.shape[-1]
    if order == "sequential":
        return np.cumsum(a, axis=-1, dtype=F32)[..., -1]
    if order == "reverse":
        return np.cumsum(a[..., ::-1], axis=-1, dtype=F32)[..., -1]
    if order == "pairwise":
        m = 1 << max(0, (n - 1).bit_length())
        full = np.zeros(a.shape[:-1] + (m,), dtype=F32)
        full[..., :n] = a
        while full.shape[-1] > 1:
            full = (full[..., 0::2] + full[..., 1::2]).astype(F32)
        return full[..., 0]
    if waves > 1:
        q = (n + waves - 1) // waves
        tot = np.zeros(a.shape[:-1], dtype=F32)
        for w_ in range(waves):
            tot = (tot + sum32(a[..., w_ * q:(w_ + 1) * q], "sequential")).astype(F32) if a[..., w_ * q:(w_ + 1) * q].shape[-1] else tot
        return tot
    step = lanes * width
    m = (n + step - 1) // step * step
    full = np.zeros(a.shape[:-1] + (m,), dtype=F32)
    full[..., :n] = a
    full = full.reshape(a.shape[:-1] + (m // step, lanes, width))
    per_lane = np.cumsum(full.transpose(*range(len(a.shape) - 1), -2, -3, -1).reshape(a.shape[:-1] + (lanes, -1)), axis=-1, dtype=F32)[..., -1]
    if lanes > 64:      # a workgroup of lanes / 64 waves: the butterfly inside each wave, then the wave partials in turn
        return np.cumsum(_fold(per_lane.reshape(a.shape[:-1] + (lanes // 64, 64))), axis=-1, dtype=F32)[..., -1]
    return _fold(per_lane)


def _ulp(x, k):
    x = x.astype(F32)
    if k == 0:
        return x
    return np.nextafter(x, F32(np.inf if k > 0 else -np.inf)).astype(F32)


def sig32(x, k):
    with np.errstate(over="ignore"):
        return _ulp(F32(1) / (F32(1) + _ulp(expf32(-x), k)).astype(F32), -k)


def tanh32(x, k):
    e = _ulp(expf32((F32(-2) * np.abs(x)).astype(F32)), k)
    return np.copysign(((F32(1) - e).astype(F32) * _ulp(F32(1) / (F32(1) + e).astype(F32), k)).astype(F32), x).astype(F32)


def _np(t):
    return t.detach().to(torch.float32).numpy()


def emulation(case, order, k, sub=None):
    """{output: float64 tensor} of a float32 implementation of the case's operation: every operation rounded to float32, sums in
    `order`, __expf / rcp results moved k ulps (k = -1, 0, 1)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(F64)
    if case.op == "lstm":
        I = lstm_inputs(case)
        hs = case.hs
        hq = _np(I["h"].to(torch.bfloat16))
        P = hq[:, None, :] * _np(I["w"])[None, :, :]                       # exact in float32
        z = (_np(I["x"]) + sum32(P, order, waves=4)).astype(F32)
        i, f, g, o = sig32(z[:, :hs], k), sig32(z[:, hs:2 * hs], k), tanh32(z[:, 2 * hs:3 * hs], k), sig32(z[:, 3 * hs:], k)
        c, h = _np(I["c"]), _np(I["h"])
        cn = ((f * c).astype(F32) + (i * g).astype(F32)).astype(F32)
        hn = (o * tanh32(cn, k)).astype(F32)
        act = lstm_active(I)
        a2 = np.ones((case.B, 1), dtype=bool) if act is None else act.numpy()[:, None]
        return {"h_out": T(np.where(a2, hn, h)), "c_out": T(np.where(a2, cn, c)), "seq_out": T(np.where(a2, hn, F32(0))),
                "sv_g": T(np.concatenate([i, f, g, o], 1))}
    if case.op == "lstm_bwd":
        I = lstm_bwd_inputs(case)
        V = lstm_bwd_values(to64(I))
        hs = case.hs
        P = _np(I["dgn"])[:, None, :] * _np(I["wt"])[None, :, :]
        prod = sum32(P, order, waves=4)
        fin = np.zeros_like(prod) if I["dh_final"] is None else _np(I["dh_final"])
        dh = np.where(V["use"].numpy(), prod, fin)
        if I["d_out"] is not None:
            dh = (dh + _np(I["d_out"])).astype(F32)
        i, f, g, o = (_np(x) for x in I["svg"].split(hs, 1))
        cp = _np(I["svc"])
        tc = tanh32(((f * cp).astype(F32) + (i * g).astype(F32)).astype(F32), k)
        m = lambda *xs: functools.reduce(lambda a, b: (a * b).astype(F32), xs)
        dc = (_np(I["dc"]) + m(dh, o, (F32(1) - (tc * tc).astype(F32)).astype(F32))).astype(F32)
        d = np.concatenate([m(dc, g, i, (F32(1) - i).astype(F32)), m(dc, cp, f, (F32(1) - f).astype(F32)),
                            m(dc, i, (F32(1) - (g * g).astype(F32)).astype(F32)), m(dh, tc, o, (F32(1) - o).astype(F32))], 1)
        act = V["act"].numpy()
        d = np.where(act, d, F32(0))
        return {"dg32": T(d), "dg16": bf16r(T(d)), "dc": T(np.where(act, m(dc, f), _np(I["dc"])))}
    if case.op == "skinny":
        I = skinny_inputs(case)
        K = case.K0 + case.K1
        x = I.x0 if I.x1 is None else torch.cat([I.x0, I.x1], 1)
        P = _np(x.to(torch.bfloat16))[:, None, :] * _np(I.w[:, :K])[None, :, :]
        z = sum32(P, order, waves=4)
        if I.bias is not None:
            z = (z + _np(I.bias)[None, :]).astype(F32)
        return {"out": T(tanh32(z, k) if case.tanh else z)}
    I = softdot_inputs(case)
    B, L, D = I.ctx.shape
    mk = np.zeros((B, L), dtype=bool) if I.mask is None else I.mask.numpy()
    c = np.where(mk[:, :, None], F32(0), _np(I.ctx))
    t = _np(I.t)
    width = {"vec": 4, "vec2": 4, "element": 1}[softdot_expected_path(case, I)] if sub is None else (2 if D % 4 == 2 else 1)
    with np.errstate(invalid="ignore", over="ignore"):
        s = sum32((c * t[:, None, :]).astype(F32), order, 64, width)
        s = np.where(mk, F32(-np.inf), s)
        mx = s.max(1, keepdims=True)
        ex = _ulp(expf32((s - mx).astype(F32)), k)
        ex = np.where(mk & ~np.isnan(ex), F32(0), ex)       # every key masked: -inf - -inf = NaN in the whole row
        zs = sum32(ex, order, SD_THREADS, 1)[:, None]             # 16 wave partials
        p = (ex * _ulp(F32(1) / zs, -k)).astype(F32)
        parts = sd_parts((D + 3) // 4 if width == 4 else D, L)
        pc = (p[:, :, None] * c).astype(F32).transpose(0, 2, 1)                         # [B, D, L]
        if sub is None:
            if order == "kernel":        # every parts-th key, the parts in turn
                w = np.zeros((B, D), dtype=F32)
                for q in range(parts):
                    w = (w + sum32(pc[:, :, q::parts], "sequential")).astype(F32)
            else:
                w = sum32(pc, order)
            return {"logit": T(s), "p": T(p), "weighted": T(w)}
        prob, gsel = sub
        zl = np.zeros((B, L), dtype=F32)
        q0 = sum32((c * _np(I.dw)[:, None, :]).astype(F32), order, 64, width) if gsel in ("dw", "both") else zl
        dA = _np(I.da) if gsel in ("da", "both") else zl
        dp = np.where(mk, F32(0), (q0 + dA).astype(F32) if prob else q0)
        Pd = sum32((p * dp).astype(F32), order, SD_THREADS, 1)[:, None]
        dl = (p * (dp - Pd).astype(F32)).astype(F32)
        if not prob:
            dl = np.where(mk, dl, (dl + dA).astype(F32))
        gc = (dl[:, :, None] * c).astype(F32).transpose(0, 2, 1)
        if order == "kernel":            # the two-launch form: chunks of 32 keys in sequence, the chunks added by the caller
            dt = np.zeros((B, D), dtype=F32)
            for q in range(0, L, SDB_KEYS):
                dt = (dt + sum32(gc[:, :, q:q + SDB_KEYS], "sequential")).astype(F32)
        else:
            dt = sum32(gc, order)
        dw = _np(I.dw) if gsel in ("dw", "both") else np.zeros((B, D), dtype=F32)
        dcx = ((p[:, :, None] * dw[:, None, :]).astype(F32) + (dl[:, :, None] * t[:, None, :]).astype(F32)).astype(F32)
        return {"d_target": T(dt), "d_context": T(dcx)}
