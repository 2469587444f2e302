"""fp64 references, CPU models and derived per-element error bounds for the loss heads of csrc/loss_heads.hip:
ce_softmax_rows (two passes, online rescaled), ce_softmax_rows_reg<8|32> (row in registers), ce_double_softmax_rows and
action_head_rows, each with bf16 and fp32 gradient rows.

Everything here is plain numpy / torch on the CPU.  tests/test_host_loss_reference.py proves, without a GPU, that the bounds accept
the minimal implementation (float64, every output rounded once) and float32 emulations in four summation orders, never go vacuous
outside the elements a case names, and reject a table of subtly wrong implementations; tests/test_gpu_loss_conformance.py holds
the HIP kernels to the same bounds.  No bound below was chosen by looking at a kernel's output.

NOTATION  e = 2^-24 (fp32 unit round-off), u = the output's unit round-off (helpers_gemm.U_OUT), z the fp32 logits of one row taken as
exact, y its label, V its width.  Every quantity on the right of a bound is the float64 reference's own.  The model of
__expf(x) is helpers_attention's: the argument rounding and the log2(e) multiply give a relative error of about 2 |x| e, v_exp_f32
adds one ulp, and below a result of 2^-100 (denormal results, flushing) only an absolute floor is promised.

SINGLE SOFTMAX (ce_reference)   lse = m + log s, m = max z, s = sum exp(z - m), p = exp(z - lse), loss = lse - z_y,
dz = scale (p - onehot), amax = the first index of max z.

    R_j   = m - z_j
    a_j   = (2 R_j + 4) e                    exp(z_j - m): the subtraction (e R_j on the argument = relative in the result), __expf
                                             (2 R_j e + 1 ulp), two to spare
    rs    = (V + 2) e + sum_j p_j a_j        relative error of s: V - 1 additions in ANY order move a sum of positive terms by at
                                             most (V - 1) e relatively; the terms' own errors enter weighted by p_j
            + (2 (m - min z) + 4 L) e        two-pass kernel only: every online step and merge multiplies the running sum by
                                             exp(m_old - m_new); along one chain the arguments telescope to at most m - min z
                                             (2 e per unit, as __expf's), and each of the L = 4 ceil(V / 1024) + 9 steps of a chain
                                             (per-thread elements, 6 lane merges, 3 wave merges) rounds twice more: 4 L e
    dlse  = rs + 3 e |log s| + e |lse|       __logf = v_log_f32 times ln 2 (3 e relative), the final m + log s
    |loss_got - loss| <= dlse + e |loss|     (the subtraction lse - z_y)
    rp_j  = dlse + (3 |z_j - lse| + 6) e     relative error of p_j: through lse, or through s and 1 / s, and one more __expf
    E_j   = |scale| (p_j rp_j + 2 e (p_j + onehot_j))  +  |scale| 2^-100 where p_j < 2^-100
    |dz_got - dz_j| <= u |dz_j| + (1 + u) E_j

  2 e (p + onehot) is the subtraction of the one-hot and the multiply by scale (or the multiply and the subtraction: the register
  kernels form p scale / s - scale).  The floor is carried only by the elements below 2^-100: with |scale| >= 2^-20 (asserted by
  the case table) an element above it is a normal fp32 number at every stage, and the relative argument holds for it.  (Adding
  the floor to every element would be looser, and would make the vacuity cap below fail for p_j between 2^-100 and about 2^-76.)

DOUBLE SOFTMAX (double_reference)   p = softmax(z), q = softmax(p), T = sum_i q_i p_i, loss = log s2 - p_y with s2 = sum exp(p),
D_j = q_j - onehot_j - (T - p_y), dz_j = scale p_j D_j, amax = the first index of max z (the kernel's contract; never the argmax
of rounded probabilities).  V <= 2048.

    rp_j  = a_j + rs + 2 e                   p_j = exp(z_j - m) (1 / s): a_j and rs as above, the reciprocal and the multiply
    re_j  = p_j rp_j + (2 p_j + 2) e         exp(p_j): the argument's absolute error p_j rp_j is relative in the result, __expf
    rs2   = (V + 2) e + sum_j q_j re_j       s2, any order
    rt    = (V + 2) e + sum_j (q_j p_j / T) (re_j + rp_j + e)        t = sum exp(p_j) p_j, any order (all terms positive)
    |loss_got - loss| <= rs2 + 3 e |log s2| + p_y rp_y + e |loss| + 2^-100
    dD_j  = q_j (re_j + 2 e) + T (rt + 2 e) + (1 + 2^-10) |q_j - T| rs2 + p_y rp_y + e (|q_j - onehot_j| + |T - p_y| + |D_j|)
            (q_j and T are divided by the SAME computed s2: its error moves their difference relatively, not each of them)
    E_j   = |scale| p_j (dD_j + |D_j| (rp_j + 2 e))  +  |scale| 2^-100 where p_j < 2^-100

  q_j - onehot_j - (T - p_y) CANCELS (for a spread-out row q_j and T are both about 1 / V): its absolute error is what the lines
  above add up, a few e -- and V e from the two sums -- times q_j + onehot_j + T + p_y, and nothing relative to D_j can be promised.

ACTION HEAD (action_reference)   as the kernel's comment states: l = log_softmax(z), m = log_softmax(l), loss = -sum_valid m_y /
n_valid, accuracy = #(argmax l == y) / B over all B rows, dz = g - exp(l) rowsum(g), g = (exp(m) - onehot) valid grad_scale /
n_valid, ignore_index = -1.  Mathematically m = l and rowsum(g) = 0.  w = grad_scale / n_valid, p = exp(l), A <= 64.

    i_j   = (R_j + |l_j|) e                    the roundings of l_j = (z_j - max) - log s that are the column's own; the error of
                                               log s is COMMON to the row's columns and a log-softmax ignores a common shift of
                                               its input: it never reaches m
    C     = sum_i p_i i_i + rs + 3 e |log s|   the error common to the columns of m: the log-sum-exp of the computed l (the columns'
                                               own errors weighted by p), the second sum (rs over A columns) and its logarithm
    dm_j  = 2 i_j + C                          (l_j's own error and the same roundings once more)
    ri_j  = 2 i_j + (2 |l_j| + 2) e            relative error of exp(m_j) that is the column's own
    dg_j  = |w| (p_j ri_j + 4 e (p_j + onehot_j))      ... of g_j: the one-hot subtraction, 1 / n_valid, two multiplies
    G     = sum_j dg_j + (A + 2) e sum_j |g_j|         |rowsum(g)| less the common part: the exact sum is 0, so what the kernel adds up
                                                       is w C (the common relative error C on every exp(m_j), times sum p = 1), the
                                                       columns' own errors and the summation's rounding
    E_j   = dg_j + (1 + 2^-10) p_j (G + 2^-10 |w| C) + e |g_j|  +  |w| 2^-100 where p_j < 2^-100
            the common error w p_j C of g_j is taken out again by the correction exp(l_j) rowsum(g) = p_j (w C + ...): that is
            what the correction is for; what is left of it is second order (the relative error of exp(l_j), below 2^-10, times w C)
    |loss_got - loss| <= mean_valid dm_y + (B + 2) e mean_valid |m_y| + e |loss|      (two-level sum over the rows, times 1 / n)
    accuracy == float32(hits) / float32(B) exactly; an ignored row's gradient is exactly 0 whatever n_valid is; n_valid = 0 gives a
    NaN loss (torch's 0 / 0) and, as torch's nll_loss backward writes only the rows that are not ignored, a gradient of exact zeros.

  A kernel that DROPPED the correction would be left with the common error w p_j C, with C <= (A + 2 + 3 |log s| + ...) e in the
  worst case but a few e in any actual run (the roundings of two 64-term sums): that is below dg_j + p_j G, so the mutant
  "rowsum(g) correction dropped" is not detectable by a bound derived from fp32 arithmetic, and is not in the table.
  argmax: l is a rounded function of z, so two different logits closer than an ulp of l could tie in l.  The action head's
  logits are therefore drawn on a grid of 2^-10: columns tie exactly (then l ties bit for bit: the same operations on the same
  values) or differ by far more than l's resolution, and "first index of max z" is the contract.

VACUITY (vacuity)  From the reference alone, E_j <= (2 V + 256 + 4 max|z|) e N_j for every element a case does not name (A in place
of V for the action head), where N_j is the magnitude the element is made of:
  single softmax   N_j = |dz_j| in every column.  Named: the label column of a row the case declares saturated (1 - p_y < 2^-10:
                   dz_y -> 0 and only the absolute e |scale| term is left; at most one per row, only kind `confident` and widths
                   up to 9 may hold them) and the elements with p_j < 2^-100 (floor only; only kinds `wide` / `wide12`, at most half
                   of a row).
  action head      N_j = |dz_j| in every column but the label's, N_y = |w| there.  dz_y = -w (1 - p_y) is a difference of p_y and 1
                   and E_y holds the absolute terms |w| (p_y ri_y + 4 e (p_y + 1)) and p_y G (the rounding of a row sum whose terms
                   are of size |w|): against |dz_y| itself the cap would need 1 - p_y >= about (8 A + 4 R + ...) / (2 A + 256), which
                   rows of 2 or 7 columns drawn N(0, 3) do not give (the cap as written fails there by up to 64 times at A = 2).
                   A row with 1 - p_y < 2^-10 is the far end of the same cancellation.  Nothing is named but floor elements.
  double softmax   N_j = |scale| p_j (q_j + onehot_j + T + p_y): D_j cancels in every column (above).  Its cap is
                   (7 V + 256 + 4 max|z|) e: dD_j / N_j <= rt + rs2 + rp_y + 5 e and |D_j| (rp_j + 2 e) / N_j <= rp_j + 2 e;
                   rt <= (V + 2) e + 2 max rp + 5 e (exp(p_i) p_i carries the error of p_i twice, once through the exponential:
                   for a row with one p_i near 1 that is the whole of it), rs2 <= (V + 2) e + max rp + 4 e, and every rp holds
                   rs = (V + 2) e + ...: seven times V e.  Nothing is named but floor elements.
Every element, named or not, is held to its bound and to finiteness.

A LIMIT, STATED  The any-order term V e is about 2^-9 at V = 32k: the fp32-gradient bound at production width is only about twice as
tight as bf16 round-off.  The precision mutants of the g32 instantiations are therefore shown rejected at V <= 2048 (V e <= 2^-13).

INPUT KINDS (random_logits)  normal N(0, 3); offset = normal + 1000; wide N(0, 30); wide12 N(0, 12) (N(0, 30) puts more than half
of a row of 97 columns or more below 2^-100, which the vacuity rule forbids: `wide` itself runs at V = 8 and the longer rows get
their underflowing tail from this one); confident = normal with +40 on the label (the label's own logit capped at 9, so it
stays below the padding's 50); bf16grid = normal rounded to bf16, so ties occur naturally.  Input buffers are [rows, ldz] with
ldz > V and +50.0 in the columns [V, ldz); outputs live in SENTINEL-filled buffers [rows + 1, lddz] with lddz > Vpad.
"""
import math
import zlib

import numpy as np
import torch

import helpers_gemm as hg
from helpers_gemm import U_OUT, Ref, assert_ratios, passes, ratios, round_out, signed_stat  # noqa: F401

F64 = torch.float64
E32 = 2.0 ** -24
FLOOR = 2.0 ** -100
SENTINEL = 12345.0
PAD_IN = 50.0
INF = float("inf")
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
FMTS = ("bf16", "f32")
ORDERS = ("sequential", "pairwise", "lanes", "online")
KINDS = ("normal", "offset", "wide", "wide12", "confident", "bf16grid")
STD = {"normal": 3.0, "offset": 3.0, "wide": 30.0, "wide12": 12.0, "confident": 3.0, "bf16grid": 3.0}


def round_up(n, k):
    return (n + k - 1) // k * k


def ce_dispatch(Vpad):
    """the kernel ce_softmax_launch picks (csrc/loss_heads.hip): by the padded width"""
    need = (Vpad + 1023) // 1024
    return "ce_softmax_rows_reg<8>" if need <= 8 else "ce_softmax_rows_reg<32>" if need <= 32 else "ce_softmax_rows"


class Case(object):
    """One problem: head in ce / double / action; kind an input kind or onehot / uniform / ties."""

    def __init__(self, head, kind, rows, V, Vpad=None, ldz=None, lddz=None, scale=None, i=0, why="", **p):
        self.head, self.kind, self.rows, self.V, self.i, self.why, self.p = head, kind, rows, V, i, why, p
        if head == "action":
            self.Vpad = round_up(V, 8) if Vpad is None else Vpad
            self.ldz = V + 3 if ldz is None else ldz
            self.lddz = self.Vpad + 5 if lddz is None else lddz
            self.scale = 0.5 if scale is None else scale
            self.reaches = "action_head_rows"
        else:
            self.Vpad = round_up(V, 8) if Vpad is None else Vpad
            self.ldz = round_up(V, 4) + 4 if ldz is None else ldz
            self.lddz = self.Vpad + 8 if lddz is None else lddz
            self.scale = 2.0 ** -7 if scale is None else scale
            self.reaches = ce_dispatch(self.Vpad) if head == "ce" else "ce_double_softmax_rows"
        self.two_pass = self.reaches == "ce_softmax_rows"
        self.name = "%s %s rows=%d V=%d Vpad=%d #%d" % (head, kind, rows, V, self.Vpad, i)

    def __repr__(self):
        return self.name


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def random_logits(kind, rows, V, seed):
    """fp32 [rows, V] and int64 labels [rows] (a label is needed by `confident`)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((rows, V), generator=g, dtype=torch.float64) * STD[kind]
    y = torch.randint(0, V, (rows,), generator=g)
    if kind == "offset":
        z = z + 1000.0
    if kind == "confident":
        z[torch.arange(rows), y] = z[torch.arange(rows), y].clamp(max=9.0) + 40.0        # (below the +50 of the padding)
    z = z.to(torch.float32)
    if kind == "bf16grid":
        z = z.to(torch.bfloat16).to(torch.float32)
    return z, y


ONEHOT_POSITIONS = (0, 3, 4, 7, 8, 255, 256, 1023, 1024, 1027, 2047, 2048, 8191)


def onehot_positions(V):
    """every structural position of the one-hot sweep inside [0, V): vector, wave, chunk and kernel seams, V - 1 and the tail group
    of V % 4 != 0"""
    pos = [c for c in ONEHOT_POSITIONS if c < V] + [V - 1]
    if V % 4:
        pos += list(range(V - V % 4, V))
    return sorted(set(pos))


CE_TIES = ((5, 6), (2, 9), (255, 256), (8, 1030), (1030, 2050), (700, 1027, 2049), (3, 1024), (1023, 1024, 2047))
DOUBLE_TIES = ((7, 8), (511, 512), (2040, 2047), (3, 5), (8, 1030), (255, 256, 2047))


def tie_sets(case):
    if case.head == "ce":
        sets = [t for t in CE_TIES if t[-1] < case.V]
        if case.V > 8200:
            sets += [(8191, case.V - 1), (2050, 8192), (case.V - 2, case.V - 1)]
        return sets
    if case.head == "double":
        return [t for t in DOUBLE_TIES if t[-1] < case.V]
    A = case.V
    return sorted(set(tuple(sorted(set(t))) for t in ((0, 1), (0, A - 1), (1, A - 1), (0, 1, A - 1)) if len(set(t)) > 1 and max(t) < A))


class Inputs(object):
    pass


_INPUTS = {}


def inputs(case):
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    I = Inputs()
    V, seed = case.V, _seed(case.name)
    if case.kind == "onehot":
        # one column 0, every other -200: exp(-200) = 1.4e-87 is below fp32's smallest denormal (1.4e-45), so __expf returns exactly
        # 0, s = 1 (1 + 0 + ... and integer counts of exp(0) times 0 in the online merges), log 1 = 0, lse = m = 0 EXACTLY; scale is
        # a power of two: loss is 0 or 200, dz is 0, +scale (the hot column of a row labelled elsewhere) or -scale (its label)
        pos = onehot_positions(V)
        hot = torch.tensor([c for c in pos for _ in (0, 1)])
        other = torch.tensor([pos[(k + 1) % len(pos)] for k in range(len(pos))])
        y = hot.clone()
        y[1::2] = other
        z = torch.full((len(hot), V), -200.0, dtype=torch.float32)
        z[torch.arange(len(hot)), hot] = 0.0
        I.hot = hot
    elif case.kind == "uniform":
        # all columns 0.5, V = 2^k: exp(0) = 1, s = V (a sum of ones, exact in any order), scale / V a power of two:
        # dz = scale (1 / V - onehot) with V - 1 < 2^24, one rounding to the output format
        z = torch.full((case.rows, V), 0.5, dtype=torch.float32)
        y = torch.tensor([(r * 389 + V - 1) % V for r in range(case.rows)])
    elif case.kind == "ties":
        sets = tie_sets(case)
        z, y = random_logits("bf16grid", len(sets), V, seed)
        if case.head == "action":
            z = (z * 1024.0).round() / 1024.0
        z = z.clamp(max=20.0)
        for r, cols in enumerate(sets):
            z[r, list(cols)] = 24.0
        I.tie_first = torch.tensor([min(c) for c in sets])
    else:
        z, y = random_logits(case.kind, case.rows, V, seed)
        if case.head == "action":
            z = (z.to(F64) * 1024.0).round().div(1024.0).to(torch.float32)      # the 2^-10 grid (module docstring)
    if case.head == "action":
        n_ign, B = case.p.get("ignored", 0), z.shape[0]
        ign = torch.zeros(B, dtype=torch.bool)
        if n_ign >= B:
            ign[:] = True
        elif n_ign == 1:
            ign[B // 2] = True
        elif n_ign:
            assert n_ign == B - 1
            ign[:] = True
            ign[B // 3] = False
        y = torch.where(ign, torch.full_like(y, -1), y)
        if n_ign:
            # the first ignored row has its maximum at column 0: a kernel comparing the argmax with the CLAMPED label would count a hit
            r = int(torch.nonzero(ign)[0])
            z[r, 0] = z[r].max() + 0.5
    I.z, I.y = z.contiguous(), y.to(torch.int64)
    I.rows = z.shape[0]
    zbuf = torch.full((I.rows, case.ldz), PAD_IN, dtype=torch.float32)
    zbuf[:, :V] = z
    I.zbuf = zbuf
    _INPUTS[case.name] = I
    return I


# ---- references --------------------------------------------------------------------------------------------------------------------
class Terms(object):
    """the reference of one case for one output format: loss / dz Refs, amax, E (the fp32 part of dz's bound), named, floor, N"""


def _first_argmax(z):
    return torch.from_numpy(np.argmax(z.numpy(), axis=1).astype(np.int64))          # numpy: the first occurrence


def _softmax_terms(z):
    V = z.shape[1]
    m = z.max(1, keepdim=True).values
    R = m - z
    s = torch.exp(-R).sum(1, keepdim=True)
    lse = m + torch.log(s)
    p = torch.exp(z - lse)
    a = (2.0 * R + 4.0) * E32
    rs = (V + 2) * E32 + (p * a).sum(1, keepdim=True)
    return m, R, s, lse, p, a, rs


def _onehot(y, V):
    oh = torch.zeros((y.shape[0], V), dtype=F64)
    ok = y >= 0
    oh[torch.arange(y.shape[0])[ok], y[ok]] = 1.0
    return oh


def _others(p, oh):
    """1 - p_y as the sum of the other columns (no cancellation)"""
    return (p * (1.0 - oh)).sum(1)


_REFS = {}


def reference(case, fmt):
    key = (case.name, fmt)
    if key not in _REFS:
        _REFS[key] = {"ce": ce_reference, "double": double_reference, "action": action_reference}[case.head](case, fmt)
    return _REFS[key]


def _finish(T, case, fmt, loss, loss_bound, dz, E, N, p, oh, z):
    u = U_OUT[fmt]
    exact = case.kind == "onehot" or (case.kind == "uniform")
    T.loss = Ref(loss, loss_bound, "f32")
    T.E = E
    T.dz = Ref(dz, u * dz.abs() + (1.0 + u) * E, fmt)
    T.floor = p < FLOOR
    T.saturated = _others(p, oh) < 2.0 ** -10        # rows whose label column is saturated (declared: vacuity)
    T.named = T.floor | ((oh > 0) & T.saturated[:, None]) if case.head == "ce" else T.floor
    T.N = torch.where(oh > 0, torch.full_like(N, abs(float(case.scale)) / T.n_valid), N) if case.head == "action" else N
    T.cap = ((7.0 if case.head == "double" else 2.0) * case.V + 256.0 + 4.0 * float(z.abs().max())) * E32
    T.amax = _first_argmax(z)
    if exact:
        T.dz = Ref(round_out(T.dz_exact, fmt), torch.zeros_like(dz), fmt, signed_ok=False)
        if T.loss_exact is not None:
            T.loss = Ref(T.loss_exact, torch.zeros_like(loss), "f32")
    return T


def _exact_values(case, I, T):
    """the exact constructions' expected values, stated directly (the float64 formulas keep exp(-200) = 1.4e-87)"""
    T.dz_exact, T.loss_exact = None, None
    V, scale = case.V, case.scale
    oh = _onehot(I.y, V)
    if case.kind == "onehot":
        hot = _onehot(I.hot, V)
        T.dz_exact = scale * (hot - oh)
        T.loss_exact = torch.where(I.hot == I.y, 0.0, 200.0).to(F64)
    elif case.kind == "uniform":
        assert V & (V - 1) == 0 and not case.two_pass
        T.dz_exact = scale * (1.0 / V - oh)


def ce_reference_two_pass(case, fmt):
    """a register-kernel case judged as the two-pass kernel would be (the host's online emulation runs every width)"""
    return ce_reference(case, fmt, two_pass=True)


def ce_reference(case, fmt, two_pass=None):
    I, T = inputs(case), Terms()
    V, scale = case.V, float(case.scale)
    z = I.z.to(F64)
    oh = _onehot(I.y, V)
    m, R, s, lse, p, a, rs = _softmax_terms(z)
    if case.two_pass if two_pass is None else two_pass:
        L = 4 * math.ceil(V / 1024) + 9
        rs = rs + (2.0 * (m - z.min(1, keepdim=True).values) + 4.0 * L) * E32
    dlse = rs + 3.0 * E32 * torch.log(s).abs() + E32 * lse.abs()
    loss = (lse - z.gather(1, I.y[:, None])).view(-1)
    loss_bound = dlse.view(-1) + E32 * loss.abs()
    dz = scale * (p - oh)
    rp = dlse + (3.0 * (z - lse).abs() + 6.0) * E32
    E = abs(scale) * (p * rp + 2.0 * E32 * (p + oh)) + torch.where(p < FLOOR, abs(scale) * FLOOR, 0.0)
    _exact_values(case, I, T)
    return _finish(T, case, fmt, loss, loss_bound, dz, E, dz.abs(), p, oh, z)


def double_values(z, y, scale, mutant=None, Vpad=None):
    """float64 values of the double softmax (and its arithmetic mutants)"""
    V = z.shape[1]
    oh = _onehot(y, V)
    p = torch.softmax(z, 1)
    ep = torch.exp(p)
    s2 = ep.sum(1, keepdim=True)
    if mutant == "exp_p_summed_over_vpad":
        s2 = s2 + float(Vpad - V)
    q = ep / s2
    T_ = (q * p).sum(1, keepdim=True)
    if mutant == "exp_p_summed_over_vpad":
        T_ = (ep * p).sum(1, keepdim=True) / s2
    py = p.gather(1, y[:, None])
    if mutant == "p_y_from_the_wrong_8_group":
        groups = (V + 7) // 8
        col = (y % 8) + 8 * ((y // 8 + 1) % groups)
        py = torch.where(col[:, None] < V, p.gather(1, col.clamp(max=V - 1)[:, None]), torch.zeros_like(py))
    loss = torch.log(s2) - py
    dot = T_ - py
    if mutant == "dot_term_dropped":
        dot = torch.zeros_like(dot)
    dz = scale * p * (q - oh - dot)
    if mutant == "second_softmax_dropped":
        loss, dz = -torch.log(py), scale * (p - oh)
    return loss.view(-1), dz, p, q, T_, py, s2


def double_reference(case, fmt):
    I, T = inputs(case), Terms()
    V, scale = case.V, float(case.scale)
    z = I.z.to(F64)
    oh = _onehot(I.y, V)
    _, _, _, _, _, a, rs = _softmax_terms(z)
    loss, dz, p, q, T_, py, s2 = double_values(z, I.y, scale)
    rp = a + rs + 2.0 * E32
    re = p * rp + (2.0 * p + 2.0) * E32
    rs2 = (V + 2) * E32 + (q * re).sum(1, keepdim=True)
    rt = (V + 2) * E32 + (q * p / T_ * (re + rp + E32)).sum(1, keepdim=True)
    rpy = rp.gather(1, I.y[:, None])
    loss_bound = (rs2 + 3.0 * E32 * torch.log(s2).abs() + py * rpy).view(-1) + E32 * loss.abs() + FLOOR
    D = q - oh - (T_ - py)
    dD = (q * (re + 2.0 * E32) + T_ * (rt + 2.0 * E32) + (q - T_).abs() * rs2 * (1.0 + 2.0 ** -10) + py * rpy
          + E32 * ((q - oh).abs() + (T_ - py).abs() + D.abs()))
    E = abs(scale) * p * (dD + D.abs() * (rp + 2.0 * E32)) + torch.where(p < FLOOR, abs(scale) * FLOOR, 0.0)
    N = abs(scale) * p * (q + oh + T_ + py)
    T.dz_exact, T.loss_exact = None, None
    return _finish(T, case, fmt, loss, loss_bound, dz, E, N, p, oh, z)


def action_values(z, y, grad_scale, mutant=None):
    """float64 values of the action head as its kernel comment states (and its mutants): loss, accuracy, dz, m, g"""
    B, A = z.shape
    valid = (y != -1)
    n_valid = int(valid.sum())
    l = torch.log_softmax(z, 1)
    m = torch.log_softmax(l, 1)
    oh = _onehot(y, A)
    yc = y.clamp(min=0)
    m_y = m.gather(1, yc[:, None]).view(-1)
    denom = B if mutant == "mean_over_B" else n_valid
    loss = -(m_y * valid).sum() / denom if denom else torch.tensor(float("nan"), dtype=F64)
    amax = _first_argmax(z)
    hits = int((amax == y).sum())
    if mutant == "ignored_row_hit_when_the_argmax_is_0":
        hits = int((amax == yc).sum())
    acc = np.float32(hits) / np.float32(n_valid if mutant == "accuracy_over_n_valid" else B)
    # an ignored row has weight 0 whatever n_valid is: torch's nll_loss backward writes only the rows that are not ignored, so with
    # nothing valid the loss is NaN (0 / 0) and the gradient exactly 0.  (The mutant is the product 0 * (grad_scale / 0) = NaN.)
    w = (grad_scale / denom) if denom else (float("nan") if mutant == "nan_gradient_when_nothing_is_valid" else 0.0)
    vmask = torch.ones(B, dtype=F64) if mutant == "ignored_rows_given_a_gradient" else valid.to(F64)
    ohc = oh if mutant != "ignored_rows_given_a_gradient" else _onehot(yc, A)
    g = (torch.exp(m) - ohc) * vmask[:, None] * w
    dz = g - torch.exp(l) * g.sum(1, keepdim=True)
    return loss, acc, dz, l, m, g, valid, n_valid, amax


def action_reference(case, fmt):
    I, T = inputs(case), Terms()
    A, gs = case.V, float(case.scale)
    z = I.z.to(F64)
    B = z.shape[0]
    loss, acc, dz, l, m, g, valid, n_valid, amax = action_values(z, I.y, gs)
    oh = _onehot(I.y, A)
    mx, R, s, lse, p, a, rs = _softmax_terms(z)
    T.n_valid, T.acc, T.valid = n_valid, acc, valid
    T.amax = amax
    u = U_OUT[fmt]
    if n_valid == 0:
        T.loss, T.E, T.named, T.N, T.cap, T.floor, T.saturated = None, None, None, None, None, None, None
        T.dz = Ref(torch.zeros_like(dz), torch.zeros_like(dz), fmt, signed_ok=False)       # exactly 0, as torch
        return T
    w = abs(gs) / n_valid
    iota = (R + l.abs()) * E32
    C = (p * iota).sum(1, keepdim=True) + rs + 3.0 * E32 * torch.log(s).abs()
    dm = 2.0 * iota + C
    ri = 2.0 * iota + (2.0 * l.abs() + 2.0) * E32
    v = valid.to(F64)[:, None]
    dgi = w * (p * ri + 4.0 * E32 * (p + oh)) * v
    Gi = dgi.sum(1, keepdim=True) + (A + 2) * E32 * g.abs().sum(1, keepdim=True)
    E = dgi + (1.0 + 2.0 ** -10) * p * (Gi + 2.0 ** -10 * w * C * v) + E32 * g.abs() + torch.where(p < FLOOR, w * FLOOR, 0.0) * v
    yc = I.y.clamp(min=0)
    m_y = m.gather(1, yc[:, None]).view(-1)
    dm_y = dm.gather(1, yc[:, None]).view(-1)
    loss_bound = (dm_y * valid).sum() / n_valid + (B + 2) * E32 * (m_y.abs() * valid).sum() / n_valid + E32 * loss.abs()
    T.dz_exact, T.loss_exact = None, None
    _finish(T, case, fmt, loss.view(1), loss_bound.view(1), dz, E, dz.abs(), p, oh, z)
    T.named = T.named & valid[:, None]              # an ignored row is exact (E = 0): nothing to name
    T.amax = amax
    return T


def vacuity(case, fmt="f32"):
    """max over the un-named elements of E_j / (cap N_j): must be <= 1 (module docstring); None where nothing is to be judged"""
    T = reference(case, fmt)
    if T.E is None or case.kind in ("onehot", "uniform"):
        return None
    ok = ~T.named & (T.E > 0)
    if not bool(ok.any()):
        return None
    return float((T.E[ok] / (T.cap * T.N[ok])).max())


# ---- judging one result ------------------------------------------------------------------------------------------------------------
def _held(rs, ref, got, name):
    """helpers_gemm.ratios behind a finiteness check that reports (a wrong implementation may produce NaN) instead of raising"""
    if not bool(torch.isfinite(got.to(F64)).all()):
        rs[name + " is finite"] = INF
    else:
        rs.update(ratios(ref, got, name))


def judge(case, fmt, out):
    """out: {"loss": fp32 [rows] (action: [1]), "amax": int64 [rows] (action: "acc" float), "dzbuf": [rows + 1, lddz] in the output
    dtype or float64, or None (the call without a gradient)} -> {check: measured / bound}; 0 / inf for the exact checks."""
    T, I = reference(case, fmt), inputs(case)
    V, Vpad = case.V, case.Vpad
    rs = {}
    flag = lambda ok: 0.0 if ok else INF
    if case.head == "action":
        rs["accuracy == float32(hits) / float32(B)"] = flag(float(out["acc"]) == float(T.acc))
        if T.n_valid == 0:
            rs["loss is NaN"] = flag(bool(torch.isnan(out["loss"].to(F64)).all()))
        else:
            _held(rs, T.loss, out["loss"].view(1), "loss")
    else:
        _held(rs, T.loss, out["loss"], "loss")
        rs["amax is the first maximum"] = flag(torch.equal(out["amax"].to(torch.int64).cpu(), T.amax))
    if out.get("dzbuf") is None:
        return rs
    d = out["dzbuf"].to(F64)
    assert tuple(d.shape) == (I.rows + 1, case.lddz), (d.shape, I.rows, case.lddz)
    if T.dz is not None:
        _held(rs, T.dz, d[:I.rows, :V], "dz")
    rs["dz [V, Vpad) is zero"] = flag(bool((d[:I.rows, V:Vpad] == 0).all()))
    sent = float(round_out(torch.tensor(SENTINEL, dtype=F64), fmt))
    rs["sentinels intact"] = flag(bool((d[:I.rows, Vpad:] == sent).all()) and bool((d[I.rows] == sent).all()))
    return rs


def signed_pool(pairs):
    """pairs of (case, fmt = bf16, dz [rows, V] float64): helpers_attention.signed_stat pooled over the un-named elements of random
    cases (a rounding to nearest is zero-mean; a truncating convert follows the sign of the output) -> (stat, N)"""
    errs, refs, bounds = [], [], []
    for case, dz in pairs:
        T = reference(case, "bf16")
        if T.loss is None or case.kind in ("onehot", "uniform"):
            continue
        ok = ~T.named & (T.dz.bound > 0)
        if case.head == "action":
            ok &= T.valid[:, None]
        errs.append((dz.to(F64) - T.dz.y)[ok])
        refs.append(T.dz.y[ok])
        bounds.append(T.dz.bound[ok])
    return signed_stat(torch.cat(errs), torch.cat(refs), torch.cat(bounds))


# ---- the minimal implementation and the mutants (float64, every output rounded once) ------------------------------------------------
CE_MUTANTS = ("onehot_subtracted_at_y_plus_1", "onehot_unscaled", "last_partial_vector_left_out_of_the_sum",
              "tail_padding_read_into_the_sum", "argmax_over_vpad", "last_of_ties_argmax", "tie_merge_prefers_the_higher_wave",
              "vpad_columns_left_unwritten", "p_rounded_to_bf16_before_the_onehot", "truncating_bf16_convert",
              "lse_without_the_final_plus_m")
DOUBLE_MUTANTS = ("second_softmax_dropped", "dot_term_dropped", "p_y_from_the_wrong_8_group", "exp_p_summed_over_vpad")
ACTION_MUTANTS = ("mean_over_B", "ignored_rows_given_a_gradient", "accuracy_over_n_valid", "ignored_row_hit_when_the_argmax_is_0",
                  "nan_gradient_when_nothing_is_valid")
MUTANTS = {"ce": CE_MUTANTS, "double": DOUBLE_MUTANTS, "action": ACTION_MUTANTS}


def mutant_applies(mutant, case, fmt):
    I = inputs(case)
    V = case.V
    if mutant == "last_partial_vector_left_out_of_the_sum":
        return V % 4 != 0 and V > 4
    if mutant == "tail_padding_read_into_the_sum":
        return V % 4 != 0
    if mutant in ("argmax_over_vpad", "vpad_columns_left_unwritten", "exp_p_summed_over_vpad"):
        return case.Vpad > V
    if mutant in ("last_of_ties_argmax", "tie_merge_prefers_the_higher_wave"):
        return case.kind == "ties"
    if mutant == "p_rounded_to_bf16_before_the_onehot":
        return fmt == "f32" and 1 < V <= 2048 and case.kind not in ("onehot", "uniform")
    if mutant == "truncating_bf16_convert":
        return fmt == "bf16" and case.kind not in ("onehot", "uniform", "ties")
    if mutant == "lse_without_the_final_plus_m":
        return case.kind == "offset"
    if mutant == "onehot_subtracted_at_y_plus_1":
        return V > 1
    if mutant == "p_y_from_the_wrong_8_group":
        return V > 8
    if case.head == "action":
        n_ign = int((I.y == -1).sum())
        if mutant == "nan_gradient_when_nothing_is_valid":
            return n_ign == I.rows
        if mutant == "ignored_row_hit_when_the_argmax_is_0":
            return bool(((I.y == -1) & (reference(case, fmt).amax == 0)).any())
        return 0 < n_ign < I.rows
    return True


def _wave_of(col):
    return (col % 1024) // 256          # thread (col % 1024) // 4 of a 256-thread workgroup, 64 lanes per wave


def _buffer(case, I, dz, fmt, unwritten=False):
    buf = torch.full((I.rows + 1, case.lddz), float(round_out(torch.tensor(SENTINEL, dtype=F64), fmt)), dtype=F64)
    buf[:I.rows, :case.V] = dz
    if not unwritten:
        buf[:I.rows, case.V:case.Vpad] = 0.0
    return buf


def model(case, fmt, mutant=None):
    """the minimal implementation (float64, every output rounded once), or one wrong in the one way `mutant` names"""
    I = inputs(case)
    V, scale = case.V, float(case.scale)
    z = I.z.to(F64)
    trunc = mutant == "truncating_bf16_convert"
    if case.head == "action":
        loss, acc, dz, *_ = action_values(z, I.y, scale, mutant)
        return {"loss": round_out(loss.view(1), "f32"), "acc": acc, "dzbuf": _buffer(case, I, round_out(dz, fmt, trunc=trunc), fmt)}
    y = I.y
    if case.head == "double":
        loss, dz, *_ = double_values(z, y, scale, mutant, case.Vpad)
        amax = _first_argmax(z)
    else:
        # (an exact construction is modelled with what fp32 delivers: exp(-200) = 0)
        zc = torch.where(z == -200.0, torch.full_like(z, -INF), z) if case.kind == "onehot" else z
        zs = zc
        if mutant == "last_partial_vector_left_out_of_the_sum":
            zs = zc[:, :V - V % 4]
        elif mutant == "tail_padding_read_into_the_sum":
            zs = torch.cat([zc, I.zbuf[:, V:round_up(V, 4)].to(F64)], 1)
        m = zs.max(1, keepdim=True).values
        s = torch.exp(zs - m).sum(1, keepdim=True)
        lse = (m + torch.log(s)) if mutant != "lse_without_the_final_plus_m" else torch.log(s)
        p = torch.exp(zc - m) / s
        if mutant == "p_rounded_to_bf16_before_the_onehot":
            p = hg.bf16r(p)
        loss = (lse - z.gather(1, y[:, None])).view(-1)
        yy = (y + 1) % V if mutant == "onehot_subtracted_at_y_plus_1" else y
        oh = _onehot(yy, V)
        dz = p * scale - oh if mutant == "onehot_unscaled" else scale * (p - oh)
        amax = _first_argmax(z)
        if mutant == "argmax_over_vpad":
            amax = _first_argmax(torch.cat([z, torch.full((I.rows, case.Vpad - V), PAD_IN, dtype=F64)], 1))
        elif mutant == "last_of_ties_argmax":
            amax = V - 1 - _first_argmax(z.flip(1))
        elif mutant == "tie_merge_prefers_the_higher_wave":
            at = z == z.max(1, keepdim=True).values
            amax = amax.clone()
            for r in range(I.rows):
                cols = torch.nonzero(at[r]).view(-1)
                top = int(_wave_of(cols).max())
                amax[r] = int(cols[_wave_of(cols) == top][0])
    dzr = round_out(dz, fmt, trunc=trunc)
    return {"loss": round_out(loss, "f32"), "amax": amax,
            "dzbuf": _buffer(case, I, dzr, fmt, unwritten=mutant == "vpad_columns_left_unwritten")}


# ---- float32 emulations in four summation orders -----------------------------------------------------------------------------------
F32 = np.float32
_LOG2E, _LN2 = F32(1.4426950408889634), F32(0.6931471805599453)


def expf(x):
    """__expf on float32 numpy: the argument times log2(e) rounded to fp32, then a correctly rounded 2^y"""
    y = (x.astype(F32) * _LOG2E).astype(F32)
    with np.errstate(under="ignore", over="ignore"):
        return np.exp2(y.astype(np.float64)).astype(F32)


def logf(x):
    with np.errstate(divide="ignore"):
        return (np.log2(x.astype(np.float64)).astype(F32) * _LN2).astype(F32)


def _thread_layout(a, fill):
    """[rows, n] -> [rows, 256, steps]: thread t of a 256-thread workgroup owns the 4-vectors at columns 4 t + 1024 k, in order"""
    rows, n = a.shape
    K = (n + 1023) // 1024
    full = np.full((rows, K * 1024), fill, dtype=a.dtype)
    full[:, :n] = a
    return full.reshape(rows, K, 256, 4).transpose(0, 2, 1, 3).reshape(rows, 256, K * 4)


def sum32(a, order):
    """float32 sum over the last axis of [rows, n] in one of three orders (the fourth, `online`, is a different algorithm)"""
    a = a.astype(F32)
    if order == "sequential":
        return np.cumsum(a, axis=1, dtype=F32)[:, -1]
    if order == "pairwise":
        n = 1 << max(0, (a.shape[1] - 1).bit_length())
        full = np.zeros((a.shape[0], n), dtype=F32)
        full[:, :a.shape[1]] = a
        while full.shape[1] > 1:
            full = (full[:, 0::2] + full[:, 1::2]).astype(F32)
        return full[:, 0]
    if order == "lanes":      # the kernels' own shape: a per-thread chain, 6 butterfly levels over the lanes, the four waves in turn
        t = np.cumsum(_thread_layout(a, 0.0), axis=2, dtype=F32)[:, :, -1].reshape(-1, 4, 64)
        w = 64
        while w > 1:
            w //= 2
            t = (t[:, :, :w] + t[:, :, w:2 * w]).astype(F32)
        t = t[:, :, 0]
        return (((t[:, 0] + t[:, 1]).astype(F32) + t[:, 2]).astype(F32) + t[:, 3]).astype(F32)
    raise ValueError(order)


def _online_ms(z):
    """(m, s) of every row by the two-pass kernel's algorithm: per-thread online chains, (m, s) merges over lanes and waves"""
    t = _thread_layout(z.astype(F32), -np.inf)
    rows = t.shape[0]
    m = np.full((rows, 256), -np.inf, dtype=F32)
    s = np.zeros((rows, 256), dtype=F32)

    def merge(m1, s1, m2, s2):
        mn = np.maximum(m1, m2)
        with np.errstate(invalid="ignore"):
            a1 = np.where(m1 == -np.inf, F32(0), expf(np.where(m1 == -np.inf, F32(0), m1 - mn)))
            a2 = np.where(m2 == -np.inf, F32(0), expf(np.where(m2 == -np.inf, F32(0), m2 - mn)))
        return mn, ((s1 * a1).astype(F32) + (s2 * a2).astype(F32)).astype(F32)

    for k in range(t.shape[2]):
        m, s = merge(m, s, t[:, :, k], np.where(t[:, :, k] == -np.inf, F32(0), F32(1)))
    m, s = m.reshape(rows, 4, 64), s.reshape(rows, 4, 64)
    w = 64
    while w > 1:
        w //= 2
        m, s = merge(m[:, :, :w], s[:, :, :w], m[:, :, w:2 * w], s[:, :, w:2 * w])
    m, s = m[:, :, 0], s[:, :, 0]
    M, S = m[:, 0], s[:, 0]
    for wv in range(1, 4):
        M, S = merge(M, S, m[:, wv], s[:, wv])
    return M, S


def emulation(case, order, fmt):
    """an honest float32 implementation in one summation order -> the same dict model() returns (dz: [rows, V] only, under "dz")"""
    I = inputs(case)
    V, scale = case.V, F32(case.scale)
    z = I.z.numpy().astype(F32)
    rows = z.shape[0]
    ar = np.arange(rows)
    y = I.y.numpy()
    fin = lambda x: round_out(torch.from_numpy(np.asarray(x, dtype=np.float64)), fmt)
    if case.head == "action":
        return _action_emulation(case, order, fmt, z, y, fin)
    oh = np.zeros((rows, V), dtype=F32)
    oh[ar, y] = 1
    if order == "online":
        m, s = _online_ms(z)
    else:
        m = z.max(1)
        ev = expf(z - m[:, None])
        s = sum32(ev, order)
    if case.head == "ce":
        lse = (m + logf(s)).astype(F32)
        loss = (lse - z[ar, y]).astype(F32)
        if order == "online":       # the two-pass kernel's gradient: a second __expf against lse
            g = ((expf((z - lse[:, None]).astype(F32)) - oh).astype(F32) * scale).astype(F32)
        else:                       # the register kernels': exp(z - m) (scale / s) - scale onehot
            f = (scale / s).astype(F32)
            g = ((ev * f[:, None]).astype(F32) - oh * scale).astype(F32)
        return {"loss": torch.from_numpy(loss.astype(np.float64)), "dz": fin(g)}
    # double softmax
    if order == "online":
        ev = expf(z - m[:, None])
        order2 = "lanes"
    else:
        order2 = order
    inv = (F32(1) / s).astype(F32)
    p = (ev * inv[:, None]).astype(F32)
    e2 = expf(p)
    s2 = sum32(e2, order2)
    t = sum32((e2 * p).astype(F32), order2)
    py = p[ar, y]
    loss = (logf(s2) - py).astype(F32)
    dot = ((t / s2).astype(F32) - py).astype(F32)
    dpi = ((e2 / s2[:, None]).astype(F32) - oh).astype(F32)
    g = ((p * (dpi - dot[:, None]).astype(F32)).astype(F32) * scale).astype(F32)
    return {"loss": torch.from_numpy(loss.astype(np.float64)), "dz": fin(g)}


def _action_emulation(case, order, fmt, z, y, fin):
    B, A = z.shape
    gs = F32(case.scale)
    valid = y != -1
    n_valid = int(valid.sum())
    sm = (lambda a: sum32(a, order)) if order != "online" else None

    def log_softmax(v):
        if order == "online":
            m, s = _online_ms(v)
        else:
            m = v.max(1)
            s = sm(expf(v - m[:, None]))
        return ((v - m[:, None]).astype(F32) - logf(s)[:, None]).astype(F32)

    l = log_softmax(z)
    m = log_softmax(l)
    yc = np.maximum(y, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_n = (F32(1) / F32(n_valid)).astype(F32)
        m_y = m[np.arange(B), yc]
        loss = F32(0)
        for w in range(16):                                            # one partial per wave, rows b = w, w + 16, ...
            part = F32(0)
            for b in range(w, B, 16):
                if valid[b]:
                    part = F32(part - m_y[b])
            loss = F32(loss + part)
        loss = F32(loss * inv_n)
        oh = np.zeros((B, A), dtype=F32)
        oh[np.arange(B), yc] = 1
        wgt = (valid.astype(F32) * F32(gs * inv_n)).astype(F32)
        g = ((expf(m) - oh).astype(F32) * wgt[:, None]).astype(F32)
        gsum = sum32(g, order if order != "online" else "lanes")
        d = (g - (expf(l) * gsum[:, None]).astype(F32)).astype(F32)
    return {"loss": torch.tensor([float(loss)], dtype=F64), "dz": fin(d)}


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
def _c(rows, kinds, head, V, **kw):
    return [Case(head, k, rows, V, i=i, **kw) for i, k in enumerate(kinds)]


def ce_cases():
    out = []
    add = lambda V, kinds, rows=4, **kw: out.extend(_c(rows, kinds, "ce", V, **kw))
    add(1, ("normal",), why="one column: p = 1, dz = 0")
    add(3, ("normal", "bf16grid"), why="scalar tail only")
    add(8, ("normal", "bf16grid", "wide"), why="Vpad = V")
    add(9, ("normal", "wide12", "confident"), why="one full vector and a one-column tail, Vpad > V")
    add(97, ("normal", "offset", "wide12", "confident", "bf16grid"), rows=6, why="odd width below one chunk")
    add(1023, ("normal", "wide12"), why="a chunk less one column: 3-column tail")
    add(1024, ("normal", "confident"), why="one chunk of reg<8> exactly")
    add(1025, ("normal", "offset"), why="a chunk and one column")
    add(1601, ("normal", "wide12", "bf16grid", "confident"), rows=5, why="the token head's width")
    add(2048, ("normal", "offset", "wide12"), rows=6, why="V e = 2^-13: the g32 precision mutants are judged here")
    add(8192, ("normal",), why="the last width of reg<8>")
    add(8193, ("normal", "confident"), Vpad=8200, why="the first width of reg<32>")
    add(30522, ("normal", "bf16grid"), Vpad=30528, ldz=30528 + 4, scale=1.0 / 4272, why="production: reg<32>")
    add(32768, ("normal", "offset"), rows=3, why="the last width of reg<32>")
    add(32770, ("normal", "wide12", "confident"), rows=3, Vpad=32776, why="the first width of the two-pass kernel; V % 4 = 2")
    add(33001, ("normal", "offset", "bf16grid"), rows=3, Vpad=33024, lddz=33032, why="two-pass with padding and a row stride")
    for V, kw in ((9, {}), (1027, {}), (2051, {}), (8193, {"Vpad": 8200}), (33001, {"Vpad": 33024, "lddz": 33032})):
        out.append(Case("ce", "onehot", 0, V, scale=2.0 ** -5, why="one-hot rows: exact", **kw))
    for V in (8, 1024, 8192, 32768):
        out.append(Case("ce", "uniform", 3, V, scale=2.0 ** -3, why="uniform rows at a power of two: exact"))
    for V, kw in ((11, {}), (3000, {}), (8193, {"Vpad": 8200}), (33001, {"Vpad": 33024, "lddz": 33032})):
        out.append(Case("ce", "ties", 0, V, why="the maximum at two or three columns", **kw))
    return out


DOUBLE_V = (1, 5, 8, 9, 40, 63, 64, 65, 511, 512, 513, 1601, 2041, 2048)


def double_cases():
    out = []
    kinds = ("normal", "bf16grid", "confident", "offset", "wide12")
    for n, V in enumerate(DOUBLE_V):
        ks = ("normal", kinds[1 + n % 4]) if V > 1 else ("normal",)
        out += _c(8 if V >= 1601 else 4, ks, "double", V, why="width %d" % V, Vpad=round_up(V, 8) + (8 if V in (40, 513) else 0))
    out.append(Case("double", "ties", 0, 2048, why="the maximum at two or three columns"))
    out.append(Case("double", "ties", 0, 513, why="the maximum at two or three columns", i=1))
    return out


ACTION_B = (1, 15, 16, 17, 37, 256, 1025)
ACTION_A = (1, 2, 7, 36, 63, 64)


def action_cases():
    """B x A x the ignored counts 0, 1, B - 1, B; the kind and Ap (round_up(A, 8) or 64) alternate along the table"""
    out = []
    kinds = ("normal", "bf16grid", "confident", "offset")
    n = 0
    for B in ACTION_B:
        for A in ACTION_A:
            if B in (256, 1025) and A not in (7, 36, 64):
                continue
            for ign in sorted(set((0, 1, B - 1, B))):
                Ap = (round_up(A, 8), 64)[n % 2]
                out.append(Case("action", kinds[(n // 2) % 4], B, A, Vpad=Ap, i=n, ignored=ign,
                                why="B = %d, A = %d, Ap = %d, %d ignored" % (B, A, Ap, ign)))
                n += 1
    for A in (2, 7, 64):
        out.append(Case("action", "ties", 0, A, Vpad=round_up(A, 8), why="ties among columns 0, 1, A - 1"))
    return out


_CASES = {}


def cases(head):
    if head not in _CASES:
        _CASES[head] = {"ce": ce_cases, "double": double_cases, "action": action_cases}[head]()
    return _CASES[head]


def all_cases():
    return [c for h in ("ce", "double", "action") for c in cases(h)]


# ---- one case on the GPU -----------------------------------------------------------------------------------------------------------
def run(case, fmt, dev, grad=True):
    """through visitron_amd.ops only; the gradient lands in a SENTINEL-filled [rows + 1, lddz] buffer"""
    from visitron_amd import ops

    I = inputs(case)
    z = I.zbuf.to(dev)[:, :case.V]                                     # row stride ldz > V, +50 behind every row
    y = I.y.to(dev)
    buf = torch.full((I.rows + 1, case.lddz), SENTINEL, dtype=DT[fmt], device=dev)
    dz = buf[:I.rows, :case.Vpad] if grad else None
    g32 = fmt == "f32"
    if case.head == "action":
        f = ops.action_head_g32 if g32 else ops.action_head
        loss, acc, _ = f(z, y, case.V, case.scale, case.Vpad, dz=dz)
        torch.cuda.synchronize()
        return {"loss": loss.cpu().view(1), "acc": float(acc.cpu()), "dzbuf": buf.cpu()}
    f = {("ce", False): ops.ce_softmax_rows, ("ce", True): ops.ce_softmax_rows_g32, ("double", False): ops.ce_double_softmax_rows,
         ("double", True): ops.ce_double_softmax_rows_g32}[(case.head, g32 and grad)]
    loss, amax = f(z, y, case.V, dz, case.scale)
    torch.cuda.synchronize()
    return {"loss": loss.cpu(), "amax": amax.cpu(), "dzbuf": buf.cpu() if grad else None}


def same_bits(a, b):
    """two results of run(): every output bit for bit (NaN included)"""
    for k in a:
        if a[k] is None or isinstance(a[k], float):
            if not (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])):
                return False
            continue
        x, y = a[k].contiguous(), b[k].contiguous()
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()]
        if not torch.equal(x.view(it), y.view(it)):
            return False
    return True
