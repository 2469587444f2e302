"""float64 restatement of the turn-based decoder kernels (csrc/turn_based.hip), with per-element bounds.

Written from the formulas, not from any implementation.

THE CELL.  x = [emb | feature] (emb = table[id], or a ready block; an id outside the table counts as a zero row), K = E + F + hs:
    z_q = x . W_ih[q]^T + h . W_hh[q]^T + b_ih[q] + b_hh[q]         q = i, f, g, o (rows q*hs .. (q+1)*hs of the weights)
    i, f, o = sigmoid(z),  g = tanh(z_g),  c' = f c + i g,  h' = o tanh(c')
The weights are the bf16 operands themselves (exact in float64).  The kernel rounds each activation to bf16 (relative 2^-9),
forms exact products and adds them in fp32 in some order; with S = sum |x||w| + |b| per gate element
    |z - z_ref| <= delta = (2^-8 + (K + 8) 2^-23) S
(2^-8: twice the activation rounding; (K + 8) 2^-23: K fp32 additions in any order, the bias sum and the partial-sum hand-over).
sigmoid' <= 1/4 and tanh' <= 1, so with EPS_ACT the error of the fast sigmoid / tanh themselves
    e_i, e_f, e_o = delta / 4 + EPS_ACT        e_g = delta + EPS_ACT
    bound(c') = |c| e_f + |g| e_i + i e_g + e_i e_g + 2^-22 (|f c| + |i g|)            (two products and a sum in fp32)
    bound(h') = |tanh c'| e_o + (o + e_o) (bound(c') + EPS_ACT) + 2^-22 |h'|            (tanh' <= 1)
EPS_ACT cannot be derived (v_exp_f32 / v_rcp_f32 carry no stated bound here): it is TWICE the largest error measured on an
MI355X from vt_lstm_step_train_f32 with zero recurrent weights (gates = xproj) against float64 over [-20, 20]
(tools/turn_based_bench.py --epsilon, profiles/r14/turn_based.txt).

THE HEAD.  l = logit with blocked entries at -inf; per counted row (target != ignore_index) loss_r = logsumexp(l) - l[target],
loss = mean.  fp32 arithmetic on at most 64 terms: exp relative 2^-22, the sum of <= 64 terms relative 8 * 2^-24, log absolute
2^-23 + 2^-24 |log z|, two additions -> bound(loss_r) = 2^-20 + 2^-22 (|max| + |l[target]| + |loss_r|), and the mean adds
2^-24 (n / 16 + 17) mean |loss_r| (16 running sums, then 16 more additions and a division).
dlogit = g (softmax - onehot) / n within 2^-20 + 2^-22 |value| for |g| <= 1.
"""
import math

import numpy as np
import torch

from helpers_attention import bf16_trunc, bf16r, signed_stat  # noqa: F401
from helpers_gemm import hash32   # the one Python restatement of vt_hash32

F64 = torch.float64
EPS_MEASURED = 1.2688e-07    # profiles/r14/turn_based.txt: max |fast sigmoid / tanh - float64| over [-20, 20] on an MI355X
EPS_ACT = 2.0 * EPS_MEASURED
SENTINEL = -768.0   # exact in bf16 too

MUTANTS = ("gate_order_igfo", "no_b_hh", "bias_twice", "emb_row_plus_one", "feature_col_plus_one", "feature_col_minus_one",
           "k_tail_dropped", "pad_reads_next_row", "bf16_truncate", "c_written_back", "row_past_B")


class CellCase(object):
    """Operands of one call (CPU tensors; weights hold bf16-representable values)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def K(self):
        return self.E + self.F

    def emb_rows(self, shift=0):
        """fp32 [B, E]: the first operand as rows (an id outside the table: zeros)."""
        if self.ids is None:
            return self.x_emb
        ids = self.ids + shift
        ok = (ids >= 0) & (ids < self.A)
        rows = self.table[ids.clamp(0, self.A - 1)]
        return torch.where(ok[:, None], rows, torch.zeros_like(rows))


def marker_columns(E, F):
    """Columns of the concatenated row whose loss or shift a check must see: both ends of both sources and the last K mod 4."""
    K = E + F
    return sorted(set(c for c in (0, E - 1, E, E + 1, K - 3, K - 2, K - 1) if 0 <= c < K))


def cell_operands(B, hs, E, F, A=8, seed=0, kind="random", block=False):
    """kind: "random"   small weights (so that S stays near 1 and the bound far below the values) with large ones on the marker
                        columns, biases in [-1, 1], c ~ N(0, 1);
             "positive" non-negative activations and weights, zero bias: every activation rounding pushes z the same way under a
                        truncating convert (the signed-bias statistic);
             "exact"    small integers whose every pre-activation is zero: i = f = o = 1/2, g = 0, c' = c / 2 bit for bit."""
    g = torch.Generator().manual_seed(1000 + seed)
    K, G = E + F, 4 * hs
    rnd = lambda *s: torch.randn(*s, generator=g)
    if kind == "exact":
        # x and h in {-2..2}, weights in {-1, 0, 1}; each weight row is made orthogonal to every activation row by giving
        # columns in pairs (k, k + 1) the weights (v, -v) and the activations equal values on a pair; the odd last column
        # and the bias are zero
        def paired(n, width, lo, hi):
            half = torch.randint(lo, hi + 1, (n, width // 2), generator=g).float()
            full = torch.zeros(n, width)
            full[:, 0:2 * (width // 2):2], full[:, 1:2 * (width // 2):2] = half, half
            return full
        xcat = paired(B, K, -2, 2)
        h_prev = paired(B, hs, -2, 2)
        def anti(n, width):
            half = torch.randint(-1, 2, (n, width // 2), generator=g).float()
            full = torch.zeros(n, width)
            full[:, 0:2 * (width // 2):2], full[:, 1:2 * (width // 2):2] = half, -half
            return full
        w_ih, w_hh = anti(G, K), anti(G, hs)
        b_ih, b_hh = torch.zeros(G), torch.zeros(G)
        c_prev = torch.randint(-8, 9, (B, hs), generator=g).float() / 4.0
        ids, table, x_emb = None, None, xcat[:, :E].contiguous()
        feature = xcat[:, E:].contiguous()
        return CellCase(B=B, hs=hs, E=E, F=F, A=0, ids=ids, table=table, x_emb=x_emb, feature=feature, h_prev=h_prev,
                        c_prev=c_prev, w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh, kind=kind)
    pos = kind == "positive"
    table = rnd(A, E)
    feature = rnd(B, F).abs()                       # image features are non-negative
    h_prev = rnd(B, hs) * 0.5
    c_prev = rnd(B, hs)
    if pos:
        table, h_prev = table.abs(), h_prev.abs()
    Kt = K + hs
    w_ih = torch.rand(G, K, generator=g) if pos else rnd(G, K)
    w_hh = torch.rand(G, hs, generator=g) if pos else rnd(G, hs)
    w_ih, w_hh = w_ih * (1.0 / Kt), w_hh * (1.0 / Kt)
    if not pos:
        for c in marker_columns(E, F):
            w_ih[:, c] = (torch.rand(G, generator=g) * 0.125 + 0.125) * torch.where(torch.rand(G, generator=g) < 0.5, -1.0, 1.0)
    w_ih, w_hh = w_ih.to(torch.bfloat16).float(), w_hh.to(torch.bfloat16).float()
    b_ih = torch.zeros(G) if pos else (torch.rand(G, generator=g) - 0.5)
    b_hh = torch.zeros(G) if pos else (torch.rand(G, generator=g) - 0.5)
    ids = torch.randint(0, A, (B,), generator=g)
    o = CellCase(B=B, hs=hs, E=E, F=F, A=A, ids=ids, table=table, x_emb=None, feature=feature, h_prev=h_prev, c_prev=c_prev,
                 w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=b_hh, kind=kind)
    if block:
        o.x_emb, o.ids, o.table, o.A = o.emb_rows().clone(), None, None, 0
    return o


def _gates(z, hs, order=(0, 1, 2, 3)):
    q = [z[:, k * hs:(k + 1) * hs] for k in order]
    return torch.sigmoid(q[0]), torch.sigmoid(q[1]), torch.tanh(q[2]), torch.sigmoid(q[3])


def _cell_values(o, mutant=None, convert=None):
    """float64 z [B, 4hs] and the concatenated activations, with an optional wrong implementation."""
    emb = o.emb_rows(1 if mutant == "emb_row_plus_one" else 0).to(F64)
    feat = o.feature.to(F64)
    if mutant == "feature_col_plus_one":       # reads column E + 1 where E belongs: the feature one element late
        feat = torch.cat((feat[:, 1:], torch.zeros(o.B, 1, dtype=F64)), 1)
    if mutant == "feature_col_minus_one":      # one element early: the first feature column is the last embedding column
        feat = torch.cat((emb[:, -1:], feat[:, :-1]), 1)
    x = torch.cat((emb, feat), 1)
    h = o.h_prev.to(F64)
    if mutant == "k_tail_dropped":
        x = x.clone()
        x[:, o.K - (o.K % 4):] = 0.0
    if convert is not None:
        x, h = convert(x), convert(h)
    z = x @ o.w_ih.to(F64).t() + h @ o.w_hh.to(F64).t() + o.b_ih.to(F64)
    if mutant != "no_b_hh":
        z = z + o.b_hh.to(F64)
    if mutant == "bias_twice":
        z = z + o.b_ih.to(F64) + o.b_hh.to(F64)
    if mutant == "pad_reads_next_row":
        # the columns between K and the padded width read on into the buffer: zero weights there, so finite neighbours add
        # 0 -- but the last row's neighbour is the NaN fill around every operand
        z = z.clone()
        z[o.B - 1] = float("nan")
    return z, x, h


class CellRef(object):
    pass


def cell_reference(o):
    """float64 values and bounds: .h, .c [B, hs], .gates [B, 4hs] (activated i f g o), .bh, .bc, .bg."""
    z, x, h = _cell_values(o)
    hs = o.hs
    S = x.abs() @ o.w_ih.to(F64).abs().t() + h.abs() @ o.w_hh.to(F64).abs().t() + (o.b_ih.to(F64) + o.b_hh.to(F64)).abs()
    delta = (2.0 ** -8 + (o.K + hs + 8) * 2.0 ** -23) * S
    i, f, g, og = _gates(z, hs)
    e = [delta[:, k * hs:(k + 1) * hs] * (1.0 if k == 2 else 0.25) + EPS_ACT for k in range(4)]
    c = o.c_prev.to(F64)
    cn = f * c + i * g
    bc = c.abs() * e[1] + g.abs() * e[0] + i * e[2] + e[0] * e[2] + 2.0 ** -22 * ((f * c).abs() + (i * g).abs())
    hn = og * torch.tanh(cn)
    bh = torch.tanh(cn).abs() * e[3] + (og + e[3]) * (bc + EPS_ACT) + 2.0 ** -22 * hn.abs()
    r = CellRef()
    r.h, r.c, r.gates, r.bh, r.bc, r.bg = hn, cn, torch.cat((i, f, g, og), 1), bh, bc, torch.cat(e, 1)
    r.c_prev, r.h_prev16 = o.c_prev.clone(), o.h_prev.to(torch.bfloat16)
    return r


def _buffers(o, hn, cn, gates, mutant=None):
    """What a call leaves behind, as the checks read it: results, the caller's c buffer, guard rows around the outputs."""
    out = dict(h=hn, c=cn, gates=gates, c_prev_after=o.c_prev.clone(), h_guard=torch.full((2, o.hs), SENTINEL, dtype=F64),
               c_guard=torch.full((2, o.hs), SENTINEL, dtype=F64))
    if mutant == "c_written_back":
        out["c_prev_after"] = cn.to(torch.float32)
    if mutant == "row_past_B":
        out["h_guard"][1] = hn[0]
    return out


def cell_model(o, mutant=None):
    """float64 throughout, activations rounded to bf16 once (truncated: the mutant)."""
    z, _, _ = _cell_values(o, mutant, convert=bf16_trunc if mutant == "bf16_truncate" else bf16r)
    i, f, g, og = _gates(z, o.hs, (0, 2, 1, 3) if mutant == "gate_order_igfo" else (0, 1, 2, 3))
    cn = f * o.c_prev.to(F64) + i * g
    return _buffers(o, og * torch.tanh(cn), cn, torch.cat((i, f, g, og), 1), mutant)


def cell_emulation_f32(o, order):
    """One legitimate implementation in float32 numpy: bf16 activations, exact products, fp32 sums in the given order
    ("forward", "backward", "waves": 32-wide steps dealt to four running sums, as the kernel's four waves), fp32 gates."""
    f32 = np.float32
    x = torch.cat((o.emb_rows(), o.feature), 1)
    xa = torch.cat((bf16r(x), bf16r(o.h_prev)), 1).numpy().astype(f32)               # [B, Kt]
    w = torch.cat((o.w_ih, o.w_hh), 1).numpy().astype(f32)                            # [G, Kt]
    Kt = xa.shape[1]
    z = np.zeros((o.B, 4 * o.hs), dtype=f32)
    for b in range(o.B):
        prod = w * xa[b][None, :]                                                     # exact: bf16 x bf16 fits fp32
        if order == "forward":
            z[b] = np.cumsum(prod, axis=1, dtype=f32)[:, -1]
        elif order == "backward":
            z[b] = np.cumsum(prod[:, ::-1], axis=1, dtype=f32)[:, -1]
        else:
            pad = (-Kt) % 128
            p = np.concatenate((prod, np.zeros((prod.shape[0], pad), dtype=f32)), 1).reshape(prod.shape[0], -1, 4, 32)
            parts = np.cumsum(p.transpose(0, 2, 1, 3).reshape(prod.shape[0], 4, -1), axis=2, dtype=f32)[:, :, -1]
            z[b] = ((parts[:, 0] + parts[:, 1]) + parts[:, 2]) + parts[:, 3]
    z = z + (o.b_ih.numpy().astype(f32) + o.b_hh.numpy().astype(f32))[None, :]
    hs = o.hs
    sig = lambda v: (f32(1.0) / (f32(1.0) + np.exp(-v, dtype=f32))).astype(f32)
    i, f, g, og = sig(z[:, :hs]), sig(z[:, hs:2 * hs]), np.tanh(z[:, 2 * hs:3 * hs], dtype=f32), sig(z[:, 3 * hs:])
    cn = (f * o.c_prev.numpy().astype(f32) + i * g).astype(f32)
    hn = (og * np.tanh(cn, dtype=f32)).astype(f32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(F64)
    return _buffers(o, t(hn), t(cn), torch.cat((t(i), t(f), t(g), t(og)), 1))


def cell_ratios(o, ref, got, signed=False):
    """{check: measured / bound}; every value must lie in [0, 1] (the signed statistic in [-1, 1]).  A NaN result, a changed
    c buffer or a touched guard row gives inf."""
    out = {}
    for name, val, want, bound in (("h", got["h"], ref.h, ref.bh), ("c", got["c"], ref.c, ref.bc)):
        val = val.to(F64)
        if not bool(torch.isfinite(val).all()):
            out[name + " err/bound"] = math.inf
            continue
        err = (val - want).abs()
        out[name + " err/bound"] = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    if got.get("gates") is not None:
        gt = got["gates"].to(F64)
        err = gt - ref.gates
        out["gates err/bound"] = float((err.abs() / ref.bg).max()) if bool(torch.isfinite(gt).all()) else math.inf
        if signed:
            st, n = signed_stat(err, ref.gates, ref.bg)
            out["gates signed bias"] = st
    out["c_prev untouched"] = 0.0 if torch.equal(got["c_prev_after"].to(torch.float32), ref.c_prev) else math.inf
    guards = torch.cat((got["h_guard"].reshape(-1), got["c_guard"].reshape(-1))).to(F64)
    out["guard rows untouched"] = 0.0 if bool((guards == SENTINEL).all()) else math.inf
    return out


def passes(rs):
    return all(abs(r) <= 1.0 and r == r for r in rs.values())


# ---- the action head -------------------------------------------------------------------------------------------------------------
def _blocked_logits(logit, blocked):
    l = logit.to(F64).clone()
    if blocked is not None:
        l[blocked.bool()] = -math.inf
    return l


class HeadRef(object):
    pass


def head_reference(logit, target, blocked=None, ignore_index=-100):
    """float64 loss / dlogit (for an upstream gradient of 1) and their bounds."""
    l = _blocked_logits(logit, blocked)
    B, A = l.shape
    counted = target != ignore_index
    n = int(counted.sum())
    m = l.max(1).values
    lse = torch.log(torch.exp(l - m[:, None]).sum(1)) + m
    tsafe = torch.where(counted, target, torch.zeros_like(target))
    lt = l.gather(1, tsafe[:, None])[:, 0]
    rows = lse - lt
    r = HeadRef()
    r.n = n
    r.loss = float(rows[counted].sum() / n) if n else math.nan
    finite = torch.isfinite(rows) & counted
    rb = 2.0 ** -20 + 2.0 ** -22 * (m.abs() + lt.abs() + rows.abs())
    r.loss_bound = (float(rb[finite].sum() / n) + 2.0 ** -24 * (n / 16.0 + 17.0) * float(rows[finite].abs().sum() / n)) if n else 0.0
    p = torch.softmax(l, 1)
    onehot = torch.zeros(B, A, dtype=F64)
    onehot[torch.arange(B), tsafe] = 1.0
    d = torch.where(counted[:, None], (p - onehot) / max(n, 1), torch.zeros_like(p))
    if blocked is not None:
        d[blocked.bool()] = 0.0
    r.dlogit, r.dlogit_bound = d, 2.0 ** -20 + 2.0 ** -22 * d.abs()
    return r


def head_argmax(logit, blocked=None):
    """Lowest index of the row maximum of the blocked logits."""
    l = _blocked_logits(logit, blocked)
    return (l == l.max(1, keepdim=True).values).to(torch.int64).argmax(1)


def sample_u(seed, B):
    """u[row] = (hash32(seed, row) >> 8) * 2^-24."""
    return (hash32(int(seed) & 0xFFFFFFFF, np.arange(B)) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def head_sample(logit, blocked, seed, margin=1e-5):
    """float64 inverse CDF in index order -> (a int64 [B], safe bool [B]): the smallest a with cdf[a] > u; safe = u farther
    than `margin` from every CDF step (a row where fp32 rounding may legitimately pick the neighbour otherwise)."""
    l = _blocked_logits(logit, blocked)
    cdf = torch.softmax(l, 1).cumsum(1)
    u = torch.from_numpy(sample_u(seed, l.shape[0]))
    a = (cdf <= u[:, None]).sum(1).clamp(max=l.shape[1] - 1)
    safe = ((cdf - u[:, None]).abs() > margin).all(1)
    return a, safe


def head_case(B, A, seed, block_p=0.3):
    """Random logits, a ragged `blocked` with at least one open entry per row, targets with every fourth row ignored."""
    g = torch.Generator().manual_seed(seed)
    logit = torch.randn(B, A, generator=g) * 2.0
    blocked = torch.rand(B, A, generator=g) < block_p
    blocked[torch.arange(B), torch.randint(0, A, (B,), generator=g)] = False
    target = torch.randint(0, A, (B,), generator=g)
    target[::4] = -100
    return logit, target, blocked


SAMPLE_CASE, SAMPLE_SEEDS = (64, 6, 77), tuple(range(1000, 1008))   # 64 rows x 8 seeds (host: at most 1 % of them left out)
