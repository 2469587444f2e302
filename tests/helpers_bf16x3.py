"""The bf16x3 arithmetic (csrc/bf16x3_path.hip) in pure torch on the CPU, and the two checks a bf16x3 result must pass.

Every fp32 operand element is split into two bf16 terms, x ~ hi + lo with hi = bf16_rne(x), lo = bf16_rne(x - hi), and a
product is formed as hi.hi + hi.lo + lo.hi with fp32 accumulation.  Each split leaves a residue of at most 2^-16 |x|
(u = 2^-8 twice), so to first order

    |a.b - (ah.bh + ah.bl + al.bh)| <= 3 * 2^-16 * |a||b|          (the dropped lo.lo term, and one residue per operand)

(A) pins the arithmetic: the result against act(alpha * emulated + bias) + R within 2e-5 * (1 + max|z|), the tolerance
    tests/test_gpu_fp32.py gives fp32 accumulation order.  A single bf16 product or a dropped cross term misses it.
(B) is the accuracy contract: the result against the fp64 value within 1.13 * bound + (A)'s tolerance; 1.13 is the Lipschitz
    constant of erf-GELU (tanh and the identity have 1).
"""
import torch

from helpers import check_close

U16 = 2.0 ** -16
TOL_ORDER = 2e-5          # fp32 accumulation order, per unit of (1 + max|z|)
LIP_GELU = 1.13

# (M, N, K, act, residual, w_is_kn): the six shapes of test_linear_f32_matches_fp64 with their settings, then the tails
GEMM_CASES = [(300, 200, 2182, 0, False, False), (77, 768, 768, 1, False, False), (513, 130, 64, 2, True, False),
              (228, 64, 228, 0, False, True), (37, 37, 64, 0, True, False), (1000, 3072, 768, 1, True, False),
              (5, 7, 1, 0, False, False), (64, 64, 31, 1, True, False), (64, 64, 33, 2, False, False),
              (1, 1009, 768, 0, False, False), (129, 37, 2182, 1, True, False), (228, 64, 228, 2, True, True)]
ALPHA = 0.5


def split_rne(x):
    """x fp32 -> (hi, lo) fp32 tensors holding bf16 values: hi = bf16_rne(x), lo = bf16_rne(x - hi)."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def three_terms(a, w, dtype=torch.float64, terms=("lh", "hl", "hh"), lo_zero=False):
    """sum of the named products of the splits of a [M, K] and w [N, K], evaluated in `dtype`, in the kernel's order."""
    ah, al = (t.to(dtype) for t in split_rne(a))
    wh, wl = (t.to(dtype) for t in split_rne(w))
    if lo_zero:
        al, wl = torch.zeros_like(al), torch.zeros_like(wl)
    parts = {"lh": (al, wh), "hl": (ah, wl), "hh": (ah, wh), "ll": (al, wl)}
    out = None
    for t in terms:
        p = parts[t][0] @ parts[t][1].t()
        out = p if out is None else out + p
    return out


def emulated(a, w):
    """hi.hi + hi.lo + lo.hi of a [M, K] and w [N, K] in fp64."""
    return three_terms(a, w)


def bound(a, w, alpha=1.0):
    """3 * 2^-16 * |alpha| * (|a| @ |w|^T), per element, fp64."""
    return 3.0 * U16 * abs(alpha) * (a.double().abs() @ w.double().abs().t())


def _epilogue(prod, bias, res, act, alpha):
    z = prod * alpha
    if bias is not None:
        z = z + bias.double()
    if act == 1:
        z = torch.nn.functional.gelu(z)
    elif act == 2:
        z = torch.tanh(z)
    if res is not None:
        z = z + res.double()
    return z


def gemm_inputs(M, N, K, res, kn, seed=None):
    """The inputs of test_linear_f32_matches_fp64: a [M, K], w ([K, N] when kn), bias [N], residual or None."""
    g = torch.Generator().manual_seed(M + N + K if seed is None else seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn((K, N) if kn else (N, K), generator=g) * 0.05
    b = torch.randn(N, generator=g) * 0.1
    r = torch.randn(M, N, generator=g) if res else None
    return a, w, b, r


def gemm_ratios(got, a, w_nk, bias=None, res=None, act=0, alpha=1.0):
    """-> (worst |got - want_A| / tol_A, worst |got - z| / (1.13 * bound + tol_A)): both must be <= 1.  w_nk is [N, K]."""
    got = got.detach().double().cpu()
    z = _epilogue(a.double() @ w_nk.double().t(), bias, res, act, alpha)
    zA = _epilogue(emulated(a, w_nk), bias, res, act, alpha)
    tol = TOL_ORDER * (1.0 + float(z.abs().max()))
    ra = float(((got - zA).abs() / tol).max())
    rb = float(((got - z).abs() / (LIP_GELU * bound(a, w_nk, alpha) + tol)).max())
    return ra, rb


def check_gemm(name, got, a, w_nk, bias=None, res=None, act=0, alpha=1.0):
    """Assert (A) and (B) on a finite result; the measured fractions of the two tolerances are printed and recorded."""
    assert bool(torch.isfinite(got).all()), name + ": non-finite result"
    ra, rb = gemm_ratios(got, a, w_nk, bias, res, act, alpha)
    check_close(name + " (A) / tolerance", ra, 0.0, 1.0)
    check_close(name + " (B) / bound", rb, 0.0, 1.0)
    return ra, rb


def sixteen_bit_values(shape, seed):
    """Asymmetric fp32 values that carry exactly 16 significant bits (odd 16-bit mantissa, random sign, scaled by 2^-12)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(2 ** 15, 2 ** 16, shape, generator=g) | 1
    s = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (m * s).float() * 2.0 ** -12


def attention_reference(qkv, B, S, nh, ext, hm):
    """fp64 attention on the packed projection and the per-element bounds of a bf16x3 result.
    scores:        delta = 3 * 2^-16 * (|q| @ |k|^T) / 8
    probabilities: p * (exp(2 * max_row delta) - 1) + 2e-6     (a row's softmax moves by at most that under score errors <= delta)
    context:       sum |dp||v| + 3 * 2^-16 * sum p|v| + 2e-5
    -> (probs [B, nh, S, S], ctx [B*S, H], probs bound, ctx bound)"""
    H = nh * 64
    sp = lambda t: t.double().view(B, S, nh, 64).permute(0, 2, 1, 3)
    q, k, v = sp(qkv[:, :H]), sp(qkv[:, H:2 * H]), sp(qkv[:, 2 * H:])
    sc = q @ k.transpose(-1, -2) / 8.0 + (ext if torch.is_tensor(ext) else 0.0)
    pr = torch.softmax(sc, -1) * hm.double().view(1, nh, 1, 1)
    ctx = pr @ v
    delta = 3.0 * U16 * (q.abs() @ k.abs().transpose(-1, -2)) / 8.0
    dp = pr * torch.expm1(2.0 * delta.amax(-1, keepdim=True)) + 2e-6
    dc = dp @ v.abs() + 3.0 * U16 * (pr @ v.abs()) + 2e-5
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, H)
    return pr, flat(ctx), dp, flat(dc)
