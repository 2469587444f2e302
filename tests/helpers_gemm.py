"""fp64 reference, CPU rounding model, derived per-element bounds, exact constructions and the case table of the bf16 NT GEMM
family (vt_linear_bf16_ex, vt_linear_lnres_bf16, vt_linear_ln_bf16, vt_linear_splitk_bf16).

Everything here is plain torch / numpy on the CPU in float64, taken from the bf16-, fp16- or fp32-exact inputs.
tests/test_host_gemm_reference.py proves without a GPU that the bounds accept the minimal implementation and reject a table of
subtly wrong ones; tests/test_gpu_gemm_conformance.py holds the HIP kernels to the same bounds.  No bound below was chosen by
looking at a kernel's output.

REFERENCE FORMS (one function per entry point, restating include/visitron_hip.h and csrc/gemm_common.hpp)
  linear               y = [keep s] act(A W^T + b) [+ r | * r];  s = the fp32 value 1.0f / (1.0f - p) (common.hpp, vt_make_drop),
                       keep from the Python restatement of vt_site_seed / vt_hash32 / vt_keep below (never from the GPU);
                       second output z = A W^T + b, or gelu'(z) under GELU.
  linear, residual_ln  r = (v - mean) rstd gamma + beta with v fp16 (GemmArgs::r_mean).
  linear_ln mode 1     act(rstd_r (A W'^T - mean_r g) + h)
  linear_ln mode 2     v' = A W^T + cb + gamma ((Rs - mean_r) rstd_r): the fp16 stream and the bf16 copy are both rounded from the
                       fp32 v' (gemm_v7_ln_epilogue.hpp: pack_f16x2 and pack_bf16x2 of the same v[]), stats_out[p][row] = (sum,
                       sum of squares) of the UNROUNDED v' over the 128-column slice p.
                       For both modes mean_r, var_r = max(q_r - mean_r^2, 0) and rstd_r = 1 / sqrt(var_r + eps) are formed in
                       float64 from the given fp32 partial statistics (inputs), as the epilogue forms them.
  linear_splitk        bf16(A W^T)

BOUND, per element.  u_out = 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32):

    |got - y| <= u_out |y| + (1 + u_out) E
    F   = (K + 8) 2^-23 (sum_k |a_k w_k| + |b|)       fp32 accumulation in ANY order, one ulp per add (MFMA's inner sum is not
                                                       documented as round to nearest: twice the RN bound 2^-24); + 8: the bias
                                                       add, the dropout scale, split-K / shared-tile plane sums
    E   = s L_act F + eps_act(z)                       plain / dropout (s = 1 without; dropout is used with act = none only)
          a bf16 / fp16 residual is exact and the final add's rounding is inside u_out |y|
    ACT_MUL              E = |r| F
    rebuilt LayerNorm    E += 2^-21 ((|v| + |mean|) rstd |gamma| + |beta|)        four fp32 operations
    L_act, eps_act       none 1, 0
                         GELU 1.13 (sup |gelu'| = 1.129); the erf form |z| 2^-20 (Abramowitz-Stegun 7.1.26, 1.5e-7 on erf, times
                         |z| / 2, plus v_rcp / v_exp ulps); the polynomial form min(1.2e-4, 2.6e-5 |z|)
                         (tests/test_host_round2.py::test_gelu_polynomial_of_the_epilogues_meets_its_stated_error)
                         tanh 1, 2^-20 (1 + |z|)  (1 - 2 / (exp(2 z) + 1): the exponent's argument error is relative to |z|)
    second output        plain  u |z| + (1 + u) F
                         gelu'  u |gelu'(z)| + (1 + u) (0.8 F + 2^-20 (1 + |z|))   sup |gelu''| = 0.798

  The worst-case F is knowingly slack (real fp32 sums err like sqrt K, not K): it catches arithmetic done in the wrong precision
  or with a wrong operand wherever |y| is small; structure (a dropped / duplicated / misplaced K-step, tile, row or column) is the
  exact constructions' job.

DEFERRED LAYERNORM.  kappa_r = (q_r + mean_r^2) / (var_r + eps) (the cancellation of q - mean^2 in fp32), rho_r = 2^-22 kappa_r + 2^-21:

    mode 1 pre-activation  E = rstd F + (rho + 2^-20) (|rstd P| + |mean rstd g|) + 2^-22 |h|,  then L_act / eps_act as above
    mode 2 v'              E = F + (rho + 2^-20) |gamma| (|Rs| + |mean|) rstd + 2^-22 |cb|
    mode 2 statistics      |sum err| <= sum_128 E + 130 2^-24 sum_128 |v'|
                           |sq err|  <= sum_128 (2 |v'| E + E^2) + 130 2^-24 sum_128 v'^2

SIGNED BIAS  helpers_attention.signed_stat: mean(err sign(y) / bound) over N >= 1e5 elements within 6 / sqrt(N) of zero.  It
presumes roundings of zero mean, which fails where the references pile up between two grid points: the saved gelu'(z) is flat at
its extremes (1.129, -0.129) and lies in (1, 1 + 2^-8) for z > 2.6, where it always rounds down.  The statistic is not applied to
that output (linear_reference); every other bf16 / fp16 output of a case with N >= 1e5 elements gets it.

EXACT CONSTRUCTIONS  a in [-4, 4], w in [-2, 2], b in [-8, 8], r in [-16, 16], integers, dropout at p = 0.5 (scale 2, threshold
32 768): every partial sum in any order is an integer below 2^24, so the fp32 output must EQUAL the float64 reference, the bf16 /
fp16 output its single rounding, dropped elements the residual.

WHICH GELU FORM A KERNEL RUNS (gelu_form):
  polynomial  the straight-line epilogue of the 256x256-tile kernels (families V7, V8, V8_SHARED; bf16 / fp16 output, N % 64 == 0, no
              row remap: csrc/gemm_v7.hip launch_v7 / launch_v8 `fast`) WITHOUT a second output: csrc/gemm_v7_kernels.hpp, V7_SLAB,
              `else if (ACT == ACT_GELU) { ... gelu_poly4` ; and the linear_ln epilogue: csrc/gemm_v7_ln_epilogue.hpp, V7_LN_SLAB,
              `if (ACT == ACT_GELU) z = gelu_poly4(z);`
  erf         everything else: csrc/gemm_common.hpp apply_act (`if (ACT == ACT_GELU) return gelu_erf(x);`), epi_row_values
              (gelu_erf_both2), V7_SLAB with a second output (gelu_erf_both4); variant 33's epilogue kernel runs epi_row_direct.
"""
import functools
import math

import numpy as np
import torch

from helpers_attention import bf16_trunc, bf16r, signed_stat  # noqa: F401  (signed_stat: re-exported)

F64 = torch.float64
U_OUT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}
LN_EPS = 1e-12
DROP_P, DROP_P_EXACT = 0.1, 0.5


# ---- rounding ---------------------------------------------------------------------------------------------------------------
def f16r(x):
    return x.to(torch.float32).clamp(-65504.0, 65504.0).to(torch.float16).to(F64)


def f16_trunc(x):
    h = x.to(torch.float32).clamp(-65504.0, 65504.0).to(torch.float16)
    over = h.to(F64).abs() > x.abs()
    bits = h.view(torch.int16) - over.to(torch.int16)      # sign-magnitude: one step towards zero
    return bits.view(torch.float16).to(F64)


def f32r(x):
    return x.to(torch.float32).to(F64)


def round_out(x, fmt, trunc=False):
    if fmt == "f32":
        return f32r(x)
    if fmt == "f16":
        return f16_trunc(x) if trunc else f16r(x)
    return bf16_trunc(x) if trunc else bf16r(x)


# ---- the dropout hash of csrc/common.hpp in numpy ----------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def site_seed(step_seed, site):
    x = (int(step_seed) + 0x9E3779B97F4A7C15 * (int(site) + 1)) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x >> 32


def hash32(seed, idx):
    m = np.uint64(0xFFFFFFFF)
    x = ((np.asarray(idx, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B1)) & m
    x ^= x >> np.uint64(15)
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0x85EBCB)) & m
    x ^= x >> np.uint64(12)
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0xC2B2AF)) & m
    x ^= x >> np.uint64(16)
    return x


def drop_thresh(p):
    return int(np.float32(p) * np.float32(65536.0)) if p > 0 else 0


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def keep_mask(n, drop, first=0, seed_offset=0):
    """bool numpy [n]: vt_keep of elements first .. first + n - 1 of site drop = (p, step seed, site)."""
    p, step_seed, site = drop
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(first)) & np.uint64(0xFFFFFFFF)
    seed = (site_seed(step_seed, site) + seed_offset) & 0xFFFFFFFF
    h = hash32(seed, (idx >> np.uint64(1)) & np.uint64(0xFFFFFFFF))
    field = np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return field >= np.uint64(drop_thresh(p))


# ---- activations in float64 ----------------------------------------------------------------------------------------------------
def gelu64(z):
    return 0.5 * z * (1.0 + torch.special.erf(z / math.sqrt(2.0)))


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.special.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gelu_tanh64(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def act_terms(act, z, gelu_form):
    """(act(z), L_act, eps_act(z))"""
    if act == "gelu":
        eps = z.abs() * 2.0 ** -20 if gelu_form == "erf" else torch.clamp(2.6e-5 * z.abs(), max=1.2e-4)
        return gelu64(z), 1.13, eps
    if act == "tanh":
        return torch.tanh(z), 1.0, 2.0 ** -20 * (1.0 + z.abs())
    return z, 1.0, torch.zeros_like(z)


# ---- epilogue sets of `linear` ---------------------------------------------------------------------------------------------------
EPILOGUES = {
    "plain": {},
    "bias": {"bias": True},
    "bias_c2": {"bias": True, "c2": True},                                        # the plain second output z
    "bias_res": {"bias": True, "res": "bf16"},
    "bias_res16": {"bias": True, "res": "f16", "out": "f16"},
    "drop_res": {"bias": True, "res": "bf16", "drop": True},
    "gelu": {"bias": True, "act": "gelu"},
    "gelu_c2": {"bias": True, "act": "gelu", "c2": True},
    "tanh_f32": {"bias": True, "act": "tanh", "out": "f32"},
    "f32": {"bias": True, "out": "f32"},
    "mul": {"act": "mul", "res": "bf16"},
    "lnres": {"bias": True, "res": "ln"},
    "lnres_drop16": {"bias": True, "res": "ln", "drop": True, "out": "f16"},      # the training layer's own residual GEMM
    "drop_res_f32": {"bias": True, "res": "bf16", "drop": True, "out": "f32"},   # exact constructions only
}
ALL_EPIS = ("plain", "bias", "bias_c2", "bias_res", "bias_res16", "drop_res", "gelu", "gelu_c2", "tanh_f32", "f32", "mul", "lnres",
            "lnres_drop16")
FAST_EPIS = ("plain", "bias", "bias_c2", "bias_res", "bias_res16", "drop_res", "gelu", "gelu_c2", "mul", "lnres", "lnres_drop16")
FEW_EPIS = ("plain", "bias_res", "drop_res", "gelu")
EXACT_EPIS = ("f32", "bias_res", "bias_res16", "mul", "drop_res", "drop_res_f32")


def epi(name):
    e = {"bias": False, "res": None, "act": "none", "out": "bf16", "c2": False, "drop": False}
    e.update(EPILOGUES[name])
    return e


# ---- cases -----------------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, name, M, N, K, why, epis=ALL_EPIS, exact=EXACT_EPIS, lda=None, ldc=None, grp=(0, 0), families=None, mtn=None,
                 only=None, auto=False):
        self.name, self.M, self.N, self.K, self.why = name, M, N, K, why
        self.lda = K if lda is None else lda
        self.ldc = (N + 7) // 8 * 8 if ldc is None else ldc
        self.grp = grp
        self.epis = tuple(e for e in epis if not (e.startswith("lnres") and (N % 16 or grp[0])))
        self.exact = tuple(exact)
        self.families, self.mtn, self.only, self.auto = families, mtn, only, auto

    @property
    def out_rows(self):
        gr, gs = self.grp
        return self.M if not gr else ((self.M - 1) // gr) * gs + (self.M - 1) % gr + 1

    def out_row_index(self):
        m = torch.arange(self.M)
        gr, gs = self.grp
        return m if not gr else (m // gr) * gs + m % gr

    def __repr__(self):
        return self.name


V78 = ("V7", "V8", "V8_SHARED")


def tail_split_rows(cus, N=512):
    """(M, M1) of the tail-split case: two column tiles, cus + 4 tiles of 256x256 -> one full round and a last round of 4 tiles
    (at most half full); M1 = the rows of the full round (vt_gemm_dispatch), the last row tile 100 rows short."""
    tn = (N + 255) // 256
    tm = cus // tn + 2
    M = tm * 256 - 100
    T = tm * tn
    Fr = T // cus
    M1 = (Fr * cus) // tn * 256
    assert T > cus and 0 < T - Fr * cus and 2 * (T - Fr * cus) <= cus and 0 < M1 < M
    return M, M1


def cases(cus=256, host=False):
    """The case table shared by the host and the GPU file.  cus: the device's compute units (the persistent and tail-split shapes
    depend on it); host: the large persistent-only shapes shrink to N = 256, K = 64."""
    out = [
        Case("1x8x64", 1, 8, 64, "the smallest legal call; one K-step"),
        Case("130x36x128", 130, 36, 128, "N tail inside the first 64-column block; the element-wise epilogue path"),
        Case("200x201x128", 200, 201, 128, "odd N: odd dropout start index per row (vt_drop_run's element-wise branch), a 16-column "
             "block straddling N", ldc=208),
        Case("257x264x192", 257, 264, 192, "one row and eight columns past a 256x256 tile; three K-steps (odd)"),
        Case("300x520x768", 300, 520, 768, "the signed-bias case (156 000 elements); partial last tile of every tile width"),
        Case("260x392x3072", 260, 392, 3072, "48 K-steps: every ring wraps many times; a strided operand", lda=3072 + 64,
             epis=("plain", "bias_c2", "bias_res", "bias_res16", "drop_res", "gelu", "gelu_c2", "f32", "mul", "lnres", "lnres_drop16")),
    ]
    for mtn in (8, 7, 6, 5, 4):
        out.append(Case("mtail%d_%dx384x128" % (mtn, 32 * mtn * 3 + 5), 32 * mtn * 3 + 5, 384, 128,
                        "M tail of the %d-row tile; a last 256-column tile holding 128 columns" % (32 * mtn), mtn=mtn))
    out += [
        Case("640x768x768", 640, 768, 768, "split-K with the whole epilogue (variant 33): four copies of nine tiles", families=("SPLITK_EPI",),
             epis=("plain", "bias", "bias_c2", "bias_res", "bias_res16", "drop_res", "gelu", "gelu_c2", "f32", "mul", "lnres", "lnres_drop16")),
        Case("300x264x1024", 300, 264, 1024, "split-K with the whole epilogue: five copies, N tail in the epilogue kernel", families=("SPLITK_EPI",)),
        Case("1534x768x3072", 1534, 768, 3072, "shared tiles (31, 32): every tile shared; 48 K-steps on every 256x256-tile kernel",
             families=V78 + ("SPLITK_EPI",), epis=FEW_EPIS, exact=("bias_res", "drop_res")),
        Case("300x256x192", 300, 256, 192, "shared tiles: K too short to share", families=("V8_SHARED",), epis=FAST_EPIS),
        Case("remap21x128x64", 21, 128, 64, "row remap (grp_rows 7, grp_stride 12) with a partial group", grp=(7, 12),
             epis=("plain", "bias_res", "drop_res", "gelu_c2", "f32"), exact=("f32", "bias_res", "drop_res")),
    ]
    for mtn in (8, 7, 6, 5, 4):
        M = 32 * mtn * (cus + 5)
        out.append(Case("persistent%d_%dx256x%d" % (mtn, M, 64 if host else 128), M, 256, 64 if host else 128,
                        "several tiles per persistent workgroup (%d-row tiles): the pipeline runs across tile boundaries" % (32 * mtn),
                        mtn=mtn, families=("V8", "V8_SHARED"), epis=(), exact=("bias_res", "drop_res")))
    M, _ = tail_split_rows(cus)
    out.append(Case("tailsplit_%dx512x128" % M, M, 512, 128, "the tail launch: dropout pair index across the two launches", epis=(),
                    exact=("drop_res", "drop_res_f32"), auto=True, only=()))
    return out


LN_SHAPES = ((384, 768), (768, 384))      # (row length of A = K, N) ... and the reverse


def ln_cases():
    """linear_ln: [32 mtn 2 + 37, K] x N for every tile height, both shapes."""
    return [(32 * mtn * 2 + 37, K, N, mtn) for mtn in (8, 7, 6, 5, 4) for (K, N) in LN_SHAPES]


# ---- variants: what runs under a variant's own name ----------------------------------------------------------------------------
def variant_table():
    from visitron_amd import ops

    return ops.GEMM_VARIANTS


def production_variants():
    return tuple(v for v, e in variant_table().items() if e["family"] not in ("V10", "V11", "V12"))


def splitk_epi_copies(M, N, K, cus):
    """launch_splitk_epi's ks (csrc/gemm_bf16.hip) and whether the planes fit one workspace region (launch_splitk_tiles)."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    nk = K >> 6
    ks = int(float(np.sqrt(np.float32(16.0) * np.float32(nk) / np.float32(tiles))) + 0.5)
    ks = min(ks, cus // tiles, nk // 3, 16)
    fits = ks * tiles * (256 * 64 * 16) <= 64 * (1 << 20)      # V8_SK_PART_BYTES per copy and tile, one region of 64 MiB
    return ks, fits


def tile_of(variant):
    """(tile height, tile width) of a variant's own kernel."""
    e = variant_table()[variant]
    fam = e["family"]
    if fam in ("V2_RING2", "V2_RING3", "V6"):
        return 128, 128
    if fam == "V4_192":
        return 256, 192
    return (32 * e["mtn"] if fam in V78 else 256), 256


def is_fast(case, ep):
    """the straight-line epilogue of the 256x256-tile kernels (launch_v7 / launch_v8)"""
    return ep["out"] != "f32" and case.N % 64 == 0 and not case.grp[0]


def runnable(variant, case, epi_name, cus=256):
    """Does `variant` run this combination with its OWN kernel?  Restates the library's substitution rules:
      BF16_IO_ONLY with an fp16 operand runs the default kernel (vt_gemm_dispatch);
      28 .. 30 run as their twins (launch_v8: the stream-K region exists on 160- and 128-row tiles only), and so do 31, 32 where
      the epilogue is not the straight-line one;
      a 256x256-tile variant on shorter tiles runs the 256-row kernel (variants 15 / 16) where the epilogue is not the straight-line
      one or the activation is tanh, and variant 16 runs a rebuilt-LayerNorm residual on 224-row tiles (as 18);
      33 returns VT_ERR_UNSUPPORTED when launch_splitk_epi's ks < 2 or the planes do not fit the workspace."""
    e, ep = variant_table()[variant], epi(epi_name)
    fam, mtn = e["family"], e["mtn"]
    if case.only is not None and variant not in case.only:
        return False
    if case.families is not None and fam not in case.families:
        return False
    if case.mtn is not None and fam in V78 and mtn != case.mtn:
        return False
    if case.mtn is not None and fam not in V78 and case.mtn != 8:
        return False
    if "BF16_IO_ONLY" in e["flags"] and (ep["res"] in ("f16", "ln") or ep["out"] == "f16"):
        return False
    if fam in V78:
        fast = is_fast(case, ep) and ep["act"] != "tanh"
        if fam == "V8_SHARED" and (mtn > 5 or not fast):
            return False
        if mtn < 8 and not fast:
            return False
        if fam == "V8" and mtn == 8 and ep["res"] == "ln" and fast:
            return False
    if fam == "SPLITK_EPI":
        ks, fits = splitk_epi_copies(case.M, case.N, case.K, cus)
        return ks >= 2 and fits
    return True


def splitk33_supported(case, cus):
    ks, fits = splitk_epi_copies(case.M, case.N, case.K, cus)
    return ks >= 2 and fits


def ln_runnable(variant):
    """linear_ln: a variant without LN_EPILOGUE runs 16 (vt_gemm_ln_dispatch); 28 .. 30 run as their twins (launch_ln)."""
    e = variant_table()[variant]
    return "LN_EPILOGUE" in e["flags"] and not (e["family"] == "V8_SHARED" and e["mtn"] > 5)


def gelu_form(variant, case, epi_name):
    e, ep = variant_table()[variant], epi(epi_name)
    return "poly" if (e["family"] in V78 and is_fast(case, ep) and not ep["c2"]) else "erf"


# ---- operands ------------------------------------------------------------------------------------------------------------------
class Operands(object):
    """a [M, K], w [N, K], b [N], residuals [M, N] (logical rows), the rebuilt-LayerNorm vectors, keep [M, N]; P = a w^T and its
    absolute-value twin, all float64 of bf16- / fp16- / fp32-exact values."""


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (1 << 31)


@functools.lru_cache(maxsize=2)
def operands(case, exact=False):
    o = Operands()
    g = torch.Generator().manual_seed(_seed(case.name) + (7 if exact else 0))
    M, N, K = case.M, case.N, case.K
    o.case, o.M, o.N, o.K, o.exact = case, M, N, K, exact
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(torch.float32)
        a, w = ri(-4, 4, M, K), ri(-2, 2, N, K)
        o.b, o.r_bf16 = ri(-8, 8, N).to(F64), ri(-16, 16, M, N).to(F64)
        o.r_f16 = o.r_mul = o.r_bf16
        o.P = (a @ w.t()).to(F64)            # integers below 2^24: float32 torch is exact (the host test proves it)
        o.Pabs = (a.abs() @ w.abs().t()).to(F64)
        o.a, o.w = a.to(F64), w.to(F64)
        o.drop = (DROP_P_EXACT, 1234 + _seed(case.name) % 1000, 9)
    else:
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
        o.a, o.w = bf16r(rn(M, K)), bf16r(rn(N, K) * (1.5 / math.sqrt(K)))
        o.b = (rn(N) * 0.5).to(F64)
        o.r_bf16, o.r_f16, o.r_mul = bf16r(rn(M, N)), f16r(rn(M, N)), bf16r(0.5 + 0.5 * rn(M, N))
        v = f16r(rn(M, N) * (0.5 + torch.rand(M, 1, generator=g)) + 0.3 * rn(M, 1))
        o.v = v
        o.mean = f32r(v.mean(-1))
        o.rstd = f32r(1.0 / torch.sqrt(v.var(-1, unbiased=False) + LN_EPS))
        o.gamma, o.beta = f32r(1.0 + 0.2 * rn(N)), f32r(0.1 * rn(N))
        o.P = o.a @ o.w.t()
        o.Pabs = o.a.abs() @ o.w.abs().t()
        o.drop = (DROP_P, 77 + _seed(case.name) % 1000, 3)
    o.keep = torch.from_numpy(keep_mask(M * N, o.drop)).view(M, N)
    return o


# ---- `linear`: reference, bound, model ---------------------------------------------------------------------------------------------
LINEAR_MUTANTS = ("last_k_dropped", "one_product_dropped", "first_k_step_of_second_split_dropped", "bias_from_next_column",
                  "bias_missing_on_column_tail", "residual_row_clamped_on_row_tail", "output_truncated", "rounded_before_residual",
                  "residual_added_before_dropout", "dropout_scale_from_threshold", "dropout_pair_index_off_by_one_in_second_launch",
                  "gelu_tanh_form", "gelu_grad_of_rounded_preactivation", "row_remap_ignores_stride")
LN_MUTANTS = ("ln_stats_slice_dropped", "ln_var_unclamped_negative", "ln_mode2_bf16_copy_from_fp16", "stats_out_of_rounded_stream")
MUTANTS = LINEAR_MUTANTS + LN_MUTANTS


def mutant_applies(mutant, case, epi_name):
    ep = epi(epi_name)
    add_res = ep["res"] is not None and ep["act"] != "mul"
    return {
        "last_k_dropped": True, "one_product_dropped": True,
        "first_k_step_of_second_split_dropped": case.K >= 128,
        "bias_from_next_column": ep["bias"] and case.N > 1,
        "bias_missing_on_column_tail": ep["bias"] and case.N % 16 != 0,
        "residual_row_clamped_on_row_tail": ep["res"] is not None and case.M % 16 != 0 and case.M > 16,
        "output_truncated": ep["out"] != "f32",
        "rounded_before_residual": add_res,
        "residual_added_before_dropout": ep["drop"],
        "dropout_scale_from_threshold": ep["drop"],
        "dropout_pair_index_off_by_one_in_second_launch": ep["drop"] and case.auto,
        "gelu_tanh_form": ep["act"] == "gelu",
        "gelu_grad_of_rounded_preactivation": ep["act"] == "gelu" and ep["c2"],
        "row_remap_ignores_stride": bool(case.grp[0]) and ep["res"] is not None,
    }[mutant]


def _linear_values(o, ep, mutant=None, M1=None):
    """Unrounded (y, y2, z, parts) in float64; `mutant` changes one thing."""
    case, M, N, K = o.case, o.M, o.N, o.K
    P = o.P
    if mutant == "last_k_dropped":
        P = P - o.a[:, -1:] * o.w[:, -1][None, :]
    if mutant == "one_product_dropped":
        k = K // 3
        prod = o.a[:, k].abs()[:, None] * o.w[:, k].abs()[None, :]
        if ep["drop"]:
            prod = prod * o.keep.to(F64)          # (a product of a dropped element is not seen by anybody)
        m, n = divmod(int(prod.argmax()), N)
        P = P.clone()
        P[m, n] -= o.a[m, k] * o.w[n, k]
    if mutant == "first_k_step_of_second_split_dropped":
        c = 64 * (((K // 64) + 1) // 2)
        P = P - o.a[:, c:c + 64] @ o.w[:, c:c + 64].t()
    b = o.b if ep["bias"] else torch.zeros(N, dtype=F64)
    if mutant == "bias_from_next_column":
        b = torch.roll(b, -1)
    if mutant == "bias_missing_on_column_tail":
        b = b.clone()
        b[16 * (N // 16):] = 0
    z = P + b
    if ep["act"] == "gelu" and mutant == "gelu_tanh_form":
        t = gelu_tanh64(z)
    else:
        t = act_terms(ep["act"], z, "erf")[0]
    y2 = None
    if ep["c2"]:
        y2 = gelu_grad64(bf16r(z) if mutant == "gelu_grad_of_rounded_preactivation" else z) if ep["act"] == "gelu" else z
    r = None
    if ep["res"] is not None:
        r = {"bf16": o.r_mul if ep["act"] == "mul" else o.r_bf16, "f16": o.r_f16, "ln": getattr(o, "v", None)}[ep["res"]]
        rows = torch.arange(M)
        if mutant == "residual_row_clamped_on_row_tail":
            rows = torch.clamp(rows, max=16 * (M // 16) - 1)
        if mutant == "row_remap_ignores_stride":     # the operand read at row m of the physical buffer instead of its output row
            phys = torch.zeros(max(case.out_rows, M), N, dtype=F64)
            phys[case.out_row_index()] = r
            r = phys[:M]
        r = r[rows]
        if ep["res"] == "ln":
            r = (r - o.mean[rows, None]) * o.rstd[rows, None] * o.gamma + o.beta
    if ep["drop"]:
        s = drop_scale(o.drop[0])
        if mutant == "dropout_scale_from_threshold":
            s = 65536.0 / (65536.0 - drop_thresh(o.drop[0]))
        keep = o.keep
        if mutant == "dropout_pair_index_off_by_one_in_second_launch":
            keep = keep.clone()
            keep[M1:] = torch.from_numpy(keep_mask((M - M1) * N, o.drop, first=M1 * N + 2)).view(M - M1, N)
        if mutant == "residual_added_before_dropout":
            t, r = t + r, None
        t = t * keep.to(F64) * s
    if mutant == "rounded_before_residual" and r is not None:
        t = bf16r(t)
    if r is None:
        y = t
    else:
        y = t * r if ep["act"] == "mul" else t + r
    return y, y2, z, b


class Ref(object):
    """y (float64), its bound and the output format of one output tensor."""

    def __init__(self, y, bound, fmt, signed_ok=True):
        self.y, self.bound, self.fmt, self.signed_ok = y, bound, fmt, signed_ok


def linear_reference(o, epi_name, form="erf"):
    """{"out": Ref, "pre": Ref (second output)}: the float64 reference of one epilogue set and the module docstring's bounds."""
    ep = epi(epi_name)
    assert not (ep["drop"] and ep["act"] != "none"), "dropout is derived for act = none"
    y, y2, z, b = _linear_values(o, ep)
    F = (o.K + 8) * 2.0 ** -23 * (o.Pabs + b.abs())
    _, L, eps = act_terms(ep["act"], z, form)
    s = drop_scale(o.drop[0]) if ep["drop"] else 1.0
    if ep["act"] == "mul":
        E = o.r_mul.abs() * F
    else:
        E = s * L * F + eps
    if ep["res"] == "ln":
        E = E + 2.0 ** -21 * ((o.v.abs() + o.mean.abs()[:, None]) * o.rstd[:, None] * o.gamma.abs() + o.beta.abs())
    u = U_OUT[ep["out"]]
    out = {"out": Ref(y, u * y.abs() + (1 + u) * E, ep["out"])}
    if ep["c2"]:
        u2 = U_OUT["bf16"]
        E2 = 0.8 * F + 2.0 ** -20 * (1.0 + z.abs()) if ep["act"] == "gelu" else F
        # no signed statistic on gelu'(z): it is bounded with flat extremes (1.129 at z = sqrt 2, -0.129 at -sqrt 2) and runs into
        # 1 from above for z > 2.6, so the references pile up between two bf16 grid points and their roundings all fall the
        # same way; the minimal implementation itself shows -1.1 .. -2.1 there (host test)
        out["pre"] = Ref(y2, u2 * y2.abs() + (1 + u2) * E2, "bf16", signed_ok=ep["act"] != "gelu")
    return out


def linear_model(o, epi_name, mutant=None, M1=None):
    """float64 everywhere, each output rounded once -> {"out": tensor, "pre": tensor}"""
    ep = epi(epi_name)
    y, y2, _, _ = _linear_values(o, ep, mutant, M1)
    out = {"out": round_out(y, ep["out"], trunc=mutant == "output_truncated")}
    if ep["c2"]:
        out["pre"] = round_out(y2, "bf16", trunc=mutant == "output_truncated")
    return out


def linear_emulation_f32(o, epi_name):
    """The stated operations in float32 torch (one legitimate implementation): fp32 product, bias, activation, dropout scale,
    residual (rebuilt in four fp32 operations), unrounded output as float64."""
    ep = epi(epi_name)
    f = torch.float32
    z = o.a.to(f) @ o.w.to(f).t()
    if ep["bias"]:
        z = z + o.b.to(f)
    t = {"gelu": torch.nn.functional.gelu, "tanh": torch.tanh}.get(ep["act"], lambda x: x)(z)
    if ep["drop"]:
        t = t * o.keep.to(f) * torch.tensor(drop_scale(o.drop[0]), dtype=f)
    if ep["res"] == "ln":
        t = t + ((o.v.to(f) - o.mean.to(f)[:, None]) * o.rstd.to(f)[:, None] * o.gamma.to(f) + o.beta.to(f))
    elif ep["act"] == "mul":
        t = t * o.r_mul.to(f)
    elif ep["res"] is not None:
        t = t + (o.r_bf16 if ep["res"] == "bf16" else o.r_f16).to(f)
    out = {"out": t.to(F64)}
    if ep["c2"]:
        out["pre"] = (gelu_grad64(z.to(F64)).to(f) if ep["act"] == "gelu" else z).to(F64)
    return out


def ratios(ref, got, name="out", signed=False, rounded=True):
    """{check: measured / bound} of one output against a Ref; every value must lie in [0, 1] (the signed statistic: [-1, 1])."""
    got = got.to(F64)
    assert got.shape == ref.y.shape, (got.shape, ref.y.shape)
    assert bool(torch.isfinite(got).all()), "non-finite %s" % name
    err = got - ref.y
    r = torch.where(err == 0, torch.zeros_like(err), err.abs() / ref.bound)
    out = {name + " err/bound": float(r.max()) if r.numel() else 0.0}
    if signed and ref.fmt != "f32" and ref.signed_ok:
        out[name + " signed bias"], n = signed_stat(err, ref.y, ref.bound)
        assert n >= 100000, "the signed statistic wants N >= 1e5 (N = %d)" % n
    return out


def passes(rs):
    return all(abs(r) <= 1.0 and r == r for r in rs.values())


def assert_ratios(name, rs):
    from helpers import check_close

    for key in sorted(rs):
        check_close("gemm conformance %s: %s" % (name, key), abs(rs[key]), 0.0, 1.0)


# ---- linear_ln ----------------------------------------------------------------------------------------------------------------------
class LnOperands(object):
    pass


def row_stats(v32, rows):
    """Partial (sum, sum of squares) over 128-column slices of v [M, H] (float32 arithmetic, as a producer writes them) ->
    fp32 [H / 128, rows, 2]."""
    M, H = v32.shape
    parts = v32.to(torch.float32).view(M, H // 128, 128)
    st = torch.zeros(H // 128, rows, 2, dtype=torch.float32)
    st[:, :M, 0] = parts.sum(-1).t()
    st[:, :M, 1] = (parts * parts).sum(-1).t()
    return st


@functools.lru_cache(maxsize=2)
def ln_operands(M, K, N, mode):
    """A stream whose rows differ in scale and mean (what a pre-LayerNorm sum looks like), rows 16 .. 31 with mean = 8 x their
    spread, rows 32 .. 35 constant 0.5 with their sums of squares lowered so that q - mean^2 < 0 (the clamp)."""
    o = LnOperands()
    g = torch.Generator().manual_seed(1000 * mode + M + K + N)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    H = K if mode == 1 else N
    o.M, o.K, o.N, o.mode, o.H = M, K, N, mode, H
    o.rows = (M + 15) // 16 * 16
    spread = 0.5 + torch.rand(M, 1, generator=g)
    v = rn(M, H) * spread + 0.3 * rn(M, 1)
    v[16:32] += 8.0 * spread[16:32]
    v[32:36] = 0.5
    o.stats = row_stats(v, o.rows)
    o.stats[:, 32:36, 1] *= (1.0 - 2.0 ** -18)
    gamma, beta = 1.0 + 0.2 * rn(H), 0.1 * rn(H)
    if mode == 1:
        o.a = bf16r(v)                                   # the bf16 copy of the stream
        Wp = rn(N, K) * (1.5 / math.sqrt(K))
        o.w = bf16r(Wp * gamma[None, :])
        o.colv = f32r(o.w.sum(1))                        # g = rowsum(W')
        o.bias = f32r(Wp.to(F64) @ beta.to(F64) + 0.05 * rn(N))   # h
    else:
        o.a = bf16r(rn(M, K) * 0.7)
        o.w = bf16r(rn(N, K) * (1.0 / math.sqrt(K)))
        o.colv = f32r(gamma)
        o.bias = f32r(0.05 * rn(N) + beta)               # cb
        o.rs = f16r(v)
    o.P = o.a @ o.w.t()
    o.Pabs = o.a.abs() @ o.w.abs().t()
    return o


def _ln_row_terms(o, mutant=None):
    st = o.stats.to(F64)[:, :o.M]
    if mutant == "ln_stats_slice_dropped" and o.mode == 1:
        st = st[:-1]
    mean = st[..., 0].sum(0) / o.H
    q = st[..., 1].sum(0) / o.H
    var = q - mean * mean
    if mutant != "ln_var_unclamped_negative":
        var = torch.clamp(var, min=0.0)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    kappa = (q + mean * mean) / (var + LN_EPS)
    rho = 2.0 ** -22 * kappa + 2.0 ** -21
    return mean[:, None], rstd[:, None], rho[:, None]


def _slice_sums(x):
    M, N = x.shape
    return x.view(M, N // 128, 128).sum(-1).t()          # [N / 128, M]


def ln_reference(o, act="none"):
    """mode 1: {"out": Ref}; mode 2: {"stream": Ref (fp16), "copy": Ref (bf16), "sum": Ref, "sq": Ref ([N / 128, M], fp32)}"""
    mean, rstd, rho = _ln_row_terms(o)
    F = (o.K + 8) * 2.0 ** -23 * o.Pabs
    if o.mode == 1:
        pre = rstd * (o.P - mean * o.colv) + o.bias
        E = rstd * F + (rho + 2.0 ** -20) * ((rstd * o.P).abs() + (mean * rstd * o.colv).abs()) + 2.0 ** -22 * o.bias.abs()
        y, L, eps = act_terms(act, pre, "poly")
        u = U_OUT["bf16"]
        return {"out": Ref(y, u * y.abs() + (1 + u) * (L * E + eps), "bf16")}
    v = o.P + o.bias + o.colv * ((o.rs - mean) * rstd)
    E = F + (rho + 2.0 ** -20) * o.colv.abs() * (o.rs.abs() + mean.abs()) * rstd + 2.0 ** -22 * o.bias.abs()
    u16, u8 = U_OUT["f16"], U_OUT["bf16"]
    c = 130 * 2.0 ** -24
    return {"stream": Ref(v, u16 * v.abs() + (1 + u16) * E, "f16"), "copy": Ref(v, u8 * v.abs() + (1 + u8) * E, "bf16"),
            "sum": Ref(_slice_sums(v), _slice_sums(E) + c * _slice_sums(v.abs()), "f32"),
            "sq": Ref(_slice_sums(v * v), _slice_sums(2 * v.abs() * E + E * E) + c * _slice_sums(v * v), "f32")}


def ln_model(o, act="none", mutant=None):
    mean, rstd, _ = _ln_row_terms(o, mutant)
    if o.mode == 1:
        pre = rstd * (o.P - mean * o.colv) + o.bias
        return {"out": bf16r(act_terms(act, pre, "poly")[0])}
    v = o.P + o.bias + o.colv * ((o.rs - mean) * rstd)
    s = f16r(v)
    vs = s if mutant == "stats_out_of_rounded_stream" else v
    return {"stream": s, "copy": bf16r(s) if mutant == "ln_mode2_bf16_copy_from_fp16" else bf16r(v),
            "sum": f32r(_slice_sums(vs)), "sq": f32r(_slice_sums(vs * vs))}


def ln_emulation_f32(o, act="none"):
    """The epilogue's own operations in float32 (gemm_v7_ln_epilogue.hpp), outputs unrounded."""
    f = torch.float32
    st = o.stats[:, :o.M]
    inv = torch.tensor(1.0 / o.H, dtype=f)
    mean = st[..., 0].sum(0) * inv
    var = torch.clamp(st[..., 1].sum(0) * inv - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + torch.tensor(LN_EPS, dtype=f))
    ra, rb = rstd[:, None], (-mean * rstd)[:, None]
    acc = o.a.to(f) @ o.w.to(f).t()
    if o.mode == 1:
        z = ra * acc + (rb * o.colv.to(f) + o.bias.to(f))
        z = torch.nn.functional.gelu(z) if act == "gelu" else z
        return {"out": z.to(F64)}
    w = (o.rs.to(f) * ra + rb) * o.colv.to(f) + (acc + o.bias.to(f))
    parts = w.view(o.M, o.N // 128, 128)
    return {"stream": w.to(F64), "copy": w.to(F64), "sum": parts.sum(-1).t().to(F64), "sq": (parts * parts).sum(-1).t().to(F64)}
