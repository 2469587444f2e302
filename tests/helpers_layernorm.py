"""fp64 reference, CPU rounding model, derived per-element bounds, exact constructions and the case table of the LayerNorm family:
layernorm_rows / layernorm_rows_full, layernorm_bwd_rows / layernorm_bwd_rows_full with ln_bwd_reduce, embed_layernorm /
embed_layernorm_bwd / embed_layernorm_f32 (csrc/layernorm.hip, csrc/fp32_path.hip), layernorm_rows_f32 (fp32_path.hip), ln_bwd_f32
(fp32_train.hip), ln_apply_rows and ln_stream_init (ln_deferred.hip).

Everything here is plain torch / numpy on the CPU in float64, taken from the bf16-, fp16- or fp32-exact inputs.
tests/test_host_layernorm_reference.py proves without a GPU that the bounds accept the minimal implementation (float64, every
output rounded once) and an fp32 emulation in three summation orders with a factor two to spare, and reject a table of subtly
wrong implementations; tests/test_gpu_layernorm_conformance.py holds the HIP kernels to the same bounds through visitron_amd.ops,
tests/ln_conformance_worker.py under the non-default values of VT_LN_FWD_ROWS / VT_LN_FWD_BLOCKS / VT_LN_BWD_ROWS.  No bound
below was chosen by looking at a kernel's output.

Out of scope: the weight prefetch that rides in the spare workgroups of layernorm_rows_full and ln_bwd_reduce (LnArgs::pf,
ln_bwd_reduce's pf) is reachable through the encoder layer loops only, not through a single-op entry point; every call here runs
with n_main == gridDim.x.

FORWARD  mean, var = mean((x - mean)^2) (biased), rstd = 1 / sqrt(var + eps), xhat = (x - mean) rstd, y = xhat gamma + beta.
e = 2^-24 (fp32 unit round-off), u_out = helpers_gemm.U_OUT, A1 = mean_j |x_j|, per row and element:

    dmean = (H + 2) e A1                            an fp32 sum of H terms in ANY order ((H - 1) e sum |x|), the multiply by
                                                    fl(1 / H) (two roundings) or the divide by H
    rho   = (H / 2 + 4) e + dmean^2 / (2 (var+eps)) relative error of rstd.  The variance is two-pass: a shifted mean enters it
                                                    only squared (mean((x - m')^2) = var + (m' - mean)^2), its H squares and their
                                                    sum in any order give (H + 3) e relative, "+ eps", the root and the divide three
                                                    more; halved by the root: (H / 2 + 4) e
    E     = dmean rstd |gamma| + |xhat gamma| (rho + 3 e) + e |y|
                                                    the shifted mean in x - mean; the subtraction and two multiplies (3 e) and rstd's
                                                    own error on xhat gamma; the final add
    |got - y| <= u_out |y| + (1 + u_out) E          bf16, fp16 and fp32 outputs alike (each rounded from the fp32 value)
    |mean_got - mean| <= dmean,   |rstd_got - rstd| <= rstd (rho + 2 e)

  Embedding kernels: x = (word + pos) + type is formed in fp32 and taken in float64 here; each x_j carries
  d_j = 2 e (|word| + |pos| + |type|) (two adds).  It reaches y directly (d_j rstd |gamma|), through the mean (mean(d) is added to
  dmean) and through the variance (mean(|x - mean| d) / (var + eps) is added to rho: d(var) = 2 mean((x - mean) d), halved by the
  root).  The last two are an order below the first and are what a bound "through rstd |gamma|" alone leaves out.
  Dropout after the LayerNorm (layernorm_drop_f32, embed_layernorm with drop): a dropped element must be exactly 0 (bound 0), a
  kept one is y s with s the fp32 value 1.0f / (1.0f - p): E s + e |y s|.
  ln_apply: mean, var = max(q - mean^2, 0), rstd in float64 from the GIVEN fp32 partial statistics (helpers_gemm._ln_row_terms);
  kappa = (q + mean^2) / (var + eps) is the cancellation of q - mean^2 in fp32, rho = 2^-22 kappa + 2^-21 as in helpers_gemm, and
  E = (rho + 2^-20) |gamma| (|v| + |mean|) rstd + 2^-22 |beta| (the deferred LayerNorm's own term of helpers_gemm.ln_reference).
  ln_stream_init: nothing to bound; stream == the saturating fp16 convert, copy == the bf16 convert, statistics slice 0 ==
  (0, fl32(H fl32(1 - eps))), slices 1 .. np - 1 zero, statistic rows >= M untouched.

BACKWARD  g = dy gamma, m1 = mean(g), m2 = mean(g xhat), dx = rstd (g - m1 - xhat m2), dgamma = sum_rows dy xhat, dbeta = sum_rows dy.

    ex    = dmean rstd + |xhat| (rho + 2 e)                                       error of xhat (+ d_j rstd for the embedding)
    dm1   = (H + 2) e mean|g|          dm2 = (H + 2) e mean|g xhat| + mean(|g| ex)
    Edx   = rstd (e |g| + dm1 + |xhat| dm2 + ex |m2|) + (rho + 4 e) rstd (|g| + |m1| + |xhat m2|)
    |dx_got - dx| <= u_out |dx| + (1 + u_out) Edx
    |dgamma_got - dgamma| <= sum_rows |dy| ex + (M + 8) e sum_rows |dy xhat|   (+ e |prior + dgamma| with accumulate)
    |dbeta_got  - dbeta|  <=                    (M + 8) e sum_rows |dy|        (+ the same)

  dx_dropped / dx_drop: dropped elements exactly 0, kept ones dx s rounded once from the fp32 value: Edx s + e |dx s|.
  Input dropout (drop_in, the embedding's drop) is applied to dy first, in the reference as well: dy' = keep dy s carries one
  more rounding, e |g| in Edx; in the row sums it is one of the eight spare roundings of (M + 8).

  Like helpers_gemm's F these worst-case sums are knowingly slack (a real fp32 sum errs like sqrt H): they catch arithmetic done
  in the wrong precision or with a wrong operand where |y| is small; structure is the exact constructions' job.

THE BOUND MAY NOT GO VACUOUS  A row whose dmean rstd is large passes anything (a constant row at eps = 1e-12: rstd = 1e6).  Every
case names its degenerate rows (constant rows; for ln_apply the rows whose q - mean^2 is negative), at most eight; they are held to
finiteness and the bound as it stands, and the host test asserts from the reference alone that every other row has
dmean rstd <= 2^-10 (ln_apply: (rho + 2^-20) |mean| rstd <= 2^-10).  Inputs (random_rows): row scales in 0.5 .. 1.5, a row offset,
rows with mean = 8 x spread (x min(1, 1024 / H): the condition is linear in H), rows scaled by 0.01 -- under eps = 1e-5 eps is then
4 .. 40 % of var + eps -- and the constant rows.

EXACT CONSTRUCTIONS  Every row holds H / 2 entries +s and H / 2 entries -s at random positions, s a power of two in 2^-3 .. 2^2
that changes from row to row, eps = 0, gamma an integer in [-3, 3], beta in [-8, 8]: the sum is 0 in any order, every square is
s^2, H s^2 fl(1 / H) rounds to s^2 (the host test shows it for every H of the table in three orders), so mean = 0 and
rstd = 1 / s are exact and the output must EQUAL +-gamma + beta in every format (bound 0).  Backward: dy an integer in [-4, 4],
gamma in [-2, 2]: dgamma and dbeta are sums of small integers and must equal the float64 sums at every M, also accumulated onto
an integer prior; dx is exact where H is a power of two (m1 and m2 are then integers / 2^k) and goes by the bound elsewhere
(m1 fl(1 / 768) is inexact).  Dropout at p = 0.5 (scale 2, exact).  Every output lives in a buffer filled with a sentinel before
the call: columns past H of a row stride > H, rows past M, the gap rows of a row remap and rows t >= T of the embedding's [B, S]
must be bit-identical afterwards (check "<output> padding").
"""
import functools

import numpy as np
import torch

from helpers_attention import bf16_trunc, bf16r, signed_stat  # noqa: F401
from helpers_gemm import (F64, U_OUT, Ref, _ln_row_terms, drop_scale, f16_trunc, f16r, f32r, keep_mask, passes,  # noqa: F401
                          round_out, row_stats)
import helpers_gemm as hg

E32 = 2.0 ** -24
SENTINEL = 12345.0
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "i32": torch.int32}
DROP_P, DROP_P_EXACT = 0.1, 0.5
SITE_EMB = 0xE0
ORDERS = ("sequential", "pairwise", "lanes")
INF = float("inf")


# ---- buffers -------------------------------------------------------------------------------------------------------------------
class Buf(object):
    """A logical [M, n] tensor at rows `index`, columns [:n] of a physical [rows, ld] buffer of format fmt; everything else is
    padding and holds the sentinel."""

    def __init__(self, fmt, M, n, ld=None, rows=None, index=None):
        self.fmt, self.M, self.n = fmt, M, n
        self.ld = n if ld is None else ld
        self.index = torch.arange(M) if index is None else index
        top = int(self.index.max()) + 1 if M else 0
        self.rows = top if rows is None else rows
        assert self.rows >= top and self.ld >= n

    def blank(self):
        return torch.full((self.rows, self.ld), SENTINEL, dtype=DT[self.fmt])

    def place(self, logical, base=None):
        buf = self.blank() if base is None else base.clone()
        buf[self.index, :self.n] = logical.to(DT[self.fmt])
        return buf

    def mask(self):
        m = torch.zeros(self.rows, self.ld, dtype=torch.bool)
        m[self.index, :self.n] = True
        return m

    def read(self, buf, base=None):
        """(logical [M, n] float64, padding untouched)"""
        buf = buf.detach().cpu().reshape(self.rows, self.ld)
        base = self.blank() if base is None else base
        pad = ~self.mask()
        return buf[self.index, :self.n].to(F64), bool(torch.equal(buf[pad].to(F64), base[pad].to(F64)))


def remap_index(M, grp):
    r = torch.arange(M)
    return r if not grp[0] else (r // grp[0]) * grp[1] + r % grp[0]


def round_in(x, fmt):
    return round_out(x.to(F64), fmt)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """kind: the entry point (fwd, bwd, emb, emb_f32, emb_bwd, rows_f32, drop_f32, bwd_f32, apply, stream_init); reaches: the
    kernel instantiation the case is meant to run; p: the parameters; why: what can go wrong at this shape."""

    def __init__(self, name, kind, reaches, why, **p):
        self.name, self.kind, self.reaches, self.why, self.p = name, kind, reaches, why, p

    def __repr__(self):
        return self.name

    def get(self, key, default=None):
        return self.p.get(key, default)


FULL_H = {768: (1, 1), 512: (1, 0), 1024: (2, 0), 256: (0, 1)}
FAMILY_ENV = {
    "default": {},
    "chunked": {"VT_LN_FWD_ROWS": "0", "VT_LN_BWD_ROWS": "0"},
    "fwd1_bwd2": {"VT_LN_FWD_ROWS": "1", "VT_LN_FWD_BLOCKS": "2", "VT_LN_BWD_ROWS": "2"},
    "bwd4": {"VT_LN_BWD_ROWS": "4"},
}
LN_BWD_MAX_BLOCKS = 1024


def _switch(name, env):
    from visitron_amd import switches

    return switches.integer(name, {} if env is None else env)


def fwd_dispatch(H, grp_rows, xf16, env=None):
    """vt_layernorm_dispatch (csrc/layernorm.hip) restated: (kernel instantiation, rows per wave, workgroups of M rows -> count)."""
    rpw = _switch("VT_LN_FWD_ROWS", env)
    if rpw > 0 and grp_rows == 0 and H in FULL_H:
        R = 2 if rpw >= 2 else 1
        cap = _switch("VT_LN_FWD_BLOCKS", env)
        return "layernorm_rows_full<%d,%d,%d,%d>" % (FULL_H[H] + (R, int(xf16))), R, lambda M: min(((M + R - 1) // R + 3) // 4, cap)
    return "layernorm_rows<%d,%d>" % ((H + 511) // 512, int(xf16)), 4, lambda M: (M + 15) // 16


def bwd_dispatch(H, gamma_aligned, xf16, env=None):
    """vt_layernorm_bwd_dispatch restated: (kernel instantiation, rows per wave, M -> partial rows = workgroups)."""
    rpw = _switch("VT_LN_BWD_ROWS", env)
    if rpw > 0 and H in FULL_H and gamma_aligned:
        R = 4 if rpw >= 4 else 2 if rpw >= 2 else 1
        return ("layernorm_bwd_rows_full<%d,%d,%d,%d>" % (FULL_H[H] + (R, int(xf16))), R,
                lambda M: min(((M + R - 1) // R + 3) // 4, LN_BWD_MAX_BLOCKS))
    return "layernorm_bwd_rows<%d,%d>" % (1 if H <= 512 else 2, int(xf16)), 1, lambda M: min((M + 3) // 4, LN_BWD_MAX_BLOCKS)


def case_dispatch(case, env=None):
    """(instantiation, rows per wave, workgroups) the library runs `case` with under the switch values `env`."""
    p, k = case.p, case.kind
    if k == "fwd":
        name, R, nb = fwd_dispatch(p["H"], p.get("grp", (0, 0))[0], p["xfmt"] == "f16", env)
        return name, R, nb(p["M"])
    if k == "bwd":
        name, R, nb = bwd_dispatch(p["H"], not p.get("gamma_off"), p["xfmt"] == "f16", env)
        return name, R, nb(p["M"])
    H = p["H"]
    if k == "emb":
        return "embed_layernorm<%d>" % ((H + 511) // 512), 1, (p["B"] * p["T"] + 3) // 4
    if k == "emb_bwd":
        return "embed_layernorm_bwd<%d>" % (1 if H <= 512 else 2), 1, min((p["B"] * p["T"] + 3) // 4, LN_BWD_MAX_BLOCKS)
    if k == "emb_f32":
        return "embed_layernorm_f32", 1, (p["B"] * p["T"] + 3) // 4
    if k in ("rows_f32", "drop_f32"):
        return "layernorm_rows_f32<%d,%d>" % (int(p.get("xfmt", "f32") == "f32"), int(p.get("yfmt", "f32") == "f32")), 1, (p["M"] + 3) // 4
    if k == "bwd_f32":
        return "ln_bwd_f32", 1, min((p["M"] + 3) // 4, 512)
    return {"apply": "ln_apply_rows", "stream_init": "ln_stream_init"}[k], 1, (p["M"] + 3) // 4


INSTANTIATIONS = tuple(
    ["layernorm_rows<%d,%d>" % (ch, f) for ch in (1, 2, 3, 4) for f in (0, 1)]
    + ["layernorm_rows_full<%d,%d,%d,%d>" % (c + (r, f)) for c in FULL_H.values() for r in (1, 2) for f in (0, 1)]
    + ["layernorm_bwd_rows<%d,%d>" % (ch, f) for ch in (1, 2) for f in (0, 1)]
    + ["layernorm_bwd_rows_full<%d,%d,%d,%d>" % (c + (r, f)) for c in FULL_H.values() for r in (1, 2, 4) for f in (0, 1)]
    + ["embed_layernorm<%d>" % ch for ch in (1, 2, 3, 4)] + ["embed_layernorm_bwd<1>", "embed_layernorm_bwd<2>", "embed_layernorm_f32"]
    + ["layernorm_rows_f32<%d,%d>" % (i, o) for i in (0, 1) for o in (0, 1)] + ["ln_bwd_f32", "ln_apply_rows", "ln_stream_init"])
# loop features of a kernel that a case must enter (Case.p["enters"]); the host test proves each from the dispatch rule
FEATURES = ("fwd full: second trip round the grid-stride loop", "bwd full: second trip round the grid-stride loop",
            "bwd chunked: second trip round the grid-stride loop", "reduce: unrolled loop", "reduce: unrolled loop plus a remainder",
            "embedding bwd: second trip round the grid-stride loop", "ln_bwd_f32: second trip round the grid-stride loop",
            "fwd: tail group with a repeated row")


def _fwd(M, H, xfmt, kernel, i=0, exact=False, grp=(0, 0), R=None, why="", **kw):
    """One ops.layernorm case; i rotates the options (second output, statistics, row strides > H, eps)."""
    f16 = xfmt == "f16"
    reaches = ("layernorm_rows<%d,%d>" % ((H + 511) // 512, int(f16)) if kernel == "chunked"
               else "layernorm_rows_full<%d,%d,%d,%d>" % (FULL_H[H] + (R, int(f16))))
    p = dict(M=M, H=H, xfmt=xfmt, yh=f16 and i % 2 == 0, stats=i % 3 != 1, pad=i % 2 == 1 or exact, grp=grp,
             eps=0.0 if exact else (1e-5 if i % 2 else 1e-12), exact=exact)
    p.update(kw)
    name = "fwd%s %dx%d %s%s%s%s" % (" exact" if exact else "", M, H, xfmt, " +f16" if p["yh"] else "", " +stats" if p["stats"] else "",
                                      " remap%d/%d" % grp if grp[0] else "")
    return Case(name, "fwd", reaches, why, **p)


def _bwd(M, H, xfmt, kernel, i=0, exact=False, R=1, gamma_off=False, why="", **kw):
    f16 = xfmt == "f16"
    reaches = ("layernorm_bwd_rows<%d,%d>" % (1 if H <= 512 else 2, int(f16)) if kernel == "chunked"
               else "layernorm_bwd_rows_full<%d,%d,%d,%d>" % (FULL_H[H] + (R, int(f16))))
    p = dict(M=M, H=H, xfmt=xfmt, dx2=i % 2 == 0, accumulate=i % 3 == 0, pad=i % 2 == 1 or exact, gamma_off=gamma_off,
             eps=0.0 if exact else (1e-5 if i % 2 else 1e-12), exact=exact)
    p.update(kw)
    name = "bwd%s %dx%d %s%s%s%s" % (" exact" if exact else "", M, H, xfmt, " +dropped" if p["dx2"] else "",
                                      " accumulate" if p["accumulate"] else "", " gamma+4B" if gamma_off else "")
    return Case(name, "bwd", reaches, why, **p)


def _fwd_chunked_cases(hs, ms, exact_ms=(5, 17)):
    why = {8: "one lane", 64: "small single chunk", 264: "single chunk, not a multiple of 512", 504: "last lane of a chunk idle",
           520: "one lane in chunk 2", 1032: "three chunks", 1536: "three full chunks", 2048: "four chunks"}
    out, i = [], 0
    for H in hs:
        for M in ms:
            out.append(_fwd(M, H, ("bf16", "f16")[i % 2], "chunked", i // 2, why="%s; %d rows: four rows per wave, tail repeats the last row"
                            % (why.get(H, "chunked kernel forced by the switch"), M)))
            i += 1
        for j, M in enumerate(exact_ms):
            out.append(_fwd(M, H, ("f16", "bf16")[j % 2], "chunked", 2 * j, exact=True, why="structure: columns, chunks, rows, tail"))
    return out


def _bwd_full_cases(hs, ms, R, exact_ms):
    out, i = [], 0
    for H in hs:
        for M in ms:
            nb = min(((M + R - 1) // R + 3) // 4, LN_BWD_MAX_BLOCKS)
            enters = []
            if (M + R - 1) // R > 4 * nb:
                enters.append("bwd full: second trip round the grid-stride loop")
            if nb >= 193:
                enters.append("reduce: unrolled loop" if nb == 193 or nb % 256 == 0 else "reduce: unrolled loop plus a remainder")
            out.append(_bwd(M, H, ("bf16", "f16")[i % 2], "full", i // 2, R=R, enters=tuple(enters),
                            why="%d rows on %d-row groups: %d partial rows" % (M, R, nb)))
            i += 1
        for j, M in enumerate(exact_ms):
            out.append(_bwd(M, H, ("f16", "bf16")[j % 2], "full", 3 * j, exact=True, R=R, why="structure: rows, groups, partial rows"))
    return out


def _emb(kind, B, T, S, H, i=0, exact=False, bad=False, why=""):
    reaches = {"emb": "embed_layernorm<%d>" % ((H + 511) // 512), "emb_f32": "embed_layernorm_f32",
               "emb_bwd": "embed_layernorm_bwd<%d>" % (1 if H <= 512 else 2)}[kind]
    p = dict(B=B, T=T, S=S, H=H, M=B * T, pos_ids=i % 2 == 0, type_ids=i % 3 != 0, drop=kind != "emb_f32" and i % 2 == 1, bad=bad,
             accumulate=kind == "emb_bwd" and i % 2 == 0, pad=True, eps=0.0 if exact else (1e-12 if i % 2 else 1e-5), exact=exact)
    enters = ("embedding bwd: second trip round the grid-stride loop",) if kind == "emb_bwd" and B * T > 4 * LN_BWD_MAX_BLOCKS else ()
    p["enters"] = enters
    name = "%s%s %dx%d(S %d) H %d%s%s%s%s" % (kind, " exact" if exact else "", B, T, S, H, " pos_ids" if p["pos_ids"] else "",
                                              " type_ids" if p["type_ids"] else "", " drop" if p["drop"] else "", " bad ids" if bad else "")
    return Case(name, kind, reaches, why, **p)


@functools.lru_cache(maxsize=None)
def cases(family="default"):
    """The case table shared by the host test, the GPU test (family "default") and the worker (the other families: the switch
    values of FAMILY_ENV)."""
    out = []
    if family == "chunked":
        out += _fwd_chunked_cases((256, 512, 768, 1024), (5, 17, 33), exact_ms=(17, 21))
        i = 0
        for H in (256, 512, 768, 1024):
            for M in (5, 769):
                out.append(_bwd(M, H, ("bf16", "f16")[i % 2], "chunked", i // 2, why="the chunked backward at a full-kernel width",
                                enters=("reduce: unrolled loop",) if M == 769 else ()))
                i += 1
            out.append(_bwd(21, H, "f16", "chunked", 0, exact=True, why="structure"))
            out.append(_bwd(22, H, "bf16", "chunked", 3, exact=True, why="structure"))
        return tuple(out)
    if family == "fwd1_bwd2":
        i = 0
        for H in (256, 512, 768, 1024):
            for M in (1, 7, 8, 9, 40):
                out.append(_fwd(M, H, ("bf16", "f16")[i % 2], "full", i // 2, R=1,
                                enters=("fwd full: second trip round the grid-stride loop",) if M > 8 else (),
                                why="one row per wave on two workgroups: %d trips round the loop" % ((M + 7) // 8)))
                i += 1
            for M, xf in ((40, "f16"), (33, "bf16")):
                out.append(_fwd(M, H, xf, "full", 0, exact=True, R=1, enters=("fwd full: second trip round the grid-stride loop",),
                                why="structure over five trips"))
        out += _bwd_full_cases((256, 512, 768, 1024), (1, 3, 5, 769), 2, (7, 10))
        out.append(_bwd(8197, 256, "bf16", "full", 0, exact=True, R=2, why="structure: two trips with a ragged last pair",
                        enters=("bwd full: second trip round the grid-stride loop", "reduce: unrolled loop")))
        return tuple(out)
    if family == "bwd4":
        out += _bwd_full_cases((256, 512, 768, 1024), (1, 3, 5, 16, 17), 4, (18, 5))
        out.append(_bwd(4099, 256, "f16", "full", 1, R=4, why="257 partial rows of four-row groups",
                        enters=("reduce: unrolled loop plus a remainder",)))
        out.append(_bwd(4099, 256, "bf16", "full", 0, exact=True, R=4, why="structure", enters=("reduce: unrolled loop plus a remainder",)))
        return tuple(out)
    assert family == "default", family
    # forward, bf16 path, chunked kernel
    out += _fwd_chunked_cases((8, 64, 264, 504, 520, 1032, 1536, 2048), (1, 3, 4, 5, 16, 17, 33))
    out.append(_fwd(17, 768, "bf16", "chunked", 2, grp=(5, 9), why="the only in-process route to the chunked kernel at 768"))
    out.append(_fwd(17, 768, "bf16", "chunked", 0, grp=(5, 9), exact=True, why="structure under the row remap: gap rows"))
    # forward, full kernel at R = 2
    i = 0
    for H in (256, 512, 768, 1024):
        for M in (1, 2, 3, 7, 8, 9):
            out.append(_fwd(M, H, ("bf16", "f16")[i % 2], "full", i // 2, R=2, enters=("fwd: tail group with a repeated row",) if M % 2 else (),
                            why="two rows per wave: %s" % ("the tail pair repeats the last row" if M % 2 else "whole pairs")))
            i += 1
        for j, M in enumerate((7, 9)):
            out.append(_fwd(M, H, ("f16", "bf16")[j], "full", 2 * j, exact=True, R=2, why="structure: lanes' columns, pairs, tail"))
    out.append(_fwd(300, 768, "f16", "full", 0, R=2, why="230 400 elements: the signed statistic on both outputs"))
    loop2 = ("fwd full: second trip round the grid-stride loop", "fwd: tail group with a repeated row")
    out.append(_fwd(8195, 768, "f16", "full", 0, R=2, enters=loop2, why="twice round the grid-stride loop, ragged last pair; prefetched rows"))
    out.append(_fwd(8195, 256, "bf16", "full", 1, R=2, enters=loop2, why="the same on the 4-column-per-lane layout"))
    out.append(_fwd(8195, 256, "bf16", "full", 0, exact=True, R=2, enters=loop2, why="structure across the second trip"))
    out.append(_fwd(8195, 768, "bf16", "full", 0, exact=True, R=2, enters=loop2, why="structure across the second trip"))
    # backward, bf16 path
    i = 0
    for H in (8, 64, 504, 520, 1016):
        for M in (3, 17):
            out.append(_bwd(M, H, ("bf16", "f16")[i % 2], "chunked", i // 2, why="chunked backward, %d chunk(s)" % (1 if H <= 512 else 2)))
            i += 1
        out.append(_bwd(5, H, "f16", "chunked", 0, exact=True, why="structure"))
        out.append(_bwd(6, H, "bf16", "chunked", 3, exact=True, why="structure"))
    out.append(_bwd(769, 1016, "bf16", "chunked", 1, why="193 partial rows behind the two-chunk kernel", enters=("reduce: unrolled loop",)))
    out.append(_bwd(4099, 520, "f16", "chunked", 0, exact=True, why="structure: grid-stride loop of the chunked kernel",
                    enters=("bwd chunked: second trip round the grid-stride loop", "reduce: unrolled loop")))
    out.append(_bwd(17, 768, "bf16", "chunked", 0, gamma_off=True, why="gamma four bytes off a 16-byte boundary forces the chunked kernel"))
    out.append(_bwd(17, 768, "f16", "chunked", 0, gamma_off=True, exact=True, why="structure on the misaligned-gamma route"))
    out += _bwd_full_cases((256, 512, 768, 1024), (1, 3, 4, 5, 769, 1025, 4096, 4099), 1, (5, 769, 1025, 4099))
    # embedding
    i = 0
    for H in (128, 520, 768):
        for (B, T, S) in ((1, 1, 3), (1, 5, 7), (82, 50, 53)):
            for kind in ("emb", "emb_f32", "emb_bwd"):     # one counter per kind: pos_ids / type_ids / drop rotate within each
                out.append(_emb(kind, B, T, S, H, i, why="%d tokens; rows t >= T of [B, S] untouched" % (B * T)))
            i += 1
    for kind in ("emb", "emb_f32", "emb_bwd"):
        out.append(_emb(kind, 2, 5, 7, 520, 2, bad=True, why="one out-of-range id per table: the flag is set, the clamped row computed"))
        out.append(_emb(kind, 82, 50, 53, 128, 0, exact=True, why="structure: tokens, rows b S + t, partial rows"))
        out.append(_emb(kind, 2, 5, 7, 768, 1, exact=True, why="structure on two chunks"))
    out.append(_emb("emb", 1, 5, 7, 1032, 1, why="three chunks"))
    out.append(_emb("emb", 1, 5, 7, 1544, 0, why="four chunks"))
    # fp32 path
    pairs = (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"))
    i = 0
    for H in (4, 260, 1024, 4096):
        for M in (1, 5, 37):
            for (xf, yf) in (pairs if M == 37 else (pairs[i % 4],)):
                out.append(Case("rows_f32 %dx%d %s->%s" % (M, H, xf, yf), "rows_f32", "layernorm_rows_f32<%d,%d>" % (xf == "f32", yf == "f32"),
                                "one wave per row, %d of 16 column passes" % ((H + 255) // 256), M=M, H=H, xfmt=xf, yfmt=yf, pad=i % 2 == 1,
                                eps=1e-5 if i % 2 else 1e-12, exact=False, grp=(0, 0)))
                i += 1
        if H != 260:
            for (xf, yf) in (pairs if H == 1024 else (pairs[0], pairs[2])):
                out.append(Case("rows_f32 exact 37x%d %s->%s" % (H, xf, yf), "rows_f32", "layernorm_rows_f32<%d,%d>" % (xf == "f32", yf == "f32"),
                                "structure", M=37, H=H, xfmt=xf, yfmt=yf, pad=True, eps=0.0, exact=True, grp=(0, 0)))
    for (xf, yf) in (pairs[0], pairs[3]):
        for exact in (False, True):
            H = 256 if exact else 260
            out.append(Case("rows_f32%s 37x%d %s->%s remap5/9 in place" % (" exact" if exact else "", H, xf, yf), "rows_f32",
                            "layernorm_rows_f32<%d,%d>" % (xf == "f32", yf == "f32"), "x and y remapped, one buffer", M=37, H=H,
                            xfmt=xf, yfmt=yf, pad=True, eps=0.0 if exact else 1e-5, exact=exact, grp=(5, 9), inplace=True))
    for H, exact in ((260, False), (1024, False), (1024, True)):
        out.append(Case("drop_f32%s 37x%d remap5/9" % (" exact" if exact else "", H), "drop_f32", "layernorm_rows_f32<1,1>",
                        "compact x, remapped y, dropout indexed by the row before the remap", M=37, H=H, pad=True,
                        eps=0.0 if exact else 1e-5, exact=exact, grp=(5, 9), drop=True))
    i = 0
    for H in (4, 260, 768, 1024):
        for M in (1, 5, 2049):
            out.append(Case("bwd_f32 %dx%d #%d" % (M, H, i), "bwd_f32", "ln_bwd_f32", "fp32 backward, %d rows" % M, M=M, H=H, pad=i % 2 == 1,
                            grp=(5, 9) if i % 2 == 0 else (0, 0), drop_in=i % 3 == 0, drop_out=i % 2 == 0, no_dx=i % 4 == 2,
                            accumulate=i % 3 == 1, eps=1e-5 if i % 2 else 1e-12, exact=False,
                            enters=("ln_bwd_f32: second trip round the grid-stride loop",) if M > 2048 else ()))
            i += 1
        out.append(Case("bwd_f32 exact 2049x%d" % H, "bwd_f32", "ln_bwd_f32", "structure: rows past 512 workgroups, partial rows", M=2049, H=H,
                        pad=True, grp=(5, 9), drop_in=False, drop_out=True, no_dx=False, accumulate=True, eps=0.0, exact=True,
                        enters=("ln_bwd_f32: second trip round the grid-stride loop",)))
    # deferred path
    i = 0
    for H in (128, 768, 1024):
        for M in (1, 5, 300):
            out.append(Case("apply %dx%d np %d %s" % (M, H, H // 128, ("bf16", "f32", "bf16+f32")[i % 3]), "apply", "ln_apply_rows",
                            "one-pass variance from %d partial statistics, clamp at 0" % (H // 128), M=M, H=H, outs=("bf16", "f32", "bf16+f32")[i % 3],
                            pad=i % 2 == 0, eps=hg.LN_EPS, exact=False))
            i += 1
    for H in (4, 768):
        out.append(Case("stream_init 9x%d np 6" % H, "stream_init", "ln_stream_init", "saturating fp16 convert, identity statistics",
                        M=9, H=H, np=6, pad=True, eps=1e-12, exact=True))
    return tuple(out)


def all_cases():
    return tuple((fam, c) for fam in FAMILY_ENV for c in cases(fam))


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (1 << 31)


def random_rows(g, M, H):
    """(x [M, H] float32, constant rows): module docstring, THE BOUND MAY NOT GO VACUOUS."""
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    spread = 0.5 + torch.rand(M, 1, generator=g)
    x = rn(M, H) * spread + 0.3 * rn(M, 1)
    r = torch.arange(M)
    shifted = (r % 8 == 3) | ((r % 64 >= 16) & (r % 64 < 32))
    x[shifted] += 8.0 * min(1.0, 1024.0 / H) * spread[shifted]
    x[r % 8 == 6] *= 0.01
    const = [c for c in ((7,) if M < 20 else (7, M - 2)) if c < M]
    for c in const:
        x[c] = 0.5
    return x, const


def exact_rows(g, M, H):
    """+-s rows (module docstring, EXACT CONSTRUCTIONS) -> (x [M, H] float64, s [M, 1])"""
    s = 2.0 ** ((torch.arange(M) % 6) - 3).to(F64)[:, None]
    sign = torch.ones(M, H, dtype=F64)
    sign[:, :H // 2] = -1.0
    perm = torch.rand(M, H, generator=g).argsort(-1)
    return torch.gather(sign, 1, perm) * s, s


def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


class Inputs(object):
    pass


@functools.lru_cache(maxsize=4)
def inputs(case):
    """The float64 images of the format-exact inputs of `case` and the layout of its buffers."""
    I = Inputs()
    p, k = case.p, case.kind
    g = torch.Generator().manual_seed(_seed(case.name))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    M, H, exact = p["M"], p["H"], p["exact"]
    I.M, I.H, I.eps, I.exact = M, H, p["eps"], exact
    I.degenerate = []
    I.xin = None
    I.flag = 0.0
    I.outs = {}
    pad = 8 if p.get("pad") else 0
    grp = p.get("grp", (0, 0))
    idx = remap_index(M, grp)
    tall = 3 if pad else 0
    # gamma, beta, dy
    if exact:
        I.gamma = _randint(g, -3, 3, H) if k in ("fwd", "emb", "emb_f32", "rows_f32", "drop_f32") else _randint(g, -2, 2, H)
        I.beta = _randint(g, -8, 8, H)
    else:
        I.gamma, I.beta = f32r(1.0 + 0.2 * rn(H)), f32r(0.1 * rn(H))
    # x
    if k in ("emb", "emb_f32", "emb_bwd"):
        B, T, S = p["B"], p["T"], p["S"]
        nw, npos, nt = 50, T + 3, 2
        if exact:
            I.word = exact_rows(g, nw, H)[0]
            I.pos, I.typ = torch.zeros(npos, H, dtype=F64), torch.zeros(nt, H, dtype=F64)
        else:
            w, _ = random_rows(g, nw, H)
            w[7] = rn(H)                                  # (word row 7 not constant; pos and type are added to every row anyway)
            I.word, I.pos, I.typ = f32r(w), f32r(0.1 * rn(npos, H)), f32r(0.1 * rn(nt, H))
        I.ids = torch.randint(0, nw, (B, T), generator=g)
        I.pos_ids = torch.randint(0, npos, (B, T), generator=g) if p["pos_ids"] else None
        I.type_ids = torch.randint(0, nt, (B, T), generator=g) if p["type_ids"] else None
        if p["bad"]:                                      # one bad id per table, on three different tokens; the kernels clamp
            I.ids[0, 1] = nw + 5
            if I.pos_ids is not None:
                I.pos_ids[1, 0] = -2
            if I.type_ids is not None:
                I.type_ids[1, 3] = nt
        wi = I.ids.clamp(0, nw - 1).view(-1)
        pi = (I.pos_ids.clamp(0, npos - 1) if I.pos_ids is not None else torch.arange(T).expand(B, T)).reshape(-1)
        ti = (I.type_ids.clamp(0, nt - 1) if I.type_ids is not None else torch.zeros(B, T, dtype=torch.long)).reshape(-1)
        I.x = I.word[wi] + I.pos[pi] + I.typ[ti]
        I.x32 = ((I.word[wi].float() + I.pos[pi].float()) + I.typ[ti].float())
        I.xin = 2.0 * E32 * (I.word[wi].abs() + I.pos[pi].abs() + I.typ[ti].abs())
        I.flag = float(p["bad"])
        idx = (torch.arange(B)[:, None] * S + torch.arange(T)[None, :]).reshape(-1)
        I.rows_bs = B * S
    elif k == "apply":
        v = random_rows(g, M, H)[0]
        clamp = [r for r in (32, 33, 34, 35) if r < M] or ([4] if M > 4 else [])
        for r in ([7, M - 2] if M >= 20 else [7]):
            if r < M:
                v[r] = rn(H)                              # the constant rows of this kind are the clamp rows
        for r in clamp:
            v[r] = 0.5
        I.stat_rows = M + 5
        I.stats = row_stats(v, I.stat_rows)
        I.stats[:, M:] = SENTINEL
        for r in clamp:
            I.stats[:, r, 1] *= (1.0 - 2.0 ** -18)
        I.x = f16r(v)
        I.degenerate = clamp
        I.np = H // 128
    elif k == "stream_init":
        x = rn(M, H) * 3.0
        edge = torch.tensor([65504.0, -65504.0, 7e4, -7e4, 1e5, -1e5, 65519.0, 65520.0, 6.1e-5, -5.9e-8, 0.0, 1.0 + 2.0 ** -9])
        x.view(-1)[:min(edge.numel(), x.numel())] = edge[:x.numel()]
        I.x = f32r(x)
        I.np, I.stat_rows = p["np"], M + 3
    elif exact:
        I.x, I.s = exact_rows(g, M, H)
    else:
        x, I.degenerate = random_rows(g, M, H)
        I.x = round_in(x, p.get("xfmt", "f32"))
    # gradients
    if k in ("bwd", "emb_bwd", "bwd_f32"):
        gfmt = "f32" if k == "bwd_f32" else "bf16"
        I.dy = _randint(g, -4, 4, M, H) if exact else round_in(rn(M, H) * (0.5 + torch.rand(M, 1, generator=g)), gfmt)
        I.accumulate = bool(p.get("accumulate"))
        if exact:
            I.prior_g, I.prior_b = _randint(g, -50, 50, H), _randint(g, -50, 50, H)
        else:
            I.prior_g, I.prior_b = f32r(rn(H) * 3.0), f32r(rn(H) * 3.0)
    # dropout sites
    seed = 1000 + _seed(case.name) % 1000
    pdrop = DROP_P_EXACT if exact else DROP_P
    I.drop_out = I.drop_in = None
    if k == "bwd" and p["dx2"]:
        I.drop_out = (pdrop, seed, 5)
    if k in ("emb", "emb_bwd") and p["drop"]:
        if k == "emb":
            I.drop_out = (pdrop, seed, SITE_EMB)
        else:
            I.drop_in = (pdrop, seed, SITE_EMB)
    if k == "drop_f32":
        I.drop_out = (pdrop, seed, 0xE1)
    if k == "bwd_f32":
        if p["drop_in"]:
            I.drop_in = (pdrop, seed, SITE_EMB)
        if p["drop_out"]:
            I.drop_out = (pdrop, seed, 10)
    km = lambda d: None if d is None else torch.from_numpy(keep_mask(M * H, d)).view(M, H)
    I.keep_out, I.keep_in = km(I.drop_out), km(I.drop_in)
    I.idx, I.grp = idx, grp
    # layouts
    rows = (I.rows_bs if k.startswith("emb") else (int(idx.max()) + 1)) + tall
    if k == "fwd":
        I.x_buf = Buf(p["xfmt"], M, H, H + pad, rows, idx)
        I.outs["y"] = Buf("bf16", M, H, H + 2 * pad, rows, idx)
        if p["yh"]:
            I.outs["yh"] = Buf("f16", M, H, H + 3 * pad, rows, idx)
        if p["stats"]:
            I.outs["mean"], I.outs["rstd"] = Buf("f32", M, 1, 1, M + tall), Buf("f32", M, 1, 1, M + tall)
    elif k == "bwd":
        I.x_buf, I.dy_buf = Buf(p["xfmt"], M, H, H + pad, rows), Buf("bf16", M, H, H + 2 * pad, rows)
        I.outs["dx"] = Buf("bf16", M, H, H + pad, rows)
        if p["dx2"]:
            I.outs["dx2"] = Buf("bf16", M, H, H + 3 * pad, rows)
    elif k in ("emb", "emb_f32"):
        I.outs["y"] = Buf("bf16" if k == "emb" else "f32", M, H, H + pad, rows, idx)
        I.outs["flag"] = Buf("i32", 1, 1)
    elif k == "emb_bwd":
        I.dy_buf = Buf("bf16", M, H, H + pad, rows, idx)
        I.outs["dx"] = Buf("f32", M, H)
    elif k == "rows_f32":
        I.x_buf = Buf(p["xfmt"], M, H, H + pad, rows, idx)
        I.outs["y"] = I.x_buf if p.get("inplace") else Buf(p["yfmt"], M, H, H + 2 * pad, rows, idx)
    elif k == "drop_f32":
        I.x_buf = Buf("f32", M, H, H + pad, M)
        I.outs["y"] = Buf("f32", M, H, H + 2 * pad, rows, idx)
    elif k == "bwd_f32":
        I.x_buf, I.dy_buf = Buf("f32", M, H, H + pad, M), Buf("f32", M, H, H + 2 * pad, rows, idx)
        if not p["no_dx"]:
            I.outs["dx"] = Buf("f32", M, H, H + pad, M + tall)
        if p["drop_out"]:
            I.outs["dx2"] = Buf("f32", M, H, H + 2 * pad, M + tall)
    elif k == "apply":
        I.x_buf = Buf("f16", M, H, H + pad, M + tall)
        if "bf16" in p["outs"]:
            I.outs["y16"] = Buf("bf16", M, H, H + pad, M + tall)
        if "f32" in p["outs"]:
            I.outs["y32"] = Buf("f32", M, H, H + 2 * pad, M + tall)
    elif k == "stream_init":
        I.x_buf = Buf("f32", M, H, H + pad, M + tall)
        I.outs["stream"], I.outs["copy"] = Buf("f16", M, H, H + pad, M + tall), Buf("bf16", M, H, H + 2 * pad, M + tall)
        sidx = (torch.arange(I.np)[:, None] * I.stat_rows + torch.arange(M)[None, :]).reshape(-1)
        I.outs["stats"] = Buf("f32", I.np * M, 2, 2, I.np * I.stat_rows, sidx)
    if k in ("bwd", "emb_bwd", "bwd_f32"):
        I.outs["dgamma"], I.outs["dbeta"] = Buf("f32", 1, H, H + 4), Buf("f32", 1, H, H + 4)
    return I


def initial(case, name):
    """What output buffer `name` holds before the call: the sentinel; the prior of an accumulated sum; x itself in place."""
    I = inputs(case)
    spec = I.outs[name]
    if name in ("dgamma", "dbeta") and I.accumulate:
        return spec.place((I.prior_g if name == "dgamma" else I.prior_b)[None, :])
    if case.get("inplace") and name == "y":
        return spec.place(I.x)
    if name == "flag":
        return torch.zeros(1, 1, dtype=torch.int32)
    return spec.blank()


# ---- the arithmetic in float64 ------------------------------------------------------------------------------------------------
FWD_MUTANTS = ("mean_rounded_to_bf16", "rstd_rounded_to_bf16", "eps_outside_the_root", "unbiased_variance", "one_pass_variance_in_fp32",
               "output_truncated", "fp16_output_from_the_bf16_output", "dropout_scale_missing", "dropout_mask_of_the_remapped_row")
BWD_MUTANTS = ("dx_dropped_from_the_rounded_dx", "m2_omitted", "mean_of_dy_instead_of_dy_gamma", "dgamma_with_gamma",
               "accumulate_overwrites", "output_truncated", "dropout_scale_missing", "dropout_mask_of_the_remapped_row")
APPLY_MUTANTS = ("ln_var_unclamped_negative", "output_truncated")
STRUCTURAL_MUTANTS = ("last_chunk_columns_skipped", "tail_row_stored_into_row_M", "one_partial_row_dropped",
                      "one_grid_stride_iteration_skipped", "gap_rows_written")
MUTANTS = tuple(dict.fromkeys(FWD_MUTANTS + BWD_MUTANTS + APPLY_MUTANTS + STRUCTURAL_MUTANTS))


def fwd_values(x, gamma, beta, eps, mutant=None):
    H = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    if mutant == "mean_rounded_to_bf16":
        mean = bf16r(mean)
    xc = x - mean
    if mutant == "one_pass_variance_in_fp32":
        var = f32r(f32r((x * x).mean(-1, keepdim=True)) - f32r(mean * mean))
    else:
        var = (xc * xc).mean(-1, keepdim=True)
    if mutant == "unbiased_variance" and H > 1:
        var = var * H / (H - 1)
    rstd = 1.0 / (torch.sqrt(var) + eps) if mutant == "eps_outside_the_root" else 1.0 / torch.sqrt(var + eps)
    if mutant == "rstd_rounded_to_bf16":
        rstd = bf16r(rstd)
    xhat = xc * rstd
    return mean, var, rstd, xhat, xhat * gamma + beta


class Terms(object):
    """The float64 LayerNorm of x and the magnitudes of the module docstring's bounds."""

    def __init__(self, x, gamma, beta, eps, xin=None):
        H = x.shape[-1]
        self.H = H
        self.mean, self.var, self.rstd, self.xhat, self.y = fwd_values(x, gamma, beta, eps)
        self.dmean = (H + 2) * E32 * x.abs().mean(-1, keepdim=True)
        ve = self.var + eps
        # (a constant row at eps = 0 cannot occur: the exact constructions have var = s^2)
        self.rho = (H / 2.0 + 4.0) * E32 + self.dmean ** 2 / (2.0 * ve)
        direct = 0.0
        if xin is not None:
            self.dmean = self.dmean + xin.mean(-1, keepdim=True)
            self.rho = (H / 2.0 + 4.0) * E32 + self.dmean ** 2 / (2.0 * ve) + ((x - self.mean).abs() * xin).mean(-1, keepdim=True) / ve
            direct = xin * self.rstd
        self.ex = self.dmean * self.rstd + self.xhat.abs() * (self.rho + 2.0 * E32) + direct
        self.E = (self.dmean * self.rstd + direct) * gamma.abs() + (self.xhat * gamma).abs() * (self.rho + 3.0 * E32) + E32 * self.y.abs()
        self.gamma = gamma

    def vacuity(self):
        return (self.dmean * self.rstd).view(-1)


def _ref(y, bound, fmt, rounding=None):
    """a Ref that also names the part of its bound that is the final rounding of the output (the host test's "half" rule is about
    the rest)"""
    r = Ref(y, bound, fmt)
    r.rounding = torch.zeros_like(bound) if rounding is None else rounding
    return r


def _out_ref(y, E, fmt, keep=None, scale=1.0):
    """Ref of an output rounded once from an fp32 value with error E; under dropout: dropped exactly 0, kept y s."""
    u = U_OUT[fmt]
    if keep is not None:
        kf = keep.to(F64)
        y = y * kf * scale
        E = (E * scale + E32 * y.abs()) * kf
    return _ref(y, u * y.abs() + (1.0 + u) * E, fmt, u * y.abs())


def _exact_ref(y, fmt):
    y = round_out(y, fmt)
    return _ref(y, torch.zeros_like(y), fmt)


def _is_pow2(n):
    return n & (n - 1) == 0


def _scale(d):
    return 1.0 if d is None else drop_scale(d[0])


def _apply_rows(I, mutant=None):
    o = Inputs()
    o.stats, o.M, o.H, o.mode = I.stats, I.M, I.H, 2
    return _ln_row_terms(o, mutant)


_VAC = {}


def vacuity(case):
    """dmean rstd per row (ln_apply: (rho + 2^-20) |mean| rstd), from the reference alone; None for ln_stream_init."""
    reference(case)
    return _VAC.get(case.name)


@functools.lru_cache(maxsize=4)
def reference(case):
    """{output: Ref} of `case` (logical shapes): the float64 values and the module docstring's bounds; bound 0 where equality is
    demanded (exact constructions, dropped elements, ln_stream_init)."""
    I, k, p = inputs(case), case.kind, case.p
    out = {}
    exact = I.exact
    if k == "stream_init":
        st = torch.zeros(I.np, I.M, 2, dtype=F64)
        st[0, :, 1] = float(np.float32(I.H) * (np.float32(1.0) - np.float32(I.eps)))
        return {"stream": _exact_ref(I.x, "f16"), "copy": _exact_ref(I.x, "bf16"), "stats": _exact_ref(st.view(-1, 2), "f32")}
    if k == "apply":
        mean, rstd, rho = _apply_rows(I)
        y = (I.x - mean) * rstd * I.gamma + I.beta
        E = (rho + 2.0 ** -20) * I.gamma.abs() * (I.x.abs() + mean.abs()) * rstd + 2.0 ** -22 * I.beta.abs()
        _VAC[case.name] = ((rho + 2.0 ** -20) * mean.abs() * rstd).view(-1)
        for name, fmt in (("y16", "bf16"), ("y32", "f32")):
            if name in I.outs:
                out[name] = _out_ref(y, E, fmt)
        return out
    t = Terms(I.x, I.gamma, I.beta, I.eps, I.xin)
    _VAC[case.name] = t.vacuity()
    if k in ("fwd", "emb", "emb_f32", "rows_f32", "drop_f32"):
        s = _scale(I.drop_out)
        for name, spec in I.outs.items():
            if name in ("y", "yh"):
                if exact:
                    yy = t.y if I.keep_out is None else t.y * I.keep_out.to(F64) * s
                    out[name] = _exact_ref(yy, spec.fmt)
                else:
                    out[name] = _out_ref(t.y, t.E, spec.fmt, I.keep_out, s)
            elif name == "mean":
                out[name] = _exact_ref(t.mean, "f32") if exact else _ref(t.mean, t.dmean, "f32")
            elif name == "rstd":
                out[name] = _exact_ref(t.rstd, "f32") if exact else _ref(t.rstd, t.rstd * (t.rho + 2.0 * E32), "f32")
            elif name == "flag":
                out[name] = _ref(torch.full((1, 1), I.flag, dtype=F64), torch.zeros(1, 1, dtype=F64), "f32")
        return out
    # backward
    M, H = I.M, I.H
    dy = I.dy
    if I.keep_in is not None:
        dy = dy * I.keep_in.to(F64) * _scale(I.drop_in)
    g = dy * I.gamma
    m1, m2 = g.mean(-1, keepdim=True), (g * t.xhat).mean(-1, keepdim=True)
    dx = t.rstd * (g - m1 - t.xhat * m2)
    dm1 = (H + 2) * E32 * g.abs().mean(-1, keepdim=True)
    dm2 = (H + 2) * E32 * (g * t.xhat).abs().mean(-1, keepdim=True) + (g.abs() * t.ex).mean(-1, keepdim=True)
    eg = (2.0 if I.keep_in is not None else 1.0) * E32 * g.abs()
    Edx = t.rstd * (eg + dm1 + t.xhat.abs() * dm2 + t.ex * m2.abs()) + (t.rho + 4.0 * E32) * t.rstd * (g.abs() + m1.abs() + (t.xhat * m2).abs())
    dx_exact = exact and _is_pow2(H)
    s = _scale(I.drop_out)
    for name, spec in I.outs.items():
        if name == "dx":
            out[name] = _exact_ref(dx, spec.fmt) if dx_exact else _out_ref(dx, Edx, spec.fmt)
        elif name == "dx2":
            if dx_exact:
                out[name] = _exact_ref(dx * I.keep_out.to(F64) * s, spec.fmt)
            else:
                out[name] = _out_ref(dx, Edx, spec.fmt, I.keep_out, s)
    dgam, dbet = (dy * t.xhat).sum(0, keepdim=True), dy.sum(0, keepdim=True)
    Eg = (dy.abs() * t.ex).sum(0, keepdim=True) + (M + 8) * E32 * (dy * t.xhat).abs().sum(0, keepdim=True)
    Eb = (M + 8) * E32 * dy.abs().sum(0, keepdim=True)
    rg = rb = None
    if I.accumulate:
        dgam, dbet = dgam + I.prior_g, dbet + I.prior_b
        rg, rb = E32 * dgam.abs(), E32 * dbet.abs()
        Eg, Eb = Eg + rg, Eb + rb
    out["dgamma"] = _exact_ref(dgam, "f32") if exact else _ref(dgam, Eg, "f32", rg)
    out["dbeta"] = _exact_ref(dbet, "f32") if exact else _ref(dbet, Eb, "f32", rb)
    return out


# ---- the minimal model and its mutants -----------------------------------------------------------------------------------------
def mutant_applies(mutant, case):
    """(from the case's parameters alone: the test collection asks for every case)"""
    k, p = case.kind, case.p
    exact, grp, M, H = p["exact"], p.get("grp", (0, 0)), p["M"], p["H"]
    fwd = k in ("fwd", "emb", "emb_f32", "rows_f32", "drop_f32")
    bwd = k in ("bwd", "emb_bwd", "bwd_f32")
    narrow = k in ("fwd", "bwd", "emb") or (k == "rows_f32" and p["yfmt"] == "bf16") or (k == "apply" and "bf16" in p["outs"])
    drop = {"bwd": p.get("dx2"), "emb": p.get("drop"), "emb_bwd": p.get("drop"), "drop_f32": True,
            "bwd_f32": p.get("drop_in") or p.get("drop_out")}.get(k, False)
    rule = {
        "mean_rounded_to_bf16": fwd and not exact, "rstd_rounded_to_bf16": fwd and not exact,
        "eps_outside_the_root": fwd and p["eps"] >= 1e-6, "unbiased_variance": fwd,
        "one_pass_variance_in_fp32": fwd and not exact and M >= 4,
        "output_truncated": narrow and not exact,
        "fp16_output_from_the_bf16_output": k == "fwd" and p["yh"] and not exact,
        "dropout_scale_missing": drop,
        "dropout_mask_of_the_remapped_row": k in ("drop_f32", "bwd_f32") and bool(grp[0]) and drop and M > grp[0],
        "dx_dropped_from_the_rounded_dx": k == "bwd" and p["dx2"] and not exact,
        "m2_omitted": bwd, "mean_of_dy_instead_of_dy_gamma": bwd, "dgamma_with_gamma": bwd,
        "accumulate_overwrites": bwd and p.get("accumulate"),
        "ln_var_unclamped_negative": k == "apply" and M > 4,
        "last_chunk_columns_skipped": exact and k != "stream_init" and H > 8,
        "tail_row_stored_into_row_M": exact and k in ("fwd", "rows_f32") and p.get("pad"),
        "one_partial_row_dropped": exact and bwd and M > 4,
        "one_grid_stride_iteration_skipped": exact and any(e.endswith("second trip round the grid-stride loop") for e in p.get("enters", ())),
        "gap_rows_written": exact and bool(grp[0]) and k in ("fwd", "rows_f32", "drop_f32") and M > grp[0],
    }
    return bool(rule[mutant])


def _grid_rows(case):
    _, R, nb = case_dispatch(case, FAMILY_ENV[family_of(case)])
    return 4 * nb * R


@functools.lru_cache(maxsize=None)
def family_of(case):
    for fam in FAMILY_ENV:
        if case in cases(fam):
            return fam
    raise KeyError(case)


def model(case, mutant=None):
    """{output: physical buffer}: float64 everywhere, every output rounded once; `mutant` changes one thing."""
    I, k, p = inputs(case), case.kind, case.p
    M, H = I.M, I.H
    trunc = mutant == "output_truncated"
    logical = {}
    if k == "stream_init":
        ref = reference(case)
        logical = {n: r.y for n, r in ref.items()}
    elif k == "apply":
        mean, rstd, _ = _apply_rows(I, mutant if mutant == "ln_var_unclamped_negative" else None)
        y = (I.x - mean) * rstd * I.gamma + I.beta
        logical = {n: round_out(y, s.fmt, trunc) for n, s in I.outs.items()}
    else:
        keep_out, keep_in = I.keep_out, I.keep_in
        if mutant == "dropout_mask_of_the_remapped_row":
            d = I.drop_out if I.drop_out is not None else I.drop_in
            top = int(I.idx.max()) + 1
            wrong = torch.from_numpy(keep_mask(top * H, d)).view(top, H)[I.idx]
            keep_out = wrong if I.drop_out is not None else None
            keep_in = wrong if I.drop_in is not None else keep_in
        s_out = 1.0 if mutant == "dropout_scale_missing" else _scale(I.drop_out)
        s_in = 1.0 if mutant == "dropout_scale_missing" else _scale(I.drop_in)
        if k in ("fwd", "emb", "emb_f32", "rows_f32", "drop_f32"):
            mean, var, rstd, xhat, y = fwd_values(I.x, I.gamma, I.beta, I.eps, mutant)
            if keep_out is not None:
                y = y * keep_out.to(F64) * s_out
            for n, spec in I.outs.items():
                if n == "y":
                    logical[n] = round_out(y, spec.fmt, trunc)
                elif n == "yh":
                    logical[n] = round_out(bf16r(y) if mutant == "fp16_output_from_the_bf16_output" else y, "f16", trunc)
                elif n == "mean":
                    logical[n] = f32r(mean)
                elif n == "rstd":
                    logical[n] = f32r(rstd)
                elif n == "flag":
                    logical[n] = torch.full((1, 1), I.flag, dtype=F64)
        else:
            _, _, rstd, xhat, _ = fwd_values(I.x, I.gamma, I.beta, I.eps)
            dy = I.dy if keep_in is None else I.dy * keep_in.to(F64) * s_in
            g = dy * I.gamma
            m1 = (dy if mutant == "mean_of_dy_instead_of_dy_gamma" else g).mean(-1, keepdim=True)
            m2 = torch.zeros(M, 1, dtype=F64) if mutant == "m2_omitted" else (g * xhat).mean(-1, keepdim=True)
            dx = rstd * (g - m1 - xhat * m2)
            rows = torch.ones(M, dtype=torch.bool)
            if mutant == "one_partial_row_dropped":       # the rows of workgroup 1 (four waves, one row group each per trip)
                _, R, nb = case_dispatch(case, FAMILY_ENV[family_of(case)])
                rows = ((torch.arange(M) // R) // 4) % nb != min(1, nb - 1)
            if mutant == "one_grid_stride_iteration_skipped":
                gr = _grid_rows(case)
                rows = ~((torch.arange(M) >= gr) & (torch.arange(M) < 2 * gr))
            rw = rows.to(F64)[:, None]
            dgam = ((g if mutant == "dgamma_with_gamma" else dy) * xhat * rw).sum(0, keepdim=True)
            dbet = (dy * rw).sum(0, keepdim=True)
            if I.accumulate and mutant != "accumulate_overwrites":
                dgam, dbet = dgam + I.prior_g, dbet + I.prior_b
            for n, spec in I.outs.items():
                if n == "dx":
                    logical[n] = round_out(dx, spec.fmt, trunc)
                elif n == "dx2":
                    src = round_out(dx, spec.fmt) if mutant == "dx_dropped_from_the_rounded_dx" else dx
                    logical[n] = round_out(src * keep_out.to(F64) * s_out, spec.fmt, trunc)
            logical["dgamma"], logical["dbeta"] = f32r(dgam), f32r(dbet)
    bufs = {}
    for n, spec in I.outs.items():
        base = initial(case, n)
        buf = spec.place(logical[n], base)
        wide = spec.n == H and n not in ("dgamma", "dbeta")
        if mutant == "last_chunk_columns_skipped" and wide:
            c0 = ((H - 1) // 512) * 512 if H > 512 else H - 8
            buf[:, c0:H] = base[:, c0:H]
        if mutant == "tail_row_stored_into_row_M" and wide and spec.rows > int(spec.index.max()) + 1:
            buf[int(spec.index.max()) + 1, :spec.n] = buf[int(spec.index.max()), :spec.n]
        if mutant == "one_grid_stride_iteration_skipped" and wide and spec.M == M:
            gr = _grid_rows(case)
            sk = spec.index[gr:2 * gr]
            buf[sk] = base[sk]
        if mutant == "gap_rows_written" and wide and I.grp[0] and spec.rows > M:
            gap = torch.ones(spec.rows, dtype=torch.bool)
            gap[spec.index] = False
            gap[int(spec.index.max()) + 1:] = False
            buf[gap, :spec.n] = buf[int(spec.index[0]), :spec.n]
        bufs[n] = buf
    return bufs


# ---- judging ------------------------------------------------------------------------------------------------------------------
def signed_case(case):
    I = inputs(case)
    # every kind: judge() takes the statistic on each bf16 / fp16 output of width H; ln_stream_init's outputs are compared for
    # equality (bound 0 everywhere, which the statistic leaves out)
    return I.M * I.H >= 100000 and not I.exact and case.kind != "stream_init"


def judge(case, bufs):
    """{check: measured / bound} of the physical output buffers of `case`; every value must lie in [0, 1] (signed bias: [-1, 1])."""
    I, ref = inputs(case), reference(case)
    rs = {}
    for name, spec in I.outs.items():
        got, pad_ok = spec.read(bufs[name], initial(case, name))
        rs[name + " padding"] = 0.0 if pad_ok else INF
        if not bool(torch.isfinite(got).all()):
            rs[name + " err/bound"] = INF
            continue
        signed = signed_case(case) and spec.fmt in ("bf16", "f16") and spec.n == I.H
        rs.update(hg.ratios(ref[name], got, name, signed=signed))
    return rs


def assert_ratios(name, rs):
    """Every ratio through helpers.check_close (recorded, asserted against 1) -> the messages of those that failed, so that a caller
    can walk all its cases before it fails."""
    from helpers import check_close

    failed = []
    for key in sorted(rs):
        try:
            check_close("ln conformance %s: %s" % (name, key), abs(rs[key]), 0.0, 1.0)
        except AssertionError as e:
            failed.append(str(e))
    return failed


# ---- fp32 emulation in three summation orders -----------------------------------------------------------------------------------
def sum32(a, order):
    """float32 sum over the last axis of a float32 array: one add at a time ("sequential"), a balanced tree ("pairwise"), or the
    kernels' order ("lanes": lane l of 64 adds its own eight-column groups l, l + 64, ... one element at a time, then the butterfly
    over the lanes)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    n = a.shape[-1]
    if order == "sequential":
        return np.add.accumulate(a, axis=-1, dtype=np.float32)[..., -1]
    if order == "lanes":
        ch = (n + 511) // 512
        z = np.zeros(a.shape[:-1] + (ch * 512,), dtype=np.float32)
        z[..., :n] = a
        z = z.reshape(a.shape[:-1] + (ch, 64, 8)).swapaxes(-3, -2).reshape(a.shape[:-1] + (64, ch * 8))
        a = np.add.accumulate(z, axis=-1, dtype=np.float32)[..., -1]
        n = 64
    m = 1 << max(0, (n - 1).bit_length())
    z = np.zeros(a.shape[:-1] + (m,), dtype=np.float32)
    z[..., :n] = a
    while m > 1:
        m //= 2
        z = z[..., :m] + z[..., m:2 * m] if order == "lanes" else z[..., 0::2] + z[..., 1::2]
    return z[..., 0]


def emulation(case, order):
    """{output: unrounded float64 logical values} of the stated operations in float32, sums taken in `order`."""
    I, k = inputs(case), case.kind
    f = np.float32
    M, H = I.M, I.H
    n32 = lambda t: t.numpy().astype(f)
    gamma, beta, eps = n32(I.gamma), n32(I.beta), f(I.eps)
    out = {}
    if k == "stream_init":
        return {n: r.y for n, r in reference(case).items()}
    invH = f(1.0) / f(H)
    if k == "apply":
        st = I.stats.numpy()[:, :M]
        s, q = sum32(st[..., 0].T, "sequential"), sum32(st[..., 1].T, "sequential")
        mean = s * invH
        rstd = f(1.0) / np.sqrt(np.maximum(q * invH - mean * mean, f(0.0)) + eps)
        y = (n32(I.x) - mean[:, None]) * rstd[:, None] * gamma + beta
        return {n: torch.from_numpy(y.astype(np.float64)) for n in I.outs}
    x = I.x32.numpy() if hasattr(I, "x32") else n32(I.x)
    mean = sum32(x, order) * invH
    d = x - mean[:, None]
    rstd = f(1.0) / np.sqrt(sum32(d * d, order) * invH + eps)
    xhat = d * rstd[:, None]
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    if k in ("fwd", "emb", "emb_f32", "rows_f32", "drop_f32"):
        y = xhat * gamma + beta
        if I.keep_out is not None:
            y = y * I.keep_out.numpy().astype(f) * f(_scale(I.drop_out))
        for n in I.outs:
            out[n] = {"y": t64(y), "yh": t64(y), "mean": t64(mean[:, None]), "rstd": t64(rstd[:, None]),
                      "flag": torch.full((1, 1), I.flag, dtype=F64)}[n]
        return out
    dy = n32(I.dy)
    if I.keep_in is not None:
        dy = dy * I.keep_in.numpy().astype(f) * f(_scale(I.drop_in))
    g = dy * gamma
    m1, m2 = sum32(g, order) * invH, sum32(g * xhat, order) * invH
    dx = rstd[:, None] * (g - m1[:, None] - xhat * m2[:, None])
    if "dx" in I.outs:
        out["dx"] = t64(dx)
    if "dx2" in I.outs:
        out["dx2"] = t64(dx * I.keep_out.numpy().astype(f) * f(_scale(I.drop_out)))
    dgam, dbet = sum32((dy * xhat).T, order), sum32(dy.T, order)
    dgam, dbet = t64(dgam[None, :]), t64(dbet[None, :])
    if I.accumulate:                                      # (unrounded, like every output of the emulation)
        dgam, dbet = I.prior_g + dgam, I.prior_b + dbet
    out["dgamma"], out["dbeta"] = dgam, dbet
    return out


# ---- running a case on the device -----------------------------------------------------------------------------------------------
def run(case, dev):
    """`case` through its visitron_amd.ops entry point -> {output: physical buffer on the CPU}."""
    from visitron_amd import ops

    I, k, p = inputs(case), case.kind, case.p
    M, H, eps = I.M, I.H, I.eps
    F32 = torch.float32
    up = lambda t, dt=F32: t.to(dt).to(dev)
    bufs = {n: initial(case, n).to(dev) for n in I.outs}
    gamma, beta = up(I.gamma), up(I.beta)
    drop = lambda d: ops.NO_DROP if d is None else d
    flat = lambda n: bufs[n].view(-1) if n in bufs else None
    if k == "fwd":
        x = I.x_buf.place(I.x).to(dev)
        ops.layernorm(x, gamma, beta, eps, out=bufs["y"], mean=flat("mean"), rstd=flat("rstd"), M=M, grp_rows=I.grp[0],
                      grp_stride=I.grp[1], out_h=bufs.get("yh"))
    elif k == "bwd":
        x, dy = I.x_buf.place(I.x).to(dev), I.dy_buf.place(I.dy).to(dev)
        if p["gamma_off"]:
            holder = torch.zeros(H + 8, dtype=F32, device=dev)
            holder[1:H + 1] = gamma
            gamma = holder[1:H + 1]
            assert gamma.data_ptr() % 16 == 4
        ops.layernorm_bwd(x, dy, gamma, eps, flat("dgamma"), flat("dbeta"), dx=bufs["dx"], accumulate=I.accumulate, M=M,
                          dx_dropped=bufs.get("dx2"), drop=drop(I.drop_out))
    elif k in ("emb", "emb_f32", "emb_bwd"):
        ids = I.ids.to(dev)
        tids = None if I.type_ids is None else I.type_ids.to(dev)
        pids = None if I.pos_ids is None else I.pos_ids.to(dev)
        word, pos, typ = up(I.word), up(I.pos), up(I.typ)
        if k == "emb":
            ops.embed_layernorm(ids, tids, pids, word, pos, typ, gamma, beta, eps, bufs["y"], p["S"], err_flag=flat("flag"),
                                drop=drop(I.drop_out))
        elif k == "emb_f32":
            ops.embed_layernorm_f32(ids, tids, pids, word, pos, typ, gamma, beta, eps, bufs["y"], p["S"], err_flag=flat("flag"))
        else:
            g = I.dy_buf.place(I.dy).to(dev)
            bufs["dx"] = ops.embed_layernorm_bwd(ids, tids, pids, word, pos, typ, gamma, eps, g, p["S"], flat("dgamma"), flat("dbeta"),
                                                 accumulate=I.accumulate, drop=drop(I.drop_in))
    elif k == "rows_f32":
        if p.get("inplace"):
            x = bufs["y"]
        else:
            x = I.x_buf.place(I.x).to(dev)
        ops.layernorm_rows(x, gamma, beta, eps, out=bufs["y"], M=M, grp_rows=I.grp[0], grp_stride=I.grp[1])
    elif k == "drop_f32":
        x = I.x_buf.place(I.x).to(dev)
        ops.layernorm_drop_f32(x, gamma, beta, eps, bufs["y"], M=M, grp_rows=I.grp[0], grp_stride=I.grp[1], drop=drop(I.drop_out))
    elif k == "bwd_f32":
        x, g = I.x_buf.place(I.x).to(dev), I.dy_buf.place(I.dy).to(dev)
        ops.layernorm_bwd_f32(x, g, gamma, eps, flat("dgamma"), flat("dbeta"), dx=bufs.get("dx"), dx_drop=bufs.get("dx2"),
                              accumulate=I.accumulate, M=M, grp_rows=I.grp[0], grp_stride=I.grp[1], drop_in=drop(I.drop_in),
                              drop_out=drop(I.drop_out))
    elif k == "apply":
        vs = I.x_buf.place(I.x).to(dev)
        ops.ln_apply(vs, I.stats.to(dev), gamma, beta, eps, out16=bufs.get("y16"), out32=bufs.get("y32"), M=M)
    elif k == "stream_init":
        x = I.x_buf.place(I.x).to(dev)
        st = bufs["stats"].view(I.np, I.stat_rows, 2)
        ops.ln_stream_init(x[:, :H], bufs["stream"], bufs["copy"], st, eps, M=M)
    torch.cuda.synchronize()
    return {n: b.cpu() for n, b in bufs.items()}
