"""fp64 reference, derived per-element bound, exact constructions, turn-order fingerprint, restated dispatch rule, model with a mutant
table, fp32 emulation and the case table of the weight-gradient family behind vt_wgrad_bf16 (csrc/gemm_wgrad.hip, gemm_wgrad_v8.hip
with wgrad_v8_step.inc).

Everything here is plain torch / numpy on the CPU in float64, taken from the bf16-exact operands (the one exception: the two
float64 products of a case of more than 2^31 multiply-adds are formed with torch.matmul in float64 on the device, as
tests/test_gpu_deterministic.py does).  tests/test_host_wgrad_reference.py proves without a GPU that the bound accepts the documented
arithmetic and rejects a table of subtly wrong implementations; tests/test_gpu_wgrad_conformance.py holds the HIP kernels to it.
Nothing below was chosen by looking at a kernel's output.

REFERENCE      dW = [dW0 +] dY^T X,  db = [db0 +] colsum(dY)  in float64; dW0 / db0 only under `accumulate`.

BOUND, per element (the form and the reasoning of helpers_gemm, with the reduction length M):

    |got - y| <= 2^-24 |y| + (1 + 2^-24) F
    F = (M + 8) 2^-23 (sum_m |dy_mn x_mk| + |dW0_nk|)
    db: the same with x = 1

  A product of two bf16 values has 16 significant bits and is exact in fp32.  A sum of M such products accumulated in fp32 in ANY
  order (any split into MFMA blocks, row ranges, atomics) carries at most M - 1 roundings on its longest chain, each at most one ulp
  of a partial sum that is itself at most S = sum_m |dy x| (1 + small): one ulp = 2^-23 of the value, because MFMA's inner sum is not
  documented as round to nearest (twice the RN bound 2^-24).  "+ 8" covers the adds of the row ranges' partial sums to one
  another (the persistent kernel cuts a reduction into at most nk / 8 ranges: 8 at the table's largest atomic case, each range
  shortening the chains inside it by more than the one add it costs) and the final add of dW0, whose magnitude joins S.  The
  output is the fp32 value itself, so the u |y| term is the last rounding, 2^-24 |y|.
  The bound is knowingly slack (real fp32 sums err like sqrt M, not M; fp32 emulations in three orders measure 0.009 of it at M = 65,
  8e-4 at M = 1 000): its job is arithmetic done in the wrong precision and wrong operands.  STRUCTURE (a dropped / duplicated /
  misplaced row, block, range, tile or column) is the exact constructions' job.  The signed-bias statistic of the other families is
  not applied: the output is fp32 and MFMA's rounding is not documented.

EXACT CONSTRUCTIONS  dy in [-2, 2], x in [-4, 4], dW0 and db0 in [-16, 16], integers.  With M <= 12 400 every partial sum in any
  order and any split is an integer below 2^24 (computed per case by integer_partial_sum_cap, not assumed), so the fp32 result must
  EQUAL the float64 reference: dW and db, every form, the fp32-atomic one too.  Every case of the table runs with random bf16 data
  against the bound, with the integer construction against bound 0 and with the ROW CENSUS against bound 0: dY one-hot per row at
  column m % N, X one-hot at column (m // N) % K, so that dW[n, k] counts the token rows {m : m % N = n, (m // N) % K = k} (one row
  per element while N K >= M) and a failure names the missing or duplicated rows (census_report).

TURN-ORDER FINGERPRINT (exact).  On the elements (n in Nf, k in Kf) of the accumulating problem: dW0 = 2^24; rows 0, 1, 2 (range 0)
  carry dy = x = 1: sum 3; the first 256 rows of range 1 carry dy = -256, x = 256: sum -2^24, every partial sum a multiple of
  65 536.  In fp32  (dW0 + r0) + r1 = 4,  (dW0 + r1) + r0 = 3,  dW0 + (r0 + r1) = 3  (2^24 + 3 is a tie and rounds to even, 2^24 + 4).
  Deterministic two-range form: exactly 4.  One accumulator chain (one-tile kernels, one row range): exactly 3.  Ticket order with two
  ranges: a member of {3, 4}.  The fp32-atomic form is left out (more than two ranges: the construction does not apply).  "Range 1"
  begins at row 64 ceil(nk / 2), nk = ceil(M / 64), which is where the persistent kernel cuts two ranges.

DISPATCH RULE RESTATED  dispatch() restates vt_wgrad_dispatch (gemm_wgrad.hip) and vt_wgrad_v8_dispatch (gemm_wgrad_v8.hip) as a
  function of (problems, M, hook, deterministic, VT_WGRAD_PERSISTENT_MIN_ROWS / VT_WGRAD_SPLIT / VT_WGRAD_ORDER, CU count).  Every case
  names the form it is meant to reach; before it runs the rule must name the same one.  Where nothing observable distinguishes two
  forms (one-tile 128 against the persistent kernel with one range) the rule is the only evidence.

OPERAND PLACEMENT  dY and X are views inside NaN-filled buffers: PRE rows before row 0, POST rows from row M on, the padding
  columns N .. ldy - 1 and K .. ldx - 1; bases 16-byte aligned, ldy and ldx multiples of 8, ldw a multiple of 4 and > K in some
  cases.  dW and db live in sentinel-filled buffers; in overwrite mode the window itself holds NaN.  The result must be finite and
  inside the bound (or exact) and every sentinel outside the window bitwise intact.  A correct kernel may LOAD the padding columns
  inside the last 8-column chunk, but they reach only accumulators that are never stored.
"""
import collections
import contextlib
import functools
import zlib

import numpy as np
import torch

from helpers_attention import bf16r

F64 = torch.float64
E32 = 2.0 ** -24
SENTINEL = 12345.0
INF = float("inf")
PRE, POST = 1, 2                  # NaN rows before row 0 / from row M on of every dY and X buffer
DW_PRE, DW_POST = 1, 2            # sentinel rows around the dW window
DB_PRE, DB_POST = 4, 4            # sentinel elements around the db window
BIG = 1 << 31                     # the byte limit of a buffer descriptor (vt_wgrad_dispatch)
BIG_MADDS = 1 << 34               # multiply-adds from which the float64 products are formed on the device (allowed from 2^31)
FP_DW0 = 2.0 ** 24

# csrc/wgrad_common.hpp, gemm_wgrad_v8.hip, switches.def
WG_MAX_PROBLEMS = 8
W8_TURN_MAX = 2
W8_SEM_SLOTS = 8
W8_SEM_TILES = 1024
SWITCH_DEFAULTS = {"VT_WGRAD_PERSISTENT_MIN_ROWS": 12288, "VT_WGRAD_SPLIT": 0, "VT_WGRAD_ORDER": 1}
HOST_CUS = 256

FORM_128, FORM_256 = "one-tile 128", "one-tile 256"
FORM_ONE, FORM_TICKET, FORM_DET, FORM_ATOMIC = ("persistent one range", "persistent turns ticket", "persistent turns deterministic",
                                                "persistent atomic")
FORMS = (FORM_128, FORM_256, FORM_ONE, FORM_TICKET, FORM_DET, FORM_ATOMIC)
FAMILY_ENV = collections.OrderedDict([
    ("default", {}),
    ("split2", {"VT_WGRAD_SPLIT": "2"}),
    ("split2_order0", {"VT_WGRAD_SPLIT": "2", "VT_WGRAD_ORDER": "0"}),
    ("minrows1024", {"VT_WGRAD_PERSISTENT_MIN_ROWS": "1024"}),
])
CHILD_TIMEOUT = {"split2": 150, "split2_order0": 90, "minrows1024": 90}   # seconds, start-up of the process included


def f32r(x):
    return x.to(torch.float32).to(F64)


def _up(x, m):
    return (x + m - 1) // m * m


# ---- problems and cases -------------------------------------------------------------------------------------------------------
class Prob(object):
    """One (dY, X, dW, db) problem: py / px extra 8-column chunks of padding in dY / X, pw extra 4-column chunks in dW."""

    def __init__(self, N, K, db=True, acc=False, py=0, px=0, pw=0):
        self.N, self.K, self.db, self.acc = N, K, db, acc
        self.ldy, self.ldx, self.ldw = _up(N, 8) + 8 * py, _up(K, 8) + 8 * px, K + 4 * pw

    def __repr__(self):
        return "%dx%d%s%s ld %d/%d/%d" % (self.N, self.K, "+db" if self.db else "", " acc" if self.acc else "",
                                         self.ldy, self.ldx, self.ldw)


class Case(object):
    """reaches: the form the launch is meant to take; data: random | exact | census | fingerprint; fp: the fp32 values the
    fingerprint elements may hold; cus_below: the case is computed for devices with fewer CUs than this (None: any)."""

    def __init__(self, name, reaches, why, M, probs, hook, det=False, data="random", fp=None, cus_below=None):
        self.name, self.reaches, self.why, self.M, self.probs = name, reaches, why, M, list(probs)
        self.hook, self.det, self.data, self.fp, self.cus_below = hook, det, data, fp, cus_below

    def __repr__(self):
        return self.name

    @property
    def exact(self):
        return self.data != "random"

    @property
    def madds(self):
        return sum(self.M * p.N * p.K for p in self.probs)

    @property
    def big(self):
        return self.madds > BIG_MADDS

    @property
    def fp_problem(self):
        return [i for i, p in enumerate(self.probs) if p.acc][0]


# ---- the dispatch rule restated -------------------------------------------------------------------------------------------------
def _switch(name, env):
    v = (env or {}).get(name)
    return SWITCH_DEFAULTS[name] if v in (None, "") else int(v)


def remap_branches(total):
    """Which branches of the XCD-contiguous remap `xcd < r ? ... : ...` (r = grid & 7) a grid of `total` workgroups takes."""
    r = total & 7
    out = set()
    if r:
        out.add("xcd < r")
    if total >= 8:
        out.add("xcd >= r")
    return out


def dispatch(probs, M, hook, det, env=None, cus=HOST_CUS):
    """-> dict(form=..., grid=..., remap=...) and for the persistent kernel also nsplit, share, order, nk, tiles and `coords`, the
    set of w8_tile_coords branches its problems take; raises ValueError where the library returns an error."""
    if len(probs) <= 0 or len(probs) > WG_MAX_PROBLEMS or M <= 0:
        raise ValueError("bad shape")
    for p in probs:
        if p.N <= 0 or p.K <= 0:
            raise ValueError("bad shape")
        if p.ldy % 8 or p.ldx % 8 or p.ldw % 4 or p.K % 4:
            raise ValueError("bad alignment")
        if M * p.ldy * 2 >= BIG or M * p.ldx * 2 >= BIG:
            raise ValueError("unsupported")
    tn = hook if hook in (128, 256) else 128
    if hook in (0, 8):
        v8 = _v8_dispatch(probs, M, hook == 8, det, env, cus)
        if v8 is not None:
            return v8
    total = sum(((p.N + tn - 1) // tn) * ((p.K + 127) // 128) for p in probs)
    return dict(form=FORM_256 if tn == 256 else FORM_128, grid=total, remap=remap_branches(total), nsplit=1)


def _v8_dispatch(probs, M, force, det, env, cus):
    if not force and M < _switch("VT_WGRAD_PERSISTENT_MIN_ROWS", env):
        return None
    tiles = 0
    coords = set()
    for p in probs:
        if p.N % 256 or p.K % 256 or 256 * p.ldw * 4 >= BIG:
            return None
        tiles += (p.N // 256) * (p.K // 256)
        coords.add("k-tile outer" if p.N // 256 < p.K // 256 else "n-tile outer")
    nk = (M + 63) >> 6
    if nk < 8 or tiles * nk >= (1 << 30):
        return None
    nsplit = max(1, cus // tiles)
    nsplit = min(nsplit, nk // 8)
    if nsplit == 2 and nk <= 76:
        nsplit = 1
    split_env = _switch("VT_WGRAD_SPLIT", env)
    if 0 < split_env <= nk // 8:
        nsplit = split_env
    if det:
        if nsplit > W8_TURN_MAX:
            return None
        if tiles * nsplit > cus:
            nsplit = 1
    if tiles > W8_SEM_TILES:
        return None
    grid = tiles * nsplit
    share = (nk + nsplit - 1) // nsplit
    order = 1 if (_switch("VT_WGRAD_ORDER", env) == 1 and nsplit == 2 and grid % 8 == 0) else 0
    form = FORM_ONE if nsplit == 1 else FORM_ATOMIC if nsplit > W8_TURN_MAX else FORM_DET if det else FORM_TICKET
    return dict(form=form, grid=grid, remap=remap_branches(grid), nsplit=nsplit, share=share, order=order, nk=nk, tiles=tiles,
                coords=coords)


def case_dispatch(case, env=None, cus=HOST_CUS):
    return dispatch(case.probs, case.M, case.hook, case.det, env, cus)


def fingerprint_expectation(form):
    """The fp32 values a fingerprint element may hold under `form` (None: the construction does not apply)."""
    return {FORM_128: (3.0,), FORM_256: (3.0,), FORM_ONE: (3.0,), FORM_DET: (4.0,), FORM_TICKET: (3.0, 4.0)}.get(form)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
ONE_TILE_M = (1, 63, 64, 65, 127, 129, 200)
ONE_TILE_N = (1, 7, 36, 127, 128, 129, 130, 257)
ONE_TILE_K = (4, 12, 60, 124, 128, 132, 260)
DATA = ("random", "exact", "census")


def _three(name, reaches, why, M, mk, hook, det=False, **kw):
    """The case with random data, with the integer construction and with the row census (fresh Prob objects each)."""
    return [Case("%s %s" % (name, d), reaches, why, M, mk(), hook, det, data=d, **kw) for d in DATA]


def _one_tile_cases(tn):
    form = FORM_256 if tn == 256 else FORM_128
    out = []
    for i in range(40):
        M, N = ONE_TILE_M[i % 7], ONE_TILE_N[i % 8]
        K = ONE_TILE_K[(i + i // 8) % 7]
        db, acc = (i // 3) % 2 == 0, (i // 5) % 2 == 1
        mk = functools.partial(lambda N, K, db, acc, i: [Prob(N, K, db, acc, py=i % 3, px=(i + 1) % 3, pw=i % 3)], N, K, db, acc, i)
        out += _three("w%d M%d %dx%d%s%s" % (tn, M, N, K, " db" if db else "", " acc" if acc else ""), form,
                      "M tail / N tail skip / K-tail chunks redirected out of range / bias only from k-tile 0", M, mk, tn)

    def group8():
        shapes = [(257, 260), (1, 4), (130, 132), (7, 12), (128, 128), (36, 60), (129, 124), (127, 260)]
        return [Prob(n, k, db=j % 3 != 1, acc=j % 2 == 1, py=j % 3, px=(j + 2) % 3, pw=(j + 1) % 3) for j, (n, k) in enumerate(shapes)]

    out += _three("w%d group of 8 M129" % tn, form, "eight problems with their own N, K, leading dimensions, db and accumulate", 129,
                  group8, tn)
    out += _three("w%d M65 512x512 db" % tn, form, "a grid that is a multiple of 8: the second remap branch alone", 65,
                  lambda: [Prob(512, 512, True, False, px=1, pw=2)], tn)
    fp = lambda: [Prob(256, 256, True, True, py=1, pw=1)]  # noqa: E731
    out.append(Case("w%d M1024 256x256 fingerprint" % tn, form, "one accumulator chain: dW0 + (r0 + r1)", 1024, fp(), tn,
                    data="fingerprint", fp=(3.0,)))
    return out


def _v8_group():
    return [Prob(256, 768, True, False, py=1, pw=1), Prob(512, 256, True, False, px=2)]


def _mixed(mk, which=0):
    def make():
        ps = mk()
        for j, p in enumerate(ps):
            p.acc = (j == which)
        return ps
    return make


def _acc(mk):
    def make():
        ps = mk()
        for p in ps:
            p.acc = True
        return ps
    return make


PRODUCTION = ((2304, 768), (768, 768), (3072, 768), (768, 3072))


def _default_cases():
    out = _one_tile_cases(128) + _one_tile_cases(256)
    out += _three("auto M1024 256x256 below the row threshold", FORM_128, "eligible by shape, too few rows: hook 0 keeps the one-tile "
                  "kernel", 1024, lambda: [Prob(256, 256, True, False)], 0)
    # persistent kernel, one range
    for M in (1024, 1000):
        one = lambda: [Prob(256, 256, True, False, py=1, px=1, pw=1)]  # noqa: E731
        why = "one row range%s" % (", M tail inside the last block" if M % 64 else "")
        out += _three("v8 one range M%d 256x256" % M, FORM_ONE, why, M, one, 8)
        out += _three("v8 one range M%d 256x256 acc" % M, FORM_ONE, why, M, _acc(one), 8)
        out += _three("v8 one range M%d group" % M, FORM_ONE, why + "; both w8_tile_coords branches", M, _v8_group, 8)
        out += _three("v8 one range M%d group mixed" % M, FORM_ONE, why + "; accumulate per problem", M, _mixed(_v8_group, 1), 8)
    out.append(Case("v8 one range M1024 256x256 fingerprint", FORM_ONE, "one accumulator chain", 1024,
                    [Prob(256, 256, True, True, pw=1)], 8, data="fingerprint", fp=(3.0,)))
    # fp32-atomic form
    a4 = lambda: [Prob(256, 256, True, False, py=1, pw=1)]  # noqa: E731
    a4g = lambda: [Prob(256, 256, True, False, py=1, pw=1), Prob(256, 256, True, False, px=1)]  # noqa: E731
    a8 = lambda: [Prob(768, 768, True, False, pw=1), Prob(256, 1024, True, False, py=1, px=1)]  # noqa: E731
    for tag, M, mk, mkg in (("four ranges M2048", 2048, a4, a4g), ("eight ranges M4100", 4100, a8, a8)):
        why = "fp32 atomics into a dW that wgrad_v8_zero cleared"
        out += _three("v8 atomic %s" % tag, FORM_ATOMIC, why, M, mk, 8)
        out += _three("v8 atomic %s acc" % tag, FORM_ATOMIC, "fp32 atomics onto dW0: no zeroing pass", M, _acc(mk), 8)
        out += _three("v8 atomic %s mixed" % tag, FORM_ATOMIC, why + " for the overwritten problem ONLY", M, _mixed(mkg, 0), 8)
    # the encoder layer's group at the production size, hook 0: two ranges of 97 and 96 blocks, 42 rows in the last, map 1
    prod = lambda: [Prob(n, k, True, False) for n, k in PRODUCTION]  # noqa: E731
    why = "193 row blocks in ranges of 97 and 96, M tail of 42 rows, 216 workgroups on map 1"
    out.append(Case("production M12330 exact", FORM_TICKET, why, 12330, prod(), 0, data="exact"))
    out.append(Case("production M12330 acc exact", FORM_TICKET, why, 12330, _acc(prod)(), 0, data="exact"))
    # deterministic mode, parent: more than two ranges go to the one-tile kernel
    out += _three("det M2048 256x256 to the one-tile kernel", FORM_128, "deterministic mode never launches the fp32-atomic form", 2048,
                  a4, 8, det=True)
    out.append(Case("det M2048 256x256 fingerprint", FORM_128, "one accumulator chain", 2048, _acc(a4)(), 8, det=True,
                    data="fingerprint", fp=(3.0,)))
    return out


def _split2_cases(order0=False):
    out = []
    sq = lambda: [Prob(512, 512, True, False, py=1, pw=1)]  # noqa: E731
    wide = lambda: [Prob(256, 768, True, False, px=1)]  # noqa: E731
    g14 = lambda: [Prob(512, 512, True, False, py=1, pw=1), Prob(256, 768, True, False, px=1)]  # noqa: E731
    g16 = lambda: [Prob(512, 512, True, False, py=1, pw=1), Prob(512, 512, True, False, px=1)]  # noqa: E731
    shapes = [("512x512", sq), ("group 2x 512x512", g16)] if order0 else [("512x512", sq), ("256x768", wide), ("group 512x512 + 256x768", g14),
                                                                            ("group 2x 512x512", g16)]
    for det in (False, True):
        form = FORM_DET if det else FORM_TICKET
        for M in (1030, 1100):
            for tag, mk in shapes:
                nk = (M + 63) // 64
                why = "two row ranges of %d and %d blocks, %d rows in the last" % ((nk + 1) // 2, nk - (nk + 1) // 2, M - (nk - 1) * 64)
                pre = "%s M%d %s" % ("det" if det else "ticket", M, tag)
                group = tag.startswith("group")
                if not group:
                    out += _three(pre, form, why, M, mk, 8, det=det)
                    out += _three(pre + " acc", form, why + "; no first_overwrites", M, _acc(mk), 8, det=det)
                else:
                    out += _three(pre + " mixed", form, why + "; first_overwrites per problem", M, _mixed(mk, 1), 8, det=det)
                if M == 1030:
                    fpm = _mixed(mk, 0) if group else _acc(mk)
                    out.append(Case(pre + " fingerprint", form, "(dW0 + range 0) + range 1" if det else "either order of the two turns",
                                    M, fpm(), 8, det=det, data="fingerprint", fp=fingerprint_expectation(form)))
    if not order0:
        out.append(Case("det M1024 3072x3072 fingerprint", FORM_ONE, "144 tiles x 2 ranges > CUs: deterministic mode falls back to one "
                        "range", 1024, [Prob(3072, 3072, True, True)], 8, det=True, data="fingerprint", fp=(3.0,), cus_below=288))
    return out


def _minrows_cases():
    one = lambda: [Prob(256, 256, True, False, py=1)]  # noqa: E731
    return (_three("auto M1024 256x256", FORM_ONE, "at the moved row threshold: the persistent kernel on its own", 1024, one, 0)
            + _three("auto M1023 256x256", FORM_128, "one row below the moved threshold", 1023, one, 0))


@functools.lru_cache(maxsize=None)
def cases(family="default"):
    return tuple({"default": _default_cases, "split2": _split2_cases, "split2_order0": lambda: _split2_cases(True),
                  "minrows1024": _minrows_cases}[family]())


def all_cases():
    return [(fam, c) for fam in FAMILY_ENV for c in cases(fam)]


def applicable(case, cus):
    return case.cus_below is None or cus < case.cus_below


# ---- data ------------------------------------------------------------------------------------------------------------------------
class Inputs(object):
    pass


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def fingerprint_sites(case):
    """(problem, rows n, columns k, first row of range 1)"""
    p = case.probs[case.fp_problem]
    nk = (case.M + 63) // 64
    r1 = 64 * ((nk + 1) // 2)
    assert case.M - r1 >= 256 and r1 >= 3
    return case.fp_problem, sorted({3, 130, p.N - 2}), sorted({5, 200, p.K - 7}), r1


@functools.lru_cache(maxsize=24)
def inputs(case):
    """dy [M, N], x [M, K] bf16; dw0 [N, K], db0 [N] fp32 (None unless the problem accumulates), all on the CPU."""
    g = torch.Generator().manual_seed(_seed(case.name))
    I = Inputs()
    I.M, I.dy, I.x, I.dw0, I.db0 = case.M, [], [], [], []
    M = case.M

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int32)

    for p in case.probs:
        if case.data == "random":
            # mean 0.5: y grows like M / 4 and keeps clear of zero, where the bound would be vacuous
            dy = (0.5 + torch.randn(M, p.N, generator=g)).to(torch.bfloat16)
            x = (0.5 + torch.randn(M, p.K, generator=g)).to(torch.bfloat16)
            dw0, db0 = 4.0 * torch.randn(p.N, p.K, generator=g), 4.0 * torch.randn(p.N, generator=g)
        else:
            if case.data == "census":
                m = torch.arange(M)
                dy = torch.zeros(M, p.N, dtype=torch.bfloat16)
                dy[m, m % p.N] = 1.0
                x = torch.zeros(M, p.K, dtype=torch.bfloat16)
                x[m, (m // p.N) % p.K] = 1.0
            else:
                dy, x = ints(-2, 2, M, p.N).to(torch.bfloat16), ints(-4, 4, M, p.K).to(torch.bfloat16)
            dw0, db0 = ints(-16, 16, p.N, p.K).float(), ints(-16, 16, p.N).float()
        I.dy.append(dy)
        I.x.append(x)
        I.dw0.append(dw0 if p.acc else None)
        I.db0.append(db0 if (p.acc and p.db) else None)
    if case.data == "fingerprint":
        i, ns, ks, r1 = fingerprint_sites(case)
        a, b = torch.zeros(M), torch.zeros(M)
        a[:3], b[:3] = 1.0, 1.0
        a[r1:r1 + 256], b[r1:r1 + 256] = -256.0, 256.0
        for n in ns:
            I.dy[i][:, n] = a.to(torch.bfloat16)
        for k in ks:
            I.x[i][:, k] = b.to(torch.bfloat16)
        for n in ns:
            for k in ks:
                I.dw0[i][n, k] = FP_DW0
    return I


def integer_partial_sum_cap(case):
    """An upper bound, computed from the case's own data, on |any partial sum in any order and any split| over all elements of dW
    and db (the fingerprint's own elements left out: they reach 2^24 by construction): max_n sum_m |dy_mn| max_k |x_mk| + |dW0|."""
    I = inputs(case)
    top = 0.0
    for i, p in enumerate(case.probs):
        dy, x = I.dy[i].to(F64).abs(), I.x[i].to(F64).abs()
        dw0 = I.dw0[i].to(F64).abs() if p.acc else torch.zeros(p.N, p.K, dtype=F64)
        if case.data == "fingerprint" and i == case.fp_problem:
            _, ns, ks, _ = fingerprint_sites(case)
            keep_n = torch.ones(p.N, dtype=torch.bool)
            keep_n[ns] = False
            keep_k = torch.ones(p.K, dtype=torch.bool)
            keep_k[ks] = False
            # rows n of the construction against the other columns, the other rows against every column
            cap_f = (dy[:, ns] * x[:, keep_k].max(dim=1, keepdim=True)[0]).sum(0).max() + dw0[ns][:, keep_k].max()
            cap_o = (dy[:, keep_n] * x.max(dim=1, keepdim=True)[0]).sum(0).max() + dw0[keep_n].max()
            top = max(top, float(cap_f), float(cap_o))
        else:
            top = max(top, float((dy * x.max(dim=1, keepdim=True)[0]).sum(0).max() + dw0.max()))
        if p.db:
            top = max(top, float(dy.sum(0).max()) + 16.0)
    return top


# ---- physical buffers ---------------------------------------------------------------------------------------------------------------
def operand(logical, ld):
    """[PRE + M + POST, ld] bf16 of NaN with `logical` at rows PRE .. PRE + M - 1, columns 0 .. n - 1."""
    M, n = logical.shape
    buf = torch.full((PRE + M + POST, ld), float("nan"), dtype=torch.bfloat16)
    buf[PRE:PRE + M, :n] = logical
    return buf


def initial(case, i):
    """(dW buffer [DW_PRE + N + DW_POST, ldw], db buffer [DB_PRE + N + DB_POST] or None) as they stand before the launch."""
    p, I = case.probs[i], inputs(case)
    dw = torch.full((DW_PRE + p.N + DW_POST, p.ldw), SENTINEL, dtype=torch.float32)
    dw[DW_PRE:DW_PRE + p.N, :p.K] = I.dw0[i] if p.acc else float("nan")
    db = None
    if p.db:
        db = torch.full((DB_PRE + p.N + DB_POST,), SENTINEL, dtype=torch.float32)
        db[DB_PRE:DB_PRE + p.N] = I.db0[i] if p.acc else float("nan")
    return dw, db


def windows(p, dw, db):
    return dw[DW_PRE:DW_PRE + p.N, :p.K], (None if db is None else db[DB_PRE:DB_PRE + p.N])


def _same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def padding_intact(p, dw, db, dw_init, db_init):
    """Every element outside the dW / db windows holds the bits it held before the launch."""
    m = torch.ones_like(dw, dtype=torch.bool)
    m[DW_PRE:DW_PRE + p.N, :p.K] = False
    ok_w = _same_bits(dw[m], dw_init[m])
    ok_b = True
    if db is not None:
        mb = torch.ones_like(db, dtype=torch.bool)
        mb[DB_PRE:DB_PRE + p.N] = False
        ok_b = _same_bits(db[mb], db_init[mb])
    return ok_w, ok_b


# ---- reference and bound ----------------------------------------------------------------------------------------------------------
class Ref(object):
    def __init__(self, y, bound):
        self.y, self.bound = y, bound


def bound_of(y, A, M):
    return E32 * y.abs() + (1.0 + E32) * (M + 8) * 2.0 ** -23 * A


@functools.lru_cache(maxsize=4)
def _reference_cpu(case):
    return _reference(case, None)


def reference(case, dev=None):
    """[(Ref dW, Ref db or None)] per problem.  dev: where the float64 products of a case of more than 2^31 multiply-adds are formed."""
    if case.big:
        assert dev is not None, "%s: more than 2^31 multiply-adds, the float64 products are formed on the device" % case
        return _reference(case, dev)
    return _reference_cpu(case)


def _reference(case, dev):
    I, out = inputs(case), []
    for i, p in enumerate(case.probs):
        if dev is None:
            dy, x = I.dy[i].to(F64), I.x[i].to(F64)
            s = dy.t() @ x
            A = None if case.exact else dy.abs().t() @ x.abs()
        else:
            dy, x = I.dy[i].to(dev).to(F64), I.x[i].to(dev).to(F64)
            s = torch.matmul(dy.t(), x).cpu()
            A = None if case.exact else torch.matmul(dy.abs().t(), x.abs()).cpu()
            dy, x = dy.cpu(), None
        y = s + I.dw0[i].to(F64) if p.acc else s
        bw = torch.zeros_like(y) if case.exact else bound_of(y, A + (I.dw0[i].to(F64).abs() if p.acc else 0.0), I.M)
        rb = None
        if p.db:
            sb = dy.sum(0)
            yb = sb + I.db0[i].to(F64) if p.acc else sb
            Ab = dy.abs().sum(0) + (I.db0[i].to(F64).abs() if p.acc else 0.0)
            rb = Ref(yb, torch.zeros_like(yb) if case.exact else bound_of(yb, Ab, I.M))
        out.append((Ref(y, bw), rb))
    return out


def _ratio(got, ref, skip=None):
    err = (got - ref.y).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / ref.bound)     # (x / 0 = inf: an exact element that differs)
    if skip is not None:
        r = torch.where(skip, torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


def judge(case, outs, dev=None):
    """{check: measured / bound} of the physical output buffers [(dW buffer, db buffer or None)] of `case`; every value must lie in
    [0, 1].  Bound 0 (exact constructions, padding, the fingerprint's set) makes any difference an infinite ratio."""
    ref = reference(case, dev)
    rs = {}
    for i, p in enumerate(case.probs):
        dw, db = outs[i][0].detach().cpu(), (None if outs[i][1] is None else outs[i][1].detach().cpu())
        dw0, db0 = initial(case, i)
        ok_w, ok_b = padding_intact(p, dw, db, dw0, db0)
        gw, gb = windows(p, dw, db)
        tag = "p%d " % i
        rs[tag + "dW padding"] = 0.0 if ok_w else INF
        skip = None
        if case.data == "fingerprint" and i == case.fp_problem:
            _, ns, ks, _ = fingerprint_sites(case)
            skip = torch.zeros(p.N, p.K, dtype=torch.bool)
            vals = gw[ns][:, ks]
            skip[torch.tensor(ns)[:, None], torch.tensor(ks)[None, :]] = True
            ok = all(float(v) in case.fp for v in vals.reshape(-1))
            rs[tag + "fingerprint in {%s}" % ", ".join("%g" % v for v in case.fp)] = 0.0 if ok else INF
        rs[tag + "dW err/bound"] = _ratio(gw.to(F64), ref[i][0], skip) if bool(torch.isfinite(gw).all()) else INF
        if p.db:
            rs[tag + "db padding"] = 0.0 if ok_b else INF
            rs[tag + "db err/bound"] = _ratio(gb.to(F64), ref[i][1]) if bool(torch.isfinite(gb).all()) else INF
    return rs


def fingerprint_values(case, outs):
    i, ns, ks, _ = fingerprint_sites(case)
    gw, _ = windows(case.probs[i], outs[i][0].detach().cpu(), None)
    return sorted({float(v) for v in gw[ns][:, ks].reshape(-1)})


def passes(rs):
    return all(abs(r) <= 1.0 and r == r for r in rs.values())


def census_report(case, outs, dev=None, limit=12):
    """The token rows a row-census result misses or holds twice, per problem, as text."""
    ref, lines = reference(case, dev), []
    for i, p in enumerate(case.probs):
        gw, _ = windows(p, outs[i][0].detach().cpu(), None)
        d = torch.nan_to_num(gw.to(F64), nan=-1e9) - ref[i][0].y
        for what, sel in (("missing", d < 0), ("duplicated", d > 0)):
            idx = sel.nonzero()
            if not len(idx):
                continue
            m = torch.arange(case.M)
            rows = []
            for n, k in idx[:limit].tolist():
                rows += m[(m % p.N == n) & ((m // p.N) % p.K == k)].tolist() or ["(no row: dW[%d, %d])" % (n, k)]
            lines.append("p%d: %d element(s) %s, token rows %s%s" % (i, len(idx), what, rows[:2 * limit], " ..." if len(idx) > limit else ""))
    return "; ".join(lines)


def assert_ratios(case, rs, outs=None, dev=None, prefix=""):
    """Every ratio through helpers.check_close (recorded, asserted against 1) -> the messages of those that failed, so that a caller can
    walk all its cases before it fails.  A failed row census adds the rows it names."""
    from helpers import check_close

    failed = []
    for key in sorted(rs):
        try:
            check_close("wgrad conformance %s%s: %s" % (prefix, case.name, key), abs(rs[key]), 0.0, 1.0)
        except AssertionError as e:
            failed.append(str(e))
    if failed and case.data == "census" and outs is not None:
        failed.append("%s row census: %s" % (case.name, census_report(case, outs, dev)))
    return failed


# ---- the model of the documented arithmetic, and its mutants ---------------------------------------------------------------------
ROW_MUTANTS = ("last_row_dropped", "last_64_row_block_dropped", "first_block_of_range_1_dropped", "range_boundary_block_added_twice",
               "row_M_of_the_buffer_read")
OPERAND_MUTANTS = ("x_padding_column_leaks_into_k_below_K", "previous_problems_leading_dimension")
OUTPUT_MUTANTS = ("n_tail_row_written", "k_tail_elements_skipped", "db_summed_by_every_k_tile", "db_not_accumulated",
                  "accumulate_ignores_dw0", "overwrite_adds_dw0", "zeroing_pass_clears_an_accumulating_problem", "tile_written_transposed")
ARITHMETIC_MUTANTS = ("products_rounded_to_bf16", "bf16_running_sum_per_64_rows")
ORDER_MUTANTS = ("ranges_added_in_the_opposite_order",)
MUTANTS = ROW_MUTANTS + OPERAND_MUTANTS + OUTPUT_MUTANTS + ARITHMETIC_MUTANTS + ORDER_MUTANTS


def mutant_applies(mutant, case, d=None):
    d = d or case_dispatch(case)
    nk = (case.M + 63) // 64
    ps = case.probs
    if mutant in ("first_block_of_range_1_dropped", "range_boundary_block_added_twice"):
        return nk >= 2
    if mutant == "x_padding_column_leaks_into_k_below_K":
        return any(p.ldx > p.K for p in ps)
    if mutant == "previous_problems_leading_dimension":
        return any(ps[i].ldx != ps[i - 1].ldx for i in range(1, len(ps)))
    if mutant == "k_tail_elements_skipped":
        return any(p.K % 8 for p in ps)
    if mutant == "db_summed_by_every_k_tile":
        return any(p.db and p.K > (128 if d["form"] in (FORM_128, FORM_256) else 256) for p in ps)
    if mutant == "db_not_accumulated":
        return any(p.db and p.acc for p in ps)
    if mutant == "accumulate_ignores_dw0":
        return any(p.acc for p in ps)
    if mutant == "overwrite_adds_dw0":
        return any(not p.acc for p in ps)
    if mutant == "zeroing_pass_clears_an_accumulating_problem":
        return any(p.acc for p in ps) and any(not p.acc for p in ps)
    if mutant == "tile_written_transposed":
        return any(min(p.N, p.K) > 1 for p in ps)
    if mutant == "products_rounded_to_bf16":
        return case.madds <= (1 << 22)
    if mutant == "ranges_added_in_the_opposite_order":
        return d["nsplit"] > 1
    return True


def _ranges(M, d):
    """Physical row indices (PRE + m) of the launch's row ranges: the persistent kernel's `share` blocks of 64 rows each; one range
    for the one-tile kernels."""
    rows = PRE + torch.arange(M)
    if d["nsplit"] == 1:
        return [rows]
    step = 64 * d["share"]
    return [rows[j * step:(j + 1) * step] for j in range(d["nsplit"]) if j * step < M]


def _partial(dyb, xb, rows, p, mutant):
    """fp32(sum over `rows` of dy^T x) and fp32(column sums of dy): float64 inside, rounded once."""
    dy, x = dyb[rows][:, :p.N], xb[rows][:, :p.K]
    if mutant == "x_padding_column_leaks_into_k_below_K" and p.ldx > p.K:
        x = x.clone()
        x[:, p.K - 1] = xb[rows, p.K]
    if mutant == "products_rounded_to_bf16":
        s = torch.zeros(p.N, p.K, dtype=F64)
        step = max(1, (1 << 21) // (p.N * p.K))
        for j in range(0, len(rows), step):
            s += bf16r(dy[j:j + step, :, None] * x[j:j + step, None, :]).sum(0)
    elif mutant == "bf16_running_sum_per_64_rows":
        s = torch.zeros(p.N, p.K, dtype=F64)
        for j in range(0, len(rows), 64):
            s = bf16r(s + dy[j:j + 64].t() @ x[j:j + 64])
    else:
        s = dy.t() @ x
    return f32r(s), f32r(dy.sum(0))


def model(case, mutant=None, cus=HOST_CUS, env=None):
    """The documented arithmetic on the physical buffers, in float64 with the roundings the interface states: each row range's sum
    rounded once to fp32, the ranges and dW0 added in fp32 in the form's documented order (one chain: dW0 + sum; turns and atomics:
    ((dW0 + range 0) + range 1) ...; the ticket order is modelled by its in-order member).  -> [(dW buffer, db buffer)]."""
    I, d = inputs(case), case_dispatch(case, env, cus)
    M, outs = case.M, []
    for i, p in enumerate(case.probs):
        dw, db = initial(case, i)
        dyb, xb = operand(I.dy[i], p.ldy).to(F64), operand(I.x[i], p.ldx).to(F64)
        if mutant == "previous_problems_leading_dimension" and i > 0 and case.probs[i - 1].ldx != p.ldx:
            ld, flat = case.probs[i - 1].ldx, torch.cat([xb.reshape(-1), torch.full((1,), float("nan"), dtype=F64)])
            idx = (PRE * p.ldx + torch.arange(M + POST)[:, None] * ld + torch.arange(p.ldx)[None, :]).clamp(max=flat.numel() - 1)
            xb = torch.cat([xb[:PRE], flat[idx]])
        rng = _ranges(M, d)
        s1 = PRE + 64 * (((M + 63) // 64 + 1) // 2)           # the first row of "range 1"
        if mutant == "last_row_dropped":
            rng[-1] = rng[-1][:-1]
        elif mutant == "last_64_row_block_dropped":
            rng = [r[r < PRE + (M - 1) // 64 * 64] for r in rng]
        elif mutant == "first_block_of_range_1_dropped" and M > s1 - PRE:
            rng = [r[(r < s1) | (r >= s1 + 64)] for r in rng]
        elif mutant == "range_boundary_block_added_twice" and M > s1 - PRE:
            rng[-1] = torch.cat([rng[-1], torch.arange(s1 - 64, s1)])
        elif mutant == "row_M_of_the_buffer_read":
            rng[-1] = torch.cat([rng[-1], torch.tensor([PRE + M])])
        parts = [_partial(dyb, xb, r, p, mutant) for r in rng]
        if mutant == "ranges_added_in_the_opposite_order":
            parts = parts[::-1]
        ww, wb = windows(p, dw, db)
        add_w0 = (p.acc and mutant != "accumulate_ignores_dw0") or (not p.acc and mutant == "overwrite_adds_dw0")
        add_b0 = add_w0 and not (p.acc and mutant == "db_not_accumulated")
        if mutant == "zeroing_pass_clears_an_accumulating_problem" and p.acc and any(not q.acc for q in case.probs):
            add_w0 = add_b0 = False
        tw = ww.to(F64).clone() if add_w0 else torch.zeros(p.N, p.K, dtype=F64)
        tb = wb.to(F64).clone() if (p.db and add_b0) else torch.zeros(p.N, dtype=F64)
        if d["nsplit"] == 1:
            tw, tb = f32r(tw + parts[0][0]), f32r(tb + parts[0][1])
        else:
            for sw, sb in parts:
                tw, tb = f32r(tw + sw), f32r(tb + sb)
        if mutant == "db_summed_by_every_k_tile":
            tile = 128 if d["form"] in (FORM_128, FORM_256) else 256
            tb = tb + (tb - (wb.to(F64) if (p.db and add_b0) else 0.0)) * ((p.K + tile - 1) // tile - 1)
        if mutant == "tile_written_transposed":
            b = min(p.N, p.K, 128)
            tw[:b, :b] = tw[:b, :b].t().clone()
        if mutant == "k_tail_elements_skipped" and p.K % 8:
            tw[:, p.K - 4:] = ww[:, p.K - 4:].to(F64)
        ww.copy_(tw.to(torch.float32))
        if p.db:
            wb.copy_(tb.to(torch.float32))
        if mutant == "n_tail_row_written":
            dw[DW_PRE + p.N, :p.K] = 0.0
        outs.append((dw, db))
    return outs


# ---- fp32 emulation in three summation orders ----------------------------------------------------------------------------------
ORDERS = ("sequential", "reversed", "blocks in ranges")
EMU_SAMPLE = 40


def sample_sites(p):
    """Up to EMU_SAMPLE rows n and columns k, the edges included: elements are independent, so the emulation of a sample is the
    emulation of those elements."""
    ns = np.unique(np.linspace(0, p.N - 1, min(p.N, EMU_SAMPLE)).round().astype(np.int64))
    ks = np.unique(np.linspace(0, p.K - 1, min(p.K, EMU_SAMPLE)).round().astype(np.int64))
    return ns, ks


def emulation(case, order, nsplit=2):
    """[(ns, ks, dW[ns][:, ks] float32, db[ns] float32 or None)]: float32 arithmetic throughout, one add at a time."""
    I, out = inputs(case), []
    M = case.M
    for i, p in enumerate(case.probs):
        ns, ks = sample_sites(p)
        dy, x = I.dy[i].float().numpy()[:, ns], I.x[i].float().numpy()[:, ks]
        w0 = I.dw0[i].numpy()[np.ix_(ns, ks)].astype(np.float32) if p.acc else np.zeros((len(ns), len(ks)), np.float32)
        b0 = I.db0[i].numpy()[ns].astype(np.float32) if (p.acc and p.db) else np.zeros(len(ns), np.float32)
        if order in ("sequential", "reversed"):
            aw, ab = np.zeros_like(w0), np.zeros_like(b0)
            for m in (range(M) if order == "sequential" else range(M - 1, -1, -1)):
                aw += dy[m][:, None] * x[m][None, :]
                ab += dy[m]
            tw, tb = w0 + aw, b0 + ab
        else:
            nk = (M + 63) // 64
            share = (nk + nsplit - 1) // nsplit
            tw, tb = w0.copy(), b0.copy()
            for j in range(nsplit):
                aw, ab = np.zeros_like(w0), np.zeros_like(b0)
                for r in range(64 * share * j, min(M, 64 * share * (j + 1)), 32):
                    bw, bb = np.zeros_like(w0), np.zeros_like(b0)
                    for m in range(r, min(M, r + 32, 64 * share * (j + 1))):
                        bw += dy[m][:, None] * x[m][None, :]
                        bb += dy[m]
                    aw += bw
                    ab += bb
                tw, tb = tw + aw, tb + ab
        assert tw.dtype == np.float32 and tb.dtype == np.float32
        out.append((ns, ks, tw, tb if p.db else None))
    return out


def fingerprint_arithmetic():
    """((dW0 + r0) + r1, (dW0 + r1) + r0, dW0 + (r0 + r1)) in float32, r0 and r1 summed row by row as the construction places them."""
    f = np.float32
    r0 = f(0)
    for _ in range(3):
        r0 = f(r0 + f(1) * f(1))
    r1 = f(0)
    for _ in range(256):
        r1 = f(r1 + f(-256) * f(256))
    w0 = f(FP_DW0)
    return float(f(f(w0 + r0) + r1)), float(f(f(w0 + r1) + r0)), float(f(w0 + f(r0 + r1)))


# ---- running a case on the device ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def launch_state(hook, det):
    """The tuning hook and the deterministic switch for the launches inside; both restored whatever happens."""
    from visitron_amd import ops

    was = ops.is_deterministic()
    try:
        ops.set_wgrad_kernel(hook)
        ops.set_deterministic(det)
        yield
    finally:
        ops.set_wgrad_kernel(0)
        ops.set_deterministic(was)


def device_problems(case, dev):
    """(the list ops.wgrad takes, [(dW buffer, db buffer)]) of `case` on `dev`; the operand buffers stay alive through the views."""
    I, problems, bufs = inputs(case), [], []
    for i, p in enumerate(case.probs):
        dyb, xb = operand(I.dy[i], p.ldy).to(dev), operand(I.x[i], p.ldx).to(dev)
        dw, db = initial(case, i)
        dw, db = dw.to(dev), (None if db is None else db.to(dev))
        vw, vb = windows(p, dw, db)
        problems.append(dict(dy=dyb[PRE:PRE + case.M, :p.N], x=xb[PRE:PRE + case.M, :p.K], dw=vw, db=vb, accumulate=p.acc))
        assert problems[-1]["dy"].data_ptr() % 16 == 0 and problems[-1]["x"].data_ptr() % 16 == 0 and vw.data_ptr() % 16 == 0
        bufs.append((dw, db))
    return problems, bufs


def run(case, dev):
    """One launch of `case` through visitron_amd.ops.wgrad -> [(dW buffer, db buffer or None)] on the CPU."""
    from visitron_amd import ops

    problems, bufs = device_problems(case, dev)
    with launch_state(case.hook, case.det):
        ops.wgrad(problems, case.M)
        torch.cuda.synchronize(dev)
    return [(dw.cpu(), None if db is None else db.cpu()) for dw, db in bufs]


def run_and_judge(case, dev, env, prefix=""):
    """The gate's step for one case: the rule must name the case's form on this device, then run, judge, record.  -> (ratios, failures)"""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    reached = case_dispatch(case, env, cus)["form"]
    assert reached == case.reaches, "%s runs %s on %d CUs, not %s" % (case, reached, cus, case.reaches)
    outs = run(case, dev)
    rs = judge(case, outs, dev)
    return rs, assert_ratios(case, rs, outs, dev, prefix)


# ---- launches back to back ------------------------------------------------------------------------------------------------------
def sequence_cases(family):
    """20 launches for one stream, each with its own dW and integer data.  Slots go round-robin over W8_SEM_SLOTS = 8, so launch
    j + 8 lands on launch j's slot: the two main forms of the process alternate ON EACH SLOT (parent: turn form, fp32-atomic form,
    turn form again -- the atomic form's zeroing kernel rewrites the slot's turn words, the turn form must leave them at zero;
    VT_WGRAD_SPLIT=2 child: ticket order, deterministic order, ticket order), with the one-range form at every eighth launch.
    The parent's turn form needs 86 .. 128 tiles and more than 76 row blocks: 90 tiles at M = 4 870 (ranges of 39 and 38 blocks, 6
    rows in the last)."""
    out = []
    for j in range(20):
        acc = j % 2 == 1
        if family == "default":
            kinds = [("turns", FORM_TICKET, 4870, False), ("atomic", FORM_ATOMIC, 2048, False), ("one range", FORM_ONE, 1024, False)]
        else:
            kinds = [("ticket", FORM_TICKET, 1030, False), ("det", FORM_DET, 1100, True), ("one range", FORM_ONE, 900, False)]
        tag, form, M, det = kinds[2 if j % 8 == 5 else (j % 8 + j // 8) % 2]
        if tag == "turns":
            probs = [Prob(1536, 2560, True, acc), Prob(768, 2560, j % 4 != 3, False)]
        elif j % 5:
            probs = [Prob(256, 256, True, acc, pw=j % 2), Prob(512, 256, j % 4 != 3, False, py=1)]
        else:
            probs = [Prob(512, 512, True, acc)]
        out.append(Case("sequence %d %s M%d" % (j, tag, M), form, "launch %d of 20 without a synchronisation" % j, M, probs, 8, det=det,
                        data="exact"))
    return out


def two_stream_cases():
    """The turn form on two streams at once, two launches each (ticket order and deterministic order), each on a slot of its own."""
    return [Case("two streams %d %s" % (j, "det" if j & 2 else "ticket"), FORM_DET if j & 2 else FORM_TICKET,
                 "two launches in flight: their turn words live in different slots", 1030 + 70 * (j & 1),
                 [Prob(512, 512, True, j % 2 == 1, pw=1), Prob(256, 768, True, False, py=1)], 8, det=bool(j & 2), data="exact")
            for j in range(4)]


def run_sequence(seq, dev, env, streams=1):
    """Launch every case of `seq` without a synchronisation (round-robin over `streams` streams), synchronise once, judge all.
    -> {check: ratio} with the case names inside the keys."""
    from visitron_amd import ops

    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for c in seq:
        reached = case_dispatch(c, env, cus)["form"]
        assert reached == c.reaches, "%s runs %s on %d CUs, not %s" % (c, reached, cus, c.reaches)
    built = [device_problems(c, dev) for c in seq]
    torch.cuda.synchronize(dev)
    ss = [torch.cuda.Stream(dev) for _ in range(streams)] if streams > 1 else [torch.cuda.current_stream(dev)]
    for j, c in enumerate(seq):
        with launch_state(c.hook, c.det), torch.cuda.stream(ss[j % len(ss)]):
            ops.wgrad(built[j][0], c.M)
    torch.cuda.synchronize(dev)
    rs = {}
    for c, (_, bufs) in zip(seq, built):
        outs = [(dw.cpu(), None if db is None else db.cpu()) for dw, db in bufs]
        for k, v in judge(c, outs, dev).items():
            rs["%s: %s" % (c.name, k)] = v
    rs["turn timeouts"] = 0.0 if ops.wgrad_turn_timeouts() == 0 else INF
    return rs
