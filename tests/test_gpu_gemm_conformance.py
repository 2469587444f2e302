"""The bf16 NT GEMM family (csrc/gemm_bf16.hip, gemm_v7*.hip/hpp) against the float64 reference and the derived per-element bounds
of tests/helpers_gemm.py, through visitron_amd.ops only: every production variant of csrc/gemm_variants.def forced in turn over
the case table, the automatic path, the tail launch, split-K, the deferred-LayerNorm epilogues and the dropout hash.  Alone:
python -m pytest tests/test_gpu_gemm_conformance.py -q -s

A combination the library would run with another variant's kernel (helpers_gemm.runnable) is not run under the forced variant's
name.  Exact constructions (small integers, dropout at p = 0.5) are compared with torch.equal; random cases go through
helpers.check_close as measured / bound against 1."""
import pytest
import torch

import helpers_gemm as hg

pytestmark = pytest.mark.gpu
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
SENTINEL = 57.0
DT = {"bf16": BF16, "f16": F16, "f32": F32}

# The parametrisation is laid out for 256 compute units (collection runs without a device); the shapes that depend on the count are
# rebuilt for the device's own at run time, in the same order.
_STATIC = hg.cases(cus=256)
_RT = {}


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _cases():
    if "cases" not in _RT:
        _RT["cases"] = hg.cases(cus=_cus())
        assert [c.name.split("_")[0] for c in _RT["cases"]] == [c.name.split("_")[0] for c in _STATIC]
    return _RT["cases"]


PAIRS = [(i, v) for i, c in enumerate(_STATIC) for v in hg.production_variants()
         if any(hg.runnable(v, c, e) for e in c.epis + c.exact)]


def _act(ops, name):
    return {"none": ops.ACT_NONE, "gelu": ops.ACT_GELU, "tanh": ops.ACT_TANH, "mul": ops.ACT_MUL}[name]


def _padded(x, ld, dtype, dev, rows=None, index=None, fill=float("nan")):
    """x [M, n] float64 -> device buffer [rows, ld] of `dtype` holding x at the rows `index`, `fill` elsewhere; (buffer, view [:, :n])."""
    M, n = x.shape
    rows = M if rows is None else rows
    buf = torch.full((rows, ld), fill, dtype=dtype)
    if index is None:
        buf[:M, :n] = x.to(dtype)
    else:
        buf[index, :n] = x.to(dtype)
    buf = buf.to(dev)
    return buf, buf[:, :n]


def _out_buffer(rows, N, ld, dtype, dev):
    buf = torch.full((rows, ld), float("nan"), dtype=dtype)
    buf[:, N:] = SENTINEL
    buf = buf.to(dev)
    return buf, buf[:, :N]


def _read_out(buf, case, what):
    """The logical rows [M, N] (float64, CPU) of an output buffer; padding columns and rows no output row maps to must be untouched."""
    got = buf.cpu()
    N = case.N
    assert bool((got[:, N:] == SENTINEL).all()), "%s: a padding column was written" % what
    idx = case.out_row_index()
    untouched = torch.ones(got.shape[0], dtype=torch.bool)
    untouched[idx] = False
    assert bool(torch.isnan(got[untouched][:, :N]).all()), "%s: a row outside the row map was written" % what
    return got[idx][:, :N].to(F64)


def run_linear(dev, case, o, e):
    """One ops.linear call of epilogue set `e` on the operands `o` -> {"out": [M, N] float64, "pre": ...}"""
    from visitron_amd import ops

    ep = hg.epi(e)
    M, N, K = case.M, case.N, case.K
    rows, idx = case.out_rows, case.out_row_index()
    _, a = _padded(o.a, case.lda, BF16, dev)
    w = o.w.to(BF16).to(dev)
    bias = o.b.to(F32).to(dev) if ep["bias"] else None
    ldr = (N + 7) // 8 * 8
    res, res_ln = None, None
    if ep["res"] == "ln":
        _, res = _padded(o.v, ldr, F16, dev)
        res_ln = tuple(t.to(F32).to(dev) for t in (o.mean, o.rstd, o.gamma, o.beta))
    elif ep["res"] is not None:
        r = o.r_mul if ep["act"] == "mul" else (o.r_bf16 if ep["res"] == "bf16" else o.r_f16)
        _, res = _padded(r, ldr, BF16 if ep["res"] == "bf16" else F16, dev, rows=rows, index=idx)
    ldc = case.ldc
    cbuf, c = _out_buffer(rows, N, ldc, DT[ep["out"]], dev)
    c2buf, c2 = _out_buffer(rows, N, ldr, BF16, dev) if ep["c2"] else (None, None)
    ops.linear(a, w, bias=bias, residual=res, act=_act(ops, ep["act"]), out=c, out_f32=ep["out"] == "f32", grp_rows=case.grp[0],
               grp_stride=case.grp[1], M=M, pre_act_out=c2, drop=o.drop if ep["drop"] else ops.NO_DROP, residual_ln=res_ln)
    torch.cuda.synchronize()
    out = {"out": _read_out(cbuf, case, "%s %s" % (case, e))}
    if ep["c2"]:
        out["pre"] = _read_out(c2buf, case, "%s %s second output" % (case, e))
    return out


_REF = {"case": None}


def _reference(case, o, e, form):
    """The float64 reference of (case, epilogue set, GELU form): computed once, shared by every variant (the cases arrive in order)."""
    if _REF["case"] != case.name:
        _REF.clear()
        _REF["case"] = case.name
    key = (e, form, o.exact)
    if key not in _REF:
        _REF[key] = hg.linear_reference(o, e, form)
    return _REF[key]


def check_case(dev, case, label, variant=None, epis=None, exact=None, twice=False):
    """Every epilogue set of `case` that `variant` runs itself (None: the automatic path): random data against the bounds, the
    exact constructions bit for bit."""
    cus = _cus()
    signed = case.M * case.N >= 100000
    ran = 0
    for kind, names in (("random", case.epis if epis is None else epis), ("exact", case.exact if exact is None else exact)):
        for e in names:
            if variant is not None and not hg.runnable(variant, case, e, cus):
                continue
            o = hg.operands(case, kind == "exact")
            form = "erf" if variant is None else hg.gelu_form(variant, case, e)
            ref = _reference(case, o, e, form)
            got = run_linear(dev, case, o, e)
            ran += 1
            if twice:
                again = run_linear(dev, case, o, e)
                assert all(torch.equal(got[k], again[k]) for k in got), "%s %s %s: two launches differ" % (label, case, e)
            for key in ref:
                if kind == "exact":
                    want = hg.round_out(ref[key].y, ref[key].fmt)
                    if not torch.equal(got[key], want):
                        bad = (got[key] != want).nonzero()
                        raise AssertionError("%s %s exact %s %s: %d elements differ, first at %s" % (
                            label, case, e, key, bad.shape[0], bad[0].tolist()))
                else:
                    hg.assert_ratios("%s %s" % (label, case), {"%s %s" % (e, k): r for k, r in
                                                               hg.ratios(ref[key], got[key], key, signed=signed).items()})
    return ran


@pytest.mark.parametrize("idx,variant", PAIRS, ids=["%s-v%d" % (_STATIC[i].name, v) for i, v in PAIRS])
def test_variant_meets_the_bounds(dev, idx, variant):
    from visitron_amd import ops

    case = _cases()[idx]
    shared = variant in ops.SHARED_TILE_VARIANTS
    ops.set_gemm_variant(variant)
    try:
        ran = check_case(dev, case, "v%d" % variant, variant=variant, twice=shared)
    finally:
        ops.set_gemm_variant(-1)
    assert ran or variant == 33, "nothing ran"      # (33 on another CU count: test_variant_33_answers_as_the_rule_predicts)
    if shared:
        assert ops.gemm_shared_tile_timeouts() == 0


def test_variant_33_answers_as_the_rule_predicts(dev):
    """launch_splitk_epi returns VT_ERR_UNSUPPORTED where it would make fewer than two copies (never another kernel, when forced)."""
    from visitron_amd import _lib, ops

    cus = _cus()
    ops.set_gemm_variant(33)
    try:
        for case in _cases():
            if case.auto or case.name.startswith("persistent") or case.grp[0]:
                continue
            o = hg.operands(case)
            want_ok = hg.splitk33_supported(case, cus)
            try:
                run_linear(dev, case, o, "plain")
                ok = True
            except RuntimeError as err:
                assert "(code %d)" % _lib.CONSTANTS["VT_ERR_UNSUPPORTED"] in str(err), err
                ok = False
            assert ok == want_ok, "%s: the library %s, the rule says %s" % (case, "ran" if ok else "refused", want_ok)
    finally:
        ops.set_gemm_variant(-1)


@pytest.mark.parametrize("variant", [28, 29, 30])
def test_shared_variants_on_tall_tiles_are_their_twins(dev, variant):
    """28 .. 30 have no kernel of their own (launch_v8): their output equals the twin's bit for bit."""
    from visitron_amd import ops

    twin = ops.GEMM_VARIANTS[variant]["twin"]
    mtn = ops.GEMM_VARIANTS[variant]["mtn"]
    case = [c for c in _cases() if c.name.startswith("mtail%d" % mtn)][0]
    o = hg.operands(case)
    outs = []
    for v in (variant, twin):
        ops.set_gemm_variant(v)
        try:
            outs.append(run_linear(dev, case, o, "drop_res")["out"])
        finally:
            ops.set_gemm_variant(-1)
    assert torch.equal(outs[0], outs[1])
    ref = hg.linear_reference(o, "drop_res")["out"]
    hg.assert_ratios("v%d (as %d) %s" % (variant, twin, case), hg.ratios(ref, outs[0], "drop_res out"))
    assert ops.gemm_shared_tile_timeouts() == 0


@pytest.mark.parametrize("name", ["200x201x128", "300x520x768", "260x392x3072"])
def test_automatic_path_meets_the_bounds(dev, name):
    """Variant -1: the shape table / heuristic.  On these shapes (N % 64 != 0) no kernel has the straight-line epilogue, so
    whichever variant the library picks runs the erf form of GELU (helpers_gemm.gelu_form)."""
    from visitron_amd import ops

    case = [c for c in _cases() if c.name == name][0]
    ops.set_gemm_variant(-1)
    assert check_case(dev, case, "auto") == len(case.epis) + len(case.exact)


def test_tail_launch_keeps_the_dropout_index(dev):
    """Automatic mode with the tail launch, the table entry forced to the persistent kernel: the rows of the last, at most half
    full round go to a second launch whose dropout seed carries the row offset (vt_gemm_dispatch).  Exact construction, p = 0.5:
    an index off by one pair in the second launch changes which elements equal the residual.  (How many launches the library
    made cannot be seen through ops: whichever it makes are held to the exact answer.)"""
    from visitron_amd import _lib, ops

    cus = _cus()
    case = [c for c in _cases() if c.auto][0]
    M, M1 = hg.tail_split_rows(cus)
    assert case.M == M
    lib = _lib.load()
    for f32 in (False, True):
        lib.vt_gemm_tune(case.M, case.N, case.K, ops.tune_kind(ops.ACT_NONE, residual=True, out_f32=f32), 16)
    lib.vt_debug_set_gemm_variant(-2)
    try:
        assert check_case(dev, case, "tail launch") == len(case.exact)
    finally:
        ops.set_gemm_variant(-1)
    o = hg.operands(case, True)
    wrong = hg.linear_model(o, "drop_res", "dropout_pair_index_off_by_one_in_second_launch", M1=M1)["out"]
    assert not torch.equal(wrong, hg.linear_model(o, "drop_res")["out"])


@pytest.mark.parametrize("name", ["640x768x768", "300x264x1024"])
def test_linear_splitk(dev, name):
    from visitron_amd import ops

    case = [c for c in _cases() if c.name == name][0]
    for exact in (True, False):
        o = hg.operands(case, exact)
        a, w = o.a.to(BF16).to(dev), o.w.to(BF16).to(dev)
        u = hg.U_OUT["bf16"]
        F = (case.K + 8) * 2.0 ** -23 * o.Pabs
        ref = hg.Ref(o.P, u * o.P.abs() + (1 + u) * F, "bf16")
        for ks in (2, 3, case.K // 64):
            out = torch.full((case.M, case.N), float("nan"), dtype=BF16, device=dev)
            ops.linear_splitk(a, w, ks, out=out)
            torch.cuda.synchronize()
            got = out.cpu().to(F64)
            if exact:
                assert torch.equal(got, hg.bf16r(o.P)), "ksplit %d" % ks
            else:
                hg.assert_ratios("splitk %s" % case, hg.ratios(ref, got, "ksplit %d out" % ks, signed=case.M * case.N >= 100000))


@pytest.mark.parametrize("drop", [(0.1, 1234, 1), (0.5, 0xDEADBEEFCAFE, 0xE0)])
def test_dropout_mask_equals_the_python_hash(dev, drop):
    from visitron_amd import ops

    got = ops.dropout_mask(1 << 16, drop, device=dev).cpu().numpy().astype(bool)
    assert (got == hg.keep_mask(1 << 16, drop)).all()


# ---- the deferred-LayerNorm epilogues --------------------------------------------------------------------------------------------
LN_PAIRS = [(v, K, N) for v in hg.production_variants() if hg.ln_runnable(v) for (K, N) in hg.LN_SHAPES]


@pytest.mark.parametrize("variant,K,N", LN_PAIRS, ids=["v%d-%dx%d" % p for p in LN_PAIRS])
def test_linear_ln_meets_the_bounds(dev, variant, K, N):
    from visitron_amd import ops

    M = 32 * ops.GEMM_VARIANTS[variant]["mtn"] * 2 + 37
    shared = variant in ops.SHARED_TILE_VARIANTS
    ops.set_gemm_variant(variant)
    try:
        for mode, acts in ((1, ("none", "gelu")), (2, ("none",))):
            o = hg.ln_operands(M, K, N, mode)
            a, w = o.a.to(BF16).to(dev), o.w.to(BF16).to(dev)
            bias, colv, stats = o.bias.to(F32).to(dev), o.colv.to(F32).to(dev), o.stats.to(dev)
            for act in acts:
                ref = hg.ln_reference(o, act)
                for rep in range(2 if shared else 1):
                    out = torch.full((M, N), float("nan"), dtype=BF16, device=dev)
                    got = {}
                    if mode == 1:
                        ops.linear_ln(a, w, bias, colv, stats, hg.LN_EPS, 1, act=_act(ops, act), out=out)
                        torch.cuda.synchronize()
                        got["out"] = out.cpu().to(F64)
                    else:
                        out_s = torch.full((M, N), float("nan"), dtype=F16, device=dev)
                        st = torch.full((N // 128, o.rows, 2), SENTINEL, dtype=F32, device=dev)
                        ops.linear_ln(a, w, bias, colv, stats, hg.LN_EPS, 2, out=out, rs=o.rs.to(F16).to(dev), out_s=out_s, stats_out=st)
                        torch.cuda.synchronize()
                        st = st.cpu().to(F64)
                        assert bool((st[:, M:] == SENTINEL).all()), "statistics rows past M were written"
                        got = {"stream": out_s.cpu().to(F64), "copy": out.cpu().to(F64), "sum": st[:, :M, 0], "sq": st[:, :M, 1]}
                    if rep:
                        assert all(torch.equal(got[k], first[k]) for k in got), "two launches differ"
                    first = got
                for key in ref:
                    hg.assert_ratios("linear_ln v%d %dx%dx%d" % (variant, M, K, N),
                                     {"mode %d %s %s" % (mode, act, k): r for k, r in
                                      hg.ratios(ref[key], got[key], key, signed=M * N >= 100000).items()})
    finally:
        ops.set_gemm_variant(-1)
    if shared:
        assert ops.gemm_shared_tile_timeouts() == 0
