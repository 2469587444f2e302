"""tests/helpers_layernorm.py judged on the CPU: the bounds accept the minimal implementation (float64, each output rounded once)
and a float32 emulation in three summation orders with a factor two to spare, reject a table of subtly wrong implementations,
never go vacuous outside the rows a case names, the exact constructions are exact in float32 in every order, the signed
statistic sees a truncating convert, and every kernel instantiation of the family is reached by a named case.  No GPU."""
import collections

import pytest
import torch

import helpers_gemm as hg
import helpers_layernorm as hl

ALL = hl.all_cases()
GROUPS = collections.OrderedDict()
for _fam, _c in ALL:
    GROUPS.setdefault((_fam, _c.kind), []).append(_c)
GROUP_IDS = ["%s-%s" % k for k in GROUPS]


def _fp32_part(ref):
    """the bound less the final rounding of the output (u |y|; e |prior + sum| of an accumulated sum)"""
    return ref.bound - ref.rounding


# ---- the model passes; the emulation has a factor two to spare; exact constructions are exact ------------------------------------
@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_model_passes_every_bound_and_the_emulation_stays_below_half(group):
    worst = collections.defaultdict(float)
    for case in GROUPS[group]:
        I, ref = hl.inputs(case), hl.reference(case)
        rs = hl.judge(case, hl.model(case))
        assert hl.passes(rs), (case, {k: v for k, v in rs.items() if not abs(v) <= 1.0})
        for order in hl.ORDERS:
            emu = hl.emulation(case, order)
            for key in ref:
                err = (emu[key] - ref[key].y).abs()
                if I.exact and float(ref[key].bound.max()) == 0.0:
                    # the fp32 value IS the float64 reference (rounded once where the output is narrower)
                    assert torch.equal(hl.round_out(emu[key], ref[key].fmt), ref[key].y), (case, order, key)
                    continue
                E = _fp32_part(ref[key])
                r = float(torch.where(err == 0, torch.zeros_like(err), err / E).max())
                assert r <= 0.5, (case, order, key, r)
                what = "statistics" if key in ("mean", "rstd") else "row sums" if key in ("dgamma", "dbeta") else "elements"
                worst[what] = max(worst[what], r)
    print("LN-HOST %s-%s: fp32 emulation / fp32 part of the bound: %s" % (
        group + (", ".join("%s %.3f" % kv for kv in sorted(worst.items())) or "exact only",)))


def test_case_names_are_unique():
    for fam in hl.FAMILY_ENV:
        names = [c.name for c in hl.cases(fam)]
        assert len(names) == len(set(names)), [n for n, k in collections.Counter(names).items() if k > 1]
    for _, case in ALL:
        assert case.why and case.reaches


# ---- the bound does not go vacuous -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_bound_is_not_vacuous_outside_the_named_rows(group):
    top = 0.0
    for case in GROUPS[group]:
        v = hl.vacuity(case)
        if v is None:
            assert case.kind == "stream_init"
            continue
        I = hl.inputs(case)
        assert len(I.degenerate) <= 8
        ok = torch.ones(I.M, dtype=torch.bool)
        ok[I.degenerate] = False
        if bool(ok.any()):
            top = max(top, float(v[ok].max()))
            assert float(v[ok].max()) <= 2.0 ** -10, (case, float(v[ok].max()))
    print("LN-HOST %s-%s: largest dmean rstd outside the named rows 2^%.1f" % (group + (torch.log2(torch.tensor(top + 1e-300)).item(),)))


def test_eps_matters_in_the_small_rows():
    """rows scaled by 0.01 under eps = 1e-5: eps is 4 .. 40 % of var + eps"""
    case = [c for c in hl.cases() if c.kind == "fwd" and c.p["eps"] == 1e-5 and c.p["M"] >= 16][0]
    I = hl.inputs(case)
    var = hl.fwd_values(I.x, I.gamma, I.beta, I.eps)[1].view(-1)
    share = I.eps / (var + I.eps)
    small = torch.arange(I.M) % 8 == 6
    assert bool(small.any()) and 0.03 <= float(share[small].min()) and float(share[small].max()) <= 0.45


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
_SEEN = collections.defaultdict(list)
ARITHMETIC_MUTANTS = tuple(m for m in hl.MUTANTS if m not in hl.STRUCTURAL_MUTANTS)
# an arithmetic mutant is judged on the cases up to this size (the larger ones repeat their widths); the structural ones are judged
# on every exact construction by the test after the next
MUTANT_MAX_ELEMENTS = 1 << 20


@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_mutants(group):
    """Every arithmetic mutant on every case of the group it applies to; which cases reject it is recorded for the test below.  A
    mutant may hide on a case (a truncation on a handful of elements, an fp32 slip below the worst-case sum of a long row): the
    counts are printed."""
    seen, hidden = collections.defaultdict(list), collections.defaultdict(list)
    for case in GROUPS[group]:
        if case.p["M"] * case.p["H"] > MUTANT_MAX_ELEMENTS:
            continue
        for mutant in ARITHMETIC_MUTANTS:
            if hl.mutant_applies(mutant, case):
                rs = hl.judge(case, hl.model(case, mutant))
                (hidden if hl.passes(rs) else seen)[mutant].append(case.name)
    for mutant in ARITHMETIC_MUTANTS:
        if seen[mutant] or hidden[mutant]:
            _SEEN[mutant] += seen[mutant]
            print("LN-HOST mutant %s on %s-%s: rejected on %d case(s), hidden on %d%s" % (
                (mutant,) + group + (len(seen[mutant]), len(hidden[mutant]),
                                     (": " + "; ".join(hidden[mutant][:3])) if hidden[mutant] else "")))


def test_zz_no_mutant_goes_unrejected():
    """(runs after test_mutants: files run in order; alone it judges what it needs itself)"""
    for mutant in ARITHMETIC_MUTANTS:
        if not _SEEN[mutant]:
            for _, case in ALL:
                if hl.mutant_applies(mutant, case) and not hl.passes(hl.judge(case, hl.model(case, mutant))):
                    _SEEN[mutant].append(case.name)
                    break
        assert _SEEN[mutant], "mutant %s is rejected nowhere" % mutant


STRUCTURAL_KINDS = {"last_chunk_columns_skipped": ("fwd", "bwd", "emb", "emb_f32", "emb_bwd", "rows_f32", "drop_f32", "bwd_f32"),
                    "tail_row_stored_into_row_M": ("fwd", "rows_f32"), "one_partial_row_dropped": ("bwd", "emb_bwd", "bwd_f32"),
                    "one_grid_stride_iteration_skipped": ("fwd", "bwd", "emb_bwd", "bwd_f32"),
                    "gap_rows_written": ("fwd", "rows_f32", "drop_f32")}


@pytest.mark.parametrize("mutant", hl.STRUCTURAL_MUTANTS)
def test_exact_constructions_reject_structural_mutants_everywhere(mutant):
    """a structural mutant is rejected on EVERY exact construction it applies to, in every kernel family that has the structure"""
    kinds = set()
    for _, case in ALL:
        if case.p["exact"] and hl.mutant_applies(mutant, case):
            assert not hl.passes(hl.judge(case, hl.model(case, mutant))), (mutant, case)
            kinds.add(case.kind)
    assert kinds == set(STRUCTURAL_KINDS[mutant]), (mutant, kinds)


# ---- the signed statistic ------------------------------------------------------------------------------------------------------------
def test_signed_statistic_accepts_the_model_and_rejects_truncation():
    signed = [c for c in hl.cases() if hl.signed_case(c)]
    narrow = lambda c: any(s.fmt in ("bf16", "f16") and s.n == c.p["H"] for s in hl.inputs(c).outs.values())
    kinds = collections.OrderedDict()
    for c in signed:                                   # per kind: the smallest case with a narrow output of width H
        if narrow(c) and (c.kind not in kinds or c.p["M"] * c.p["H"] < kinds[c.kind].p["M"] * kinds[c.kind].p["H"]):
            kinds[c.kind] = c
    assert {"fwd", "bwd", "emb", "rows_f32", "apply"} <= set(kinds), sorted(kinds)
    for case in kinds.values():
        rs = hl.judge(case, hl.model(case))
        keys = [k for k in rs if k.endswith("signed bias")]
        assert keys and all(abs(rs[k]) <= 1.0 for k in keys), (case, rs)
        rt = hl.judge(case, hl.model(case, "output_truncated"))
        assert all(abs(rt[k]) > 1.0 for k in keys), (case, {k: rt[k] for k in keys})


# ---- reachability --------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_the_instantiation_it_names():
    for fam, case in ALL:
        assert hl.case_dispatch(case, hl.FAMILY_ENV[fam])[0] == case.reaches, (fam, case)


def test_every_instantiation_is_named_by_some_case():
    reached = collections.defaultdict(list)
    for fam, case in ALL:
        reached[hl.case_dispatch(case, hl.FAMILY_ENV[fam])[0]].append((fam, case))
    missing = [k for k in hl.INSTANTIATIONS if k not in reached]
    assert not missing, missing
    assert set(reached) <= set(hl.INSTANTIATIONS), set(reached) - set(hl.INSTANTIATIONS)
    for k in hl.INSTANTIATIONS:
        if k.startswith("layernorm") or k.startswith("embed_layernorm_bwd") or k == "ln_bwd_f32":
            # both a random case and an exact construction
            assert {c.p["exact"] for _, c in reached[k]} == {False, True}, k
    # the non-default instantiations are reached only through the switches
    for k, v in reached.items():
        if k.startswith("layernorm_rows_full") and k.split(",")[2] == "1" or k.startswith("layernorm_bwd_rows_full") and k.split(",")[2] in "24":
            assert all(fam != "default" for fam, _ in v), k


def test_every_loop_feature_is_entered():
    """The cases that claim to enter a loop's second trip, the reduce's unrolled loop or the tail group do, by the dispatch rule."""
    entered = set()
    for fam, case in ALL:
        name, R, nb = hl.case_dispatch(case, hl.FAMILY_ENV[fam])
        M = case.p["M"]
        groups = (M + R - 1) // R
        for e in case.get("enters", ()):
            assert e in hl.FEATURES, e
            if e.endswith("second trip round the grid-stride loop"):
                assert groups > 4 * nb and name.startswith({"fwd full": "layernorm_rows_full", "bwd full": "layernorm_bwd_rows_full",
                                                            "bwd chunked": "layernorm_bwd_rows<", "embedding bwd": "embed_layernorm_bwd",
                                                            "ln_bwd_f32": "ln_bwd_f32"}[e.split(":")[0]]), (case, e)
            elif e == "reduce: unrolled loop":
                assert nb >= 193, (case, nb)             # `b + 192 < nblocks` holds for row group 0 from 193 partial rows on
            elif e == "reduce: unrolled loop plus a remainder":
                assert nb > 256 and nb % 256 != 0, (case, nb)   # a row group takes the unrolled trip and then single rows
            elif e == "fwd: tail group with a repeated row":
                assert M % R != 0
            entered.add(e)
    assert entered == set(hl.FEATURES), set(hl.FEATURES) - entered
    # the kernels' own thresholds: 193 partial rows at M = 769, the forward loop's second trip from M > 8192 on
    assert hl.bwd_dispatch(768, True, False)[2](769) == 193 and hl.bwd_dispatch(768, True, False)[2](768) == 192
    name, R, nb = hl.fwd_dispatch(768, 0, True)
    assert (name, R, nb(8192), nb(8195)) == ("layernorm_rows_full<1,1,2,1>", 2, 1024, 1024) and (8195 + 1) // 2 > 4 * 1024 >= 8192 // 2


def test_sum_orders_differ_and_agree_with_float64():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(7, 1000, generator=g).numpy()
    sums = [hl.sum32(a, o) for o in hl.ORDERS]
    assert all(abs(s - a.astype("float64").sum(-1)).max() < 1e-3 for s in sums)
    assert any((sums[0] != sums[1]).tolist()) and any((sums[1] != sums[2]).tolist())
    ones = torch.ones(3, 777).numpy()
    assert all((hl.sum32(ones, o) == 777.0).all() for o in hl.ORDERS)
