"""tests/helpers_rollout.py judged on the CPU: the bounds accept the minimal implementation (float64, every output rounded once) and
float32 emulations of every operation in four summation orders (sequential, reverse, pairwise and the kernels' own: lane-strided
partial sums, the 64-lane butterfly, wave partials / K quarters, key parts and chunks) with the fast exponential and reciprocal
pushed one ulp either way; the vacuity cap holds for every case and named elements stay within their limits; every entry of the
mutant table is rejected by a named case; and the case table reaches every branch of the kernels.  No GPU."""
import collections

import pytest
import torch

import helpers_rollout as hr

OPS = ("lstm", "lstm_bwd", "softdot", "skinny")


def _emulated(case):
    """every case is judged against the model; the emulations (eight float32 runs each) on the cases small enough to keep this file
    to seconds -- every path, kind and mask among them"""
    if case.op == "softdot":
        return case.D * case.L <= 21000
    if case.op == "skinny":
        return case.K0 + case.K1 <= 300 and case.M * case.N >= 256 or case.kind != "normal"
    return case.B in (17, 33) and case.hs == 128


def test_case_names_are_unique_and_the_table_reaches_every_branch():
    names = [c.name for c in hr.all_cases()]
    assert len(names) == len(set(names)), [n for n, k in collections.Counter(names).items() if k > 1]
    sd = hr.cases("softdot")
    by_path = collections.defaultdict(set)
    parts = set()
    for c in sd:
        I = hr.softdot_inputs(c)
        assert hr.softdot_expected_path(c, I) == c.path, c
        by_path[c.path].add((c.D, c.L))
        parts.add(hr.sd_parts((c.D + 3) // 4 if c.path != "element" else c.D, c.L))
        if c.pad:
            assert I.rs > c.D and I.bs > c.L * I.rs
        assert bool(torch.isnan(I.buf).sum() >= 8)
    assert {(D, L) for D in (4, 512, 1024, 2052, 4096) for L in (1, 7, 16, 17)} | {(512, 80), (4, 1030)} <= by_path["vec"]
    assert {(D, L) for D in (2, 6, 130, 2058) for L in (1, 7, 17)} <= by_path["vec2"]
    assert {(D, L) for D in (1, 3, 129, 1025, 2055, 512, 130) for L in (1, 7, 17)} <= by_path["element"]
    assert {1, 4, 7, 8} <= parts                                           # D = 4: 8 parts; D = 1024: 4; D = 2052 / 1025: 1
    assert hr.sd_parts(1, 17) == 8 and hr.sd_parts(256, 17) == 4 and hr.sd_parts(513, 17) == 1 and hr.sd_parts(1025, 17) == 1
    for path, D in (("vec", 512), ("vec2", 130), ("element", 129)):
        assert {c.mask for c in sd if c.path == path and c.D == D and c.L == 17} == set(hr.MASKS)
    assert {c.L for c in sd if (True, "da") in c.bwd} >= set(hr.BWD_L) and {1028, 2058} <= {c.D for c in sd if c.L == 40}
    assert any(c.kind == "peaked" for c in sd)
    sk = hr.cases("skinny")
    assert {(c.K0, c.K1, c.Kpad) for c in sk} == set(hr.SK_K) | {(2058, 512, 2592)}
    assert sum(c.K0 == 2058 for c in sk) == 1
    assert {c.M for c in sk} == set(hr.SK_M) and {c.N for c in sk} == set(hr.SK_N) and {c.form for c in sk} == set(hr.SK_FORMS)
    assert {(c.bias, c.tanh) for c in sk} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c.kind for c in sk} == {"normal", "saturated", "tiny"}
    for c in sk:
        I = hr.skinny_inputs(c)
        grid = not ((c.K0 | c.K1 | I.x0.stride(0) | (I.x1.stride(0) if c.K1 else 0)) & 3) and I.x0.storage_offset() % 4 == 0 and (
            not c.K1 or I.x1.storage_offset() % 4 == 0)
        assert grid == hr.skinny_is_grid(c), c
        assert bool((I.wbuf[:, c.K0 + c.K1:] == 0).all())
    ls = hr.cases("lstm")
    assert {c.B for c in ls} == set(hr.LSTM_B) and {c.hs for c in ls} == {128, 256} and {c.scale for c in ls} == set(hr.LSTM_SCALES)
    assert {c.ragged for c in ls if c.B == 17} == {True, False}
    lb = hr.cases("lstm_bwd")
    assert {c.B for c in lb} == set(hr.LSTM_B) and {c.hs for c in lb} == {128, 256}
    assert {c.tn for c in lb} == {"inside", "outside", "none"} and {c.opt for c in lb} == {"all", "no_d_out", "no_dh_final", "dc_zero", "no_lens"}


@pytest.mark.parametrize("op", OPS)
def test_model_and_emulations_are_accepted(op):
    worst = collections.defaultdict(float)
    for case in hr.cases(op):
        for sub in hr.subs(case):
            outs, _ = hr.case_terms(case, sub)
            rs = hr.judge(outs, hr.model(case, sub))
            # one rounding of the output: e |y| of a bound that holds several e |y| everywhere; a bf16 output may use its u |y| up
            assert all(v <= (1.0 if k.startswith("dg16") else 0.5) for k, v in rs.items()), (case, sub, rs)
            if not _emulated(case):
                continue
            for order in hr.ORDERS:
                for k in (-1, 1):
                    rs = hr.judge(outs, hr.emulation(case, order, k, sub))
                    assert hr.passes(rs), (case, sub, order, k, rs)
                    for name, v in rs.items():
                        worst[name] = max(worst[name], v)
    print("ROLLOUT-HOST %s: emulation / bound: %s" % (op, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert worst


@pytest.mark.parametrize("op", OPS)
def test_bound_is_not_vacuous_and_named_elements_stay_within_their_limits(op):
    top = 0.0
    for case in hr.cases(op):
        v = hr.vacuity(case)
        top = max(top, v)
        assert v <= 1.0, (case, v)
        for sub in hr.subs(case):
            outs, V = hr.case_terms(case, sub)
            for name, O in outs.items():
                assert bool(torch.isfinite(O.bound[torch.isfinite(O.y)]).all()), (case, name)
                nan_rows = torch.isnan(O.y).reshape(O.y.shape[0], -1).any(1)
                assert int(nan_rows.sum()) <= 1, (case, name)                                   # one all-masked batch row at most
                named = O.named & torch.isfinite(O.y)
                if not bool(named.any()):
                    continue
                assert case.kind in ("peaked", "tiny"), (case, name)
                if case.kind == "peaked":
                    small = (V["p"] < hr.FLOOR) & ~V["mk"]
                    assert int(small.sum(1).max()) * 2 <= case.L, case
                    assert bool((named.reshape(small.shape + (-1,)).any(-1) <= small).all()), (case, name)
        if case.kind == "peaked":
            assert bool(((hr.case_terms(case)[1]["p"] < hr.FLOOR) & ~hr.case_terms(case)[1]["mk"]).any()), case
        if case.kind == "tiny":
            assert any(bool(O.named.any()) for O in hr.case_terms(case)[0].values()), case
    print("ROLLOUT-HOST %s: largest bound / cap %.3f" % (op, top))


def test_every_mutant_is_rejected_by_a_named_case():
    for mutant, ops in hr.MUTANTS.items():
        seen = collections.OrderedDict()
        for op in ops:
            for case in hr.cases(op):
                if case.op == "softdot" and case.D * case.L > 40000:
                    continue
                for sub in hr.subs(case):
                    rs = hr.judge(hr.case_terms(case, sub)[0], hr.model(case, sub, mutant))
                    bad = sorted(k for k, v in rs.items() if not v <= 1.0)
                    if bad:
                        seen.setdefault(case.name, bad)
                if len(seen) >= 3:
                    break
        print("ROLLOUT-HOST mutant %s: rejected by %s" % (mutant, "; ".join("%s (%s)" % kv for kv in seen.items()) or "NOTHING"))
        assert seen, mutant
