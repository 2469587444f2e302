"""tests/helpers_loss.py judged on the CPU: the bounds accept the minimal implementation (float64, every output rounded once) at
half the bound and float32 emulations in four summation orders (sequential, pairwise, the kernels' 256-lane shape, online
rescaled) at half the fp32 part of the bound, never go vacuous outside the elements a case names, reject a table of subtly
wrong implementations (which check rejects which is printed), the exact constructions are exact in float32 in every order, and
every kernel instantiation of the loss heads is reached by a named case.  No GPU."""
import collections

import numpy as np
import pytest
import torch

import helpers_loss as hl

HEADS = ("ce", "double", "action")
RANDOM = lambda c: c.kind not in ("onehot", "uniform")


def _groups():
    g = collections.OrderedDict()
    for c in hl.all_cases():
        g.setdefault("%s-%s" % (c.head, c.kind), []).append(c)
    return g


GROUPS = _groups()


def test_case_names_are_unique_and_the_table_holds_what_it_must():
    names = [c.name for c in hl.all_cases()]
    assert len(names) == len(set(names)), [n for n, k in collections.Counter(names).items() if k > 1]
    ce = hl.cases("ce")
    assert {1, 3, 8, 9, 97, 1023, 1024, 1025, 1601, 8192, 8193, 30522, 32768, 32770, 33001} <= {c.V for c in ce if RANDOM(c)}
    assert {c.reaches for c in ce} == {"ce_softmax_rows_reg<8>", "ce_softmax_rows_reg<32>", "ce_softmax_rows"}
    at = {c.V: c for c in ce if c.kind == "normal"}
    assert at[8192].reaches == "ce_softmax_rows_reg<8>" and at[8193].reaches == "ce_softmax_rows_reg<32>" and at[8193].Vpad == 8200
    assert at[32768].reaches == "ce_softmax_rows_reg<32>" and at[32770].reaches == "ce_softmax_rows" and at[32770].Vpad == 32776
    assert at[33001].reaches == "ce_softmax_rows" and (at[33001].Vpad, at[33001].lddz) == (33024, 33032)
    assert (at[30522].Vpad, at[30522].ldz) == (30528, 30532)
    for kind in ("onehot", "ties"):          # both exact tables in every single-softmax kernel
        assert {c.reaches for c in ce if c.kind == kind} == {c.reaches for c in ce}
    assert {c.reaches for c in ce if c.kind == "uniform"} == {"ce_softmax_rows_reg<8>", "ce_softmax_rows_reg<32>"}
    assert {c.V for c in hl.cases("double") if RANDOM(c)} >= set(hl.DOUBLE_V)
    act = [c for c in hl.cases("action") if c.kind != "ties"]
    assert {c.rows for c in act} == set(hl.ACTION_B) and {c.V for c in act} == set(hl.ACTION_A)
    assert any(c.Vpad < 64 for c in act) and any(c.Vpad == 64 and c.V < 57 for c in act) and any(c.rows > 1024 for c in act)
    for B in hl.ACTION_B:
        assert {c.p["ignored"] for c in act if c.rows == B} == {0, 1, B - 1, B}
    for c in hl.all_cases():
        I = hl.inputs(c)
        assert c.why and c.ldz > c.V and c.lddz > c.Vpad >= c.V and abs(c.scale) >= 2.0 ** -20
        assert bool((I.zbuf[:, c.V:] == hl.PAD_IN).all()) and torch.equal(I.zbuf[:, :c.V], I.z)
        lo = -1 if c.head == "action" else 0
        assert int(I.y.min()) >= lo and int(I.y.max()) < c.V            # labels are always inside the row
        if c.kind in ("normal", "confident", "bf16grid", "ties"):
            assert float(I.z.max()) < hl.PAD_IN                             # ... so a kernel that read the padding would show
        if c.kind in ("onehot", "uniform"):
            s = abs(c.scale)
            assert s == 2.0 ** round(np.log2(s))


def test_one_hot_rows_sweep_every_structural_position():
    for c in hl.cases("ce"):
        if c.kind != "onehot":
            continue
        I = hl.inputs(c)
        want = set(p for p in hl.ONEHOT_POSITIONS if p < c.V) | {c.V - 1} | set(range(c.V - c.V % 4, c.V))
        assert set(I.hot.tolist()) == want and set(I.y.tolist()) == want
        assert bool((I.hot[0::2] == I.y[0::2]).all()) and bool((I.hot[1::2] != I.y[1::2]).all())
    assert any(c.V % 4 for c in hl.cases("ce") if c.kind == "onehot" and c.two_pass)


def test_ties_straddle_vectors_lanes_waves_and_chunks():
    thread = lambda col: (col % 1024) // 4
    chunk = lambda col: col // 1024
    for c in hl.cases("ce"):
        if c.kind != "ties" or c.V < 3000:
            continue
        sets = hl.tie_sets(c)
        assert any(len(t) == 2 and t[0] // 4 == t[1] // 4 for t in sets)                                      # one 4-vector
        assert any(thread(t[0]) != thread(t[1]) and thread(t[0]) // 64 == thread(t[1]) // 64 for t in sets)   # two lanes
        assert any(thread(t[0]) // 64 != thread(t[1]) // 64 and chunk(t[0]) == chunk(t[1]) for t in sets)     # two waves
        assert any(chunk(t[0]) < chunk(t[1]) and thread(t[0]) > thread(t[1]) for t in sets)      # the lower index in the later lane
        assert any(len(t) == 3 for t in sets)
    d = hl.tie_sets([c for c in hl.cases("double") if c.kind == "ties" and c.V == 2048][0])
    assert {(7, 8), (511, 512), (2040, 2047)} <= set(d)
    for c in hl.cases("action"):
        if c.kind == "ties" and c.V > 2:
            assert {(0, 1), (0, c.V - 1), (1, c.V - 1)} <= set(hl.tie_sets(c))
    for c in hl.all_cases():
        if c.kind == "ties":
            I = hl.inputs(c)
            top = I.z == I.z.max(1, keepdim=True).values
            assert [tuple(torch.nonzero(r).view(-1).tolist()) for r in top] == [tuple(t) for t in hl.tie_sets(c)]
            assert torch.equal(hl.reference(c, "f32").amax, I.tie_first)
    # bf16-grid rows tie on their own somewhere in the table (the reason the kind is there)
    assert any(int((hl.inputs(c).z == hl.inputs(c).z.max(1, keepdim=True).values).sum()) > hl.inputs(c).rows
               for c in hl.all_cases() if c.kind == "bf16grid")


def test_action_head_logits_lie_on_the_grid_that_keeps_the_argmax_well_defined():
    for c in hl.cases("action"):
        z = hl.inputs(c).z.double()
        assert torch.equal((z * 1024.0).round(), z * 1024.0)


# ---- the model passes at half the bound; the emulations at half the fp32 part ------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_model_and_emulations(group):
    worst = collections.defaultdict(float)
    for case in GROUPS[group]:
        I = hl.inputs(case)
        for fmt in hl.FMTS:
            T = hl.reference(case, fmt)
            rs = hl.judge(case, fmt, hl.model(case, fmt))
            # half the bound; a bf16 gradient may use its one rounding up (u |y| of u |y| + (1 + u) E: up to 1), and the loss the
            # rounding of its final subtraction (e |loss|, most of the bound of a large loss on a narrow row) counted in full
            assert all(abs(v) <= (1.0 if k.startswith("loss") or (fmt == "bf16" and k.startswith("dz")) else 0.5)
                       for k, v in rs.items()), (case, fmt, rs)
            if T.loss is None:                  # nothing is valid: a NaN loss and a gradient of exact zeros, judged by the flags above
                continue
            got = hl.model(case, fmt)["loss"].to(torch.float64).view(-1)
            err, rnd = (got - T.loss.y.view(-1)).abs(), hl.E32 * T.loss.y.view(-1).abs()
            assert bool((err <= rnd + 0.5 * (T.loss.bound.view(-1) - rnd)).all()), (case, fmt, "the model's loss")
            for order in hl.ORDERS:
                emu = hl.emulation(case, order, fmt)
                if case.kind == "onehot" or (case.kind == "uniform" and order != "online"):
                    # exact in float32 in every order (uniform rows: the register kernels' gradient, which `online` is not)
                    assert torch.equal(emu["dz"], T.dz.y), (case, fmt, order)
                    if case.kind == "onehot":
                        assert torch.equal(emu["loss"], T.loss.y), (case, fmt, order)
                    continue
                if case.kind == "uniform":
                    continue
                if order == "online" and case.head == "ce" and not case.two_pass:
                    Tt = hl.ce_reference_two_pass(case, fmt)       # the online algorithm is held to the two-pass kernel's bound
                else:
                    Tt = T
                # the loss: half the bound, the rounding of the final subtraction (e |loss|: the whole bound of a large loss on a
                # narrow row, which an honest implementation may use up) counted in full
                err = (emu["loss"] - Tt.loss.y).abs()
                rnd = hl.E32 * Tt.loss.y.abs()
                r = float(torch.where(err == 0, torch.zeros_like(err), err / Tt.loss.bound).max())
                worst["loss " + order] = max(worst["loss " + order], r)
                assert bool((err <= rnd + 0.5 * (Tt.loss.bound - rnd)).all()), (case, fmt, order, "loss", r)
                assert r <= 0.5 or case.kind == "wide", (case, fmt, order, "loss", r)
                err = (emu["dz"] - Tt.dz.y).abs()
                total = float(torch.where(err == 0, torch.zeros_like(err), err / Tt.dz.bound).max())
                assert total <= (0.5 if fmt == "f32" else 1.0), (case, fmt, order, "dz", total)
                worst["dz %s %s" % (fmt, order)] = max(worst["dz %s %s" % (fmt, order)], total)
                if fmt == "f32":
                    fp32 = float(torch.where(err == 0, torch.zeros_like(err), err / Tt.E).max())
                    assert fp32 <= 0.5, (case, order, "dz / E", fp32)
    print("LOSS-HOST %s: emulation / bound: %s" % (group, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())) or "exact only"))


# ---- the bound does not go vacuous ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", HEADS)
def test_bound_is_not_vacuous(head):
    top = collections.defaultdict(float)
    for case in hl.cases(head):
        T = hl.reference(case, "f32")
        if T.E is None or not RANDOM(case):
            continue
        v = hl.vacuity(case)
        if v is not None:
            top[case.V] = max(top[case.V], v * T.cap / hl.E32)
            assert v <= 1.0, (case, v)
        # what a case may hold: floor elements only in the wide kinds and at most half of a row; saturated label columns only in
        # `confident` rows (where they must occur) and rows of a width up to 9
        fl = T.floor.sum(1)
        assert int(fl.max()) == 0 or case.kind in ("wide", "wide12"), case
        assert int(fl.max()) * 2 <= case.V, (case, int(fl.max()))
        sat = T.saturated & (hl.inputs(case).y >= 0)
        assert not bool(sat.any()) or case.kind == "confident" or case.V <= 9, case
        if case.kind == "confident" and case.V > 1:
            assert bool(sat.any()), case
    assert any(int(hl.reference(c, "f32").floor.sum()) > 0 for c in hl.cases("ce") if c.two_pass)
    print("LOSS-HOST %s: largest E / (e N) per width: %s" % (head, ", ".join("%d: %.0f" % kv for kv in sorted(top.items()))))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def _rejecting_checks(case, fmt, mutant):
    rs = hl.judge(case, fmt, hl.model(case, fmt, mutant))
    return sorted(k for k, v in rs.items() if not abs(v) <= 1.0)


@pytest.mark.parametrize("head", HEADS)
def test_every_mutant_is_rejected(head):
    """Every mutant on every case it applies to; the checks that reject it are printed.  A mutant may hide on a case (a label one
    column off lands on a column of the same weight; a dropped tail column that carries no weight): the counts are printed."""
    for mutant in hl.MUTANTS[head]:
        if mutant == "truncating_bf16_convert":
            continue
        seen, hidden = collections.Counter(), 0
        for case in hl.cases(head):
            for fmt in hl.FMTS:
                if hl.mutant_applies(mutant, case, fmt):
                    checks = _rejecting_checks(case, fmt, mutant)
                    seen.update(checks)
                    hidden += not checks
        print("LOSS-HOST mutant %s: rejected by %s; hidden on %d case(s)" % (
            mutant, ", ".join("%s (%d)" % kv for kv in sorted(seen.items())) or "NOTHING", hidden))
        assert seen, mutant
        if mutant == "p_rounded_to_bf16_before_the_onehot":
            assert seen["dz err/bound"] and hidden == 0


def test_truncating_convert_is_seen_by_the_signed_statistic_only():
    """pooled over the random bf16 cases: invisible to the element bound (it stays within one unit round-off of the output), far
    outside the signed statistic; the rounding model sits inside it"""
    for head in HEADS:
        cs = [c for c in hl.cases(head) if hl.mutant_applies("truncating_bf16_convert", c, "bf16") and hl.reference(c, "bf16").dz]
        cut = lambda c, out: out["dzbuf"][:hl.inputs(c).rows, :c.V]
        good, n = hl.signed_pool([(c, cut(c, hl.model(c, "bf16"))) for c in cs])
        bad, _ = hl.signed_pool([(c, cut(c, hl.model(c, "bf16", "truncating_bf16_convert"))) for c in cs])
        print("LOSS-HOST signed statistic %s: N = %d, rounding %.2f, truncation %.1f" % (head, n, good, bad))
        assert n >= 100000, (head, n)
        assert abs(good) <= 1.0 and bad < -3.0, (head, good, bad)


def test_two_pass_bound_is_the_wider_one():
    """the online terms only ever add: a register-kernel case judged as if the two-pass kernel ran it has the larger bound"""
    case = [c for c in hl.cases("ce") if c.V == 1601 and c.kind == "normal"][0]
    a, b = hl.reference(case, "f32"), hl.ce_reference_two_pass(case, "f32")
    assert bool((b.dz.bound >= a.dz.bound).all()) and bool((b.loss.bound > a.loss.bound).all())
