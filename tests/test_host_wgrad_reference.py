"""tests/helpers_wgrad.py judged on the CPU: the bound accepts the model of the documented arithmetic and a float32 emulation in three
summation orders with a factor two to spare, rejects a table of subtly wrong implementations, never goes vacuous on the model's own
random data, the integer constructions stay below 2^24 (computed) and are exact in float32 in every order, the turn-order
fingerprint arithmetic gives 4 / 3 / 3, and every form of the family is reached under the restated dispatch rule at 256 CUs with
the table's hook / switch / mode values.  No GPU.

Cases of more than 2^31 multiply-adds (the production group) take their float64 products on the device; here they are held to the
dispatch rule, the computed partial-sum cap and the emulation of a sample of their elements only."""
import collections

import numpy as np
import pytest
import torch

import helpers_wgrad as hw

ALL = hw.all_cases()
GROUPS = collections.OrderedDict()
for _fam, _c in ALL:
    GROUPS.setdefault((_fam, _c.reaches), []).append(_c)
GROUP_IDS = ["%s-%s" % (f, r.replace(" ", "_")) for f, r in GROUPS]
MUTANT_MAX_MADDS = 1 << 30       # the mutants are judged on the cases up to this size ...
MUTANT_SKIP = ("M1100", "M1000", "M4100")     # ... and not on these: they repeat the forms of M1030 / M1024 / M2048


def _env(fam):
    return hw.FAMILY_ENV[fam]


@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_model_passes_and_the_emulation_stays_below_half(group):
    fam = group[0]
    worst = 0.0
    for case in GROUPS[group]:
        d = hw.case_dispatch(case, _env(fam))
        if not case.big:
            rs = hw.judge(case, hw.model(case, env=_env(fam)))
            assert hw.passes(rs), (case, {k: v for k, v in rs.items() if not abs(v) <= 1.0})
        if case.data == "fingerprint":
            continue
        I = hw.inputs(case)
        for order in hw.ORDERS:
            emu = hw.emulation(case, order, nsplit=max(2, d["nsplit"]))
            for i, p in enumerate(case.probs):
                ns, ks, tw, tb = emu[i]
                dy, x = I.dy[i].to(hw.F64)[:, ns], I.x[i].to(hw.F64)[:, ks]
                y = dy.t() @ x + (I.dw0[i].to(hw.F64)[ns][:, ks] if p.acc else 0.0)
                yb = dy.sum(0) + (I.db0[i].to(hw.F64)[ns] if (p.acc and p.db) else 0.0)
                if case.exact:
                    assert torch.equal(torch.from_numpy(tw).to(hw.F64), y), (case, order, i)
                    assert tb is None or torch.equal(torch.from_numpy(tb).to(hw.F64), yb), (case, order, i)
                    continue
                A = dy.abs().t() @ x.abs() + (I.dw0[i].to(hw.F64)[ns][:, ks].abs() if p.acc else 0.0)
                r = float(((torch.from_numpy(tw).to(hw.F64) - y).abs() / hw.bound_of(y, A, case.M)).max())
                if tb is not None:
                    Ab = dy.abs().sum(0) + (I.db0[i].to(hw.F64)[ns].abs() if p.acc else 0.0)
                    r = max(r, float(((torch.from_numpy(tb).to(hw.F64) - yb).abs() / hw.bound_of(yb, Ab, case.M)).max()))
                assert r <= 0.5, (case, order, i, r)
                worst = max(worst, r)
    print("WGRAD-HOST %s-%s: %d cases, fp32 emulation / bound at most %.4f" % (group + (len(GROUPS[group]), worst)))


def test_case_names_are_unique_and_every_case_says_why():
    for fam in hw.FAMILY_ENV:
        names = [c.name for c in hw.cases(fam)]
        assert len(names) == len(set(names)), [n for n, k in collections.Counter(names).items() if k > 1]
    for _, case in ALL:
        assert case.why and case.reaches in hw.FORMS
        assert case.data != "fingerprint" or case.fp == hw.fingerprint_expectation(case.reaches)
    print("WGRAD-HOST %d cases: %s" % (len(ALL), ", ".join("%s %d" % (f, len(hw.cases(f))) for f in hw.FAMILY_ENV)))


def test_every_case_and_every_random_case_has_its_exact_twins():
    for fam in hw.FAMILY_ENV:
        names = {c.name for c in hw.cases(fam)}
        for c in hw.cases(fam):
            if c.data == "random":
                assert c.name[:-len("random")] + "exact" in names and c.name[:-len("random")] + "census" in names, c
            assert c.data == "random" or c.M <= 12400


# ---- the restated rule reaches every form the table names ------------------------------------------------------------------------------
def test_every_case_reaches_its_form_at_256_cus():
    seen = collections.defaultdict(set)
    for fam, case in ALL:
        d = hw.case_dispatch(case, _env(fam), 256)
        assert d["form"] == case.reaches, (fam, case, d)
        seen["form"].add(d["form"])
        if d["form"] in (hw.FORM_128, hw.FORM_256):
            seen["remap " + d["form"]] |= d["remap"]
            seen["problems " + d["form"]].add(len(case.probs))
        else:
            seen["coords"] |= d["coords"]
            if d["nsplit"] == 2:
                seen["map"].add(d["order"])
                seen["map %d grids" % d["order"]].add(d["grid"])
            if d["form"] == hw.FORM_ATOMIC:
                seen["atomic ranges"].add(d["nsplit"])
    assert seen["form"] == set(hw.FORMS)
    for f in (hw.FORM_128, hw.FORM_256):
        assert seen["remap " + f] == {"xcd < r", "xcd >= r"}
        assert {1, 8} <= seen["problems " + f]
    assert seen["coords"] == {"k-tile outer", "n-tile outer"}
    assert seen["map"] == {0, 1} and seen["atomic ranges"] == {4, 8}
    assert all(g % 8 == 0 for g in seen["map 1 grids"]) and any(g % 8 for g in seen["map 0 grids"])
    # the round-4 map on a grid that IS a multiple of 8
    assert any(hw.case_dispatch(c, _env("split2_order0"))["grid"] % 8 == 0 and hw.case_dispatch(c, _env("split2_order0"))["order"] == 0
               for c in hw.cases("split2_order0"))


def test_named_dispatch_facts_of_the_table():
    env = {}
    P = hw.Prob
    prod = [P(n, k) for n, k in hw.PRODUCTION]
    d = hw.dispatch(prod, 12330, 0, False, env, 256)
    assert (d["form"], d["nsplit"], d["share"], d["grid"], d["order"], d["nk"], d["tiles"]) == (hw.FORM_TICKET, 2, 97, 216, 1, 193, 108)
    assert 12330 - 192 * 64 == 42
    assert hw.dispatch(prod, 12287, 0, False, env, 256)["form"] == hw.FORM_128
    s2 = {"VT_WGRAD_SPLIT": "2"}
    d = hw.dispatch([P(512, 512)], 1030, 8, False, s2, 256)
    assert (d["nsplit"], d["share"], d["grid"], d["order"], d["nk"]) == (2, 9, 8, 1, 17)
    d = hw.dispatch([P(256, 768)], 1030, 8, True, s2, 256)
    assert (d["form"], d["grid"], d["order"]) == (hw.FORM_DET, 6, 0)
    assert hw.dispatch([P(512, 512)], 1030, 8, False, dict(s2, VT_WGRAD_ORDER="0"), 256)["order"] == 0
    assert hw.dispatch([P(3072, 3072)], 1024, 8, True, s2, 256)["form"] == hw.FORM_ONE
    assert hw.dispatch([P(3072, 3072)], 1024, 8, True, s2, 288)["form"] == hw.FORM_DET
    assert hw.dispatch([P(256, 256)], 2048, 8, False, env, 256)["nsplit"] == 4
    assert hw.dispatch([P(768, 768), P(256, 1024)], 4100, 8, False, env, 256)["nsplit"] == 8
    assert hw.dispatch([P(256, 256)], 2048, 8, True, env, 256)["form"] == hw.FORM_128
    assert hw.dispatch([P(256, 256)], 1024, 0, False, env, 256)["form"] == hw.FORM_128
    m = {"VT_WGRAD_PERSISTENT_MIN_ROWS": "1024"}
    assert hw.dispatch([P(256, 256)], 1024, 0, False, m, 256)["form"] == hw.FORM_ONE
    assert hw.dispatch([P(256, 256)], 1023, 0, False, m, 256)["form"] == hw.FORM_128
    assert hw.dispatch([P(256, 256)], 448, 8, False, env, 256)["form"] == hw.FORM_128      # fewer than 8 K-steps
    assert hw.dispatch([P(256, 260)], 1024, 8, False, env, 256)["form"] == hw.FORM_128
    for bad in (lambda: hw.dispatch([], 64, 0, False), lambda: hw.dispatch([P(8, 8)] * 9, 64, 0, False),
                lambda: hw.dispatch([P(8, 8)], 0, 0, False), lambda: hw.dispatch([P(8, 6)], 64, 0, False)):
        with pytest.raises(ValueError):
            bad()
    for fam in hw.FAMILY_ENV:
        for c in hw.sequence_cases("default" if fam == "default" else "split2"):
            assert hw.case_dispatch(c, _env("default" if fam == "default" else "split2"))["form"] == c.reaches, c


# ---- exactness -----------------------------------------------------------------------------------------------------------------------
def test_fingerprint_arithmetic():
    assert hw.fingerprint_arithmetic() == (4.0, 3.0, 3.0)
    f = np.float32
    assert float(f(f(2.0 ** 24) + f(3))) == 2.0 ** 24 + 4      # the tie rounds to even
    for fam, case in ALL:
        if case.data == "fingerprint":
            got = hw.fingerprint_values(case, hw.model(case, env=_env(fam)))
            want = [4.0] if case.reaches == hw.FORM_DET else [3.0] if len(case.fp) == 1 else [4.0]   # (ticket: the in-order member)
            assert got == want, (case, got)
            flipped = hw.fingerprint_values(case, hw.model(case, "ranges_added_in_the_opposite_order", env=_env(fam)))
            assert flipped == [3.0], (case, flipped)


def test_integer_constructions_stay_below_2_pow_24():
    top = 0.0
    for fam, case in ALL + [("seq", c) for f in ("default", "split2") for c in hw.sequence_cases(f)]:
        if case.exact:
            cap = hw.integer_partial_sum_cap(case)
            assert cap < 2.0 ** 24, (case, cap)
            top = max(top, cap)
    print("WGRAD-HOST integer constructions: largest |partial sum| cap %d of %d" % (top, 2 ** 24))


# ---- the bound does not go vacuous ---------------------------------------------------------------------------------------------------
def test_bound_is_not_vacuous_on_the_random_data():
    worst = 1.0
    for fam, case in ALL:
        if case.data != "random":
            continue
        for rw, rb in hw.reference(case):
            for r in (rw, rb):
                if r is not None:
                    share = float((r.bound < r.y.abs()).double().mean())
                    assert share >= 0.99, (case, share)
                    worst = min(worst, share)
    print("WGRAD-HOST bound < |y| on at least %.4f of the elements of every random case" % worst)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
_SEEN = collections.defaultdict(lambda: collections.defaultdict(list))


def _what_caught(case):
    return {"random": "bound", "exact": "exact construction", "census": "row census", "fingerprint": "fingerprint"}[case.data]


@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_mutants(group):
    """Every mutant on every case of the group it applies to; which kind of check rejects it is recorded for the test below.  A
    mutant may hide on a case (integer products are bf16-exact, a symmetric corner is its own transpose): the counts are printed."""
    fam = group[0]
    seen, hidden = collections.defaultdict(list), collections.defaultdict(list)
    for case in GROUPS[group]:
        if (case.madds > MUTANT_MAX_MADDS or (case.reaches == hw.FORM_256 and case.data != "fingerprint") or fam == "split2_order0"
                or any(t in case.name for t in MUTANT_SKIP)):
            continue                                    # (the 256-wide and round-4-map cases repeat shapes and data layout)
        d = hw.case_dispatch(case, _env(fam))
        for mutant in hw.MUTANTS:
            if hw.mutant_applies(mutant, case, d):
                rs = hw.judge(case, hw.model(case, mutant, env=_env(fam)))
                if hw.passes(rs):
                    hidden[mutant].append(case.name)
                else:
                    seen[mutant].append(case.name)
                    _SEEN[mutant][_what_caught(case)].append(case.name)
    for mutant in hw.MUTANTS:
        if seen[mutant] or hidden[mutant]:
            print("WGRAD-HOST mutant %s on %s-%s: rejected on %d case(s), hidden on %d" % (
                (mutant,) + group + (len(seen[mutant]), len(hidden[mutant]))))


def test_zz_no_mutant_goes_unrejected():
    """(runs after test_mutants: files run in order; alone it judges the mutants on the small one-tile cases itself)"""
    if not _SEEN:
        for fam, case in ALL:
            if case.madds <= (1 << 22) and case.reaches != hw.FORM_256 or case.data == "fingerprint" and case.madds <= MUTANT_MAX_MADDS:
                d = hw.case_dispatch(case, _env(fam))
                for mutant in hw.MUTANTS:
                    if hw.mutant_applies(mutant, case, d) and not hw.passes(hw.judge(case, hw.model(case, mutant, env=_env(fam)))):
                        _SEEN[mutant][_what_caught(case)].append(case.name)
    print("WGRAD-HOST mutant table (cases that reject it, by the kind of check):")
    for mutant in hw.MUTANTS:
        by = _SEEN[mutant]
        print("WGRAD-HOST   %-46s %s" % (mutant, ", ".join("%s %d" % (k, len(v)) for k, v in sorted(by.items())) or "NOT REJECTED"))
    for mutant in hw.MUTANTS:
        assert _SEEN[mutant], "no case rejects %s" % mutant
    assert "fingerprint" in _SEEN["ranges_added_in_the_opposite_order"]      # (nothing else can see it: both orders are inside the bound)


def test_census_names_the_rows():
    """A dropped last row and a block added twice, on a row census: the report names exactly those token rows."""
    case = [c for c in hw.cases("split2") if c.name == "ticket M1030 512x512 census"][0]
    env = _env("split2")
    outs = hw.model(case, "last_row_dropped", env=env)
    assert not hw.passes(hw.judge(case, outs))
    assert "missing, token rows [1029]" in hw.census_report(case, outs)
    rep = hw.census_report(case, hw.model(case, "range_boundary_block_added_twice", env=env), limit=64)
    assert "64 element(s) duplicated" in rep and all(str(m) in rep for m in (512, 575))
    assert hw.census_report(case, hw.model(case, env=env)) == ""
