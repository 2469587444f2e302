"""CPU: the turn-based task's modules construct with the reference's parameters, and the float64 restatements / bounds of
tests/helpers_turn_based.py are sound: a legitimate fp32 implementation sits far inside them, every wrong implementation of
the table falls outside, and the head's restatement is torch's CrossEntropyLoss plus autograd."""
import math
import os

import numpy as np
import pytest
import torch

import helpers_turn_based as ht

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_turn_based.npz")))


def test_modules_construct_with_the_reference_parameters(fx):
    from visitron_amd import rollout, turn_based

    want = {k[3:]: v.shape for k, v in fx.items() if k.startswith("sd.")}
    assert sorted(want) == sorted([
        "embedding.weight", "lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih", "lstm.bias_hh", "attention_layer.linear_in.weight",
        "attention_layer.linear_out.weight", "decoder2action.weight", "decoder2action.bias"])
    dec = turn_based.AttnDecoderLSTM(8, 6, 8, 128, 0.5, feature_size=70)
    got = {k: tuple(v.shape) for k, v in dec.state_dict().items()}
    assert got == {k: tuple(s) for k, s in want.items()}
    dec.load_state_dict({k[3:]: torch.from_numpy(v.astype(np.float32)) for k, v in fx.items() if k.startswith("sd.")})
    att = turn_based.SoftDotAttention(128)
    assert {k: tuple(v.shape) for k, v in att.state_dict().items()} == {"linear_in.weight": (128, 128), "linear_out.weight": (128, 256)}
    assert turn_based.OscarEncoder is rollout.OscarEncoder
    assert int(fx["oscar_encoder_same"]) == 1           # the two tasks' encoder classes computed the same bits
    assert turn_based.AttnDecoderLSTM(8, 6, 8, 128, 0.5).feature_size == 2048
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 70), torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(2, 3, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        turn_based.action_feedback(torch.zeros(2, 6), torch.zeros(2, dtype=torch.int64))


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_turn_based.npz")) < 1 << 20


HOST_CASES = [(5, 128, 8, 70), (17, 128, 3, 5), (3, 128, 64, 2054), (2, 512, 64, 2052)]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for c in HOST_CASES:
        o = ht.cell_operands(*c, seed=sum(c))
        out[c] = (o, ht.cell_reference(o))
    return out


@pytest.mark.parametrize("case", HOST_CASES)
def test_fp32_emulation_stays_below_half_of_every_bound(cases, case):
    o, ref = cases[case]
    for order in ("forward", "backward", "waves"):
        rs = ht.cell_ratios(o, ref, ht.cell_emulation_f32(o, order))
        assert all(r <= 0.5 for r in rs.values()), (order, rs)


@pytest.mark.parametrize("case", HOST_CASES)
def test_bound_is_below_the_value_on_99_percent(cases, case):
    o, ref = cases[case]
    for name, y, b in (("h", ref.h, ref.bh), ("c", ref.c, ref.bc)):
        frac = float((b < y.abs()).double().mean())
        assert frac >= 0.99, (name, frac)


# (dropping the last K mod 4 columns changes nothing where K is a multiple of 4: those pairs are not cases)
MUTANT_CASES = [(c, m) for c in HOST_CASES for m in ht.MUTANTS
                if m != "bf16_truncate" and not (m == "k_tail_dropped" and (c[2] + c[3]) % 4 == 0)]


@pytest.mark.parametrize("case,mutant", MUTANT_CASES)
def test_wrong_implementations_are_rejected(cases, case, mutant):
    o, ref = cases[case]
    assert ht.passes(ht.cell_ratios(o, ref, ht.cell_model(o)))
    rs = ht.cell_ratios(o, ref, ht.cell_model(o, mutant))
    assert not ht.passes(rs), rs


def test_truncating_convert_is_rejected_by_the_signed_bias():
    """Non-negative operands: round-to-nearest leaves no bias, truncation pushes every gate down."""
    o = ht.cell_operands(21, 512, 64, 2054, seed=7, kind="positive", block=True)
    ref = ht.cell_reference(o)
    good = ht.cell_ratios(o, ref, ht.cell_model(o), signed=True)
    assert ht.passes(good), good
    emu = ht.cell_ratios(o, ref, ht.cell_emulation_f32(o, "waves"), signed=True)
    assert ht.passes(emu) and abs(emu["gates signed bias"]) <= 0.5, emu
    bad = ht.cell_ratios(o, ref, ht.cell_model(o, "bf16_truncate"), signed=True)
    assert abs(bad["gates signed bias"]) > 1.0, bad


def test_exact_construction_is_exact():
    for c in ((17, 128, 3, 5), (5, 512, 64, 2054)):
        o = ht.cell_operands(*c, seed=3, kind="exact")
        ref = ht.cell_reference(o)
        assert bool((ref.gates[:, 2 * o.hs:3 * o.hs] == 0).all()) and torch.equal(ref.c, o.c_prev.double() * 0.5)
        for order in ("forward", "waves"):
            got = ht.cell_emulation_f32(o, order)
            assert torch.equal(got["c"], ref.c)
        assert float(o.w_ih.abs().sum()) > 0 and float(o.feature.abs().sum()) > 0


def test_out_of_range_id_counts_as_a_zero_row():
    o = ht.cell_operands(5, 128, 8, 70, seed=2)
    o.ids[1], o.ids[4] = o.A, -1
    rows = o.emb_rows()
    assert bool((rows[1] == 0).all()) and bool((rows[4] == 0).all()) and bool((rows[0] != 0).any())


# ---- the head ------------------------------------------------------------------------------------------------------------------------
def _torch_head(logit, target, blocked, ignore_index=-100):
    lg = logit.clone().double().requires_grad_()
    l = lg if blocked is None else lg.masked_fill(blocked.bool(), -math.inf)
    loss = torch.nn.CrossEntropyLoss(ignore_index=ignore_index)(l, target)
    if bool(torch.isfinite(loss)):
        loss.backward()
        return float(loss), lg.grad
    return float(loss), None


_head_case = ht.head_case


@pytest.mark.parametrize("A", [1, 6, 15, 64])
def test_head_restatement_is_torch_cross_entropy(A):
    logit, target, blocked = _head_case(37, A, 100 + A)
    open_t = ~blocked[torch.arange(37), target.clamp(min=0)] | (target == -100)
    target = torch.where(open_t, target, torch.full_like(target, -100))
    for bl in (None, blocked):
        ref = ht.head_reference(logit, target, bl)
        loss, grad = _torch_head(logit, target, bl)
        assert abs(ref.loss - loss) <= 1e-12 * max(1.0, abs(loss))
        assert float((ref.dlogit - grad).abs().max()) <= 1e-14
        assert 0 < ref.loss_bound <= 2.0 ** -18 * (1.0 + abs(loss))        # fp32-sized


def test_head_corners_are_torch():
    logit, target, blocked = _head_case(9, 6, 5)
    target = target.clamp(min=0)
    blocked[4, target[4]] = True                                  # a blocked target: +inf
    assert ht.head_reference(logit, target, blocked).loss == math.inf == _torch_head(logit, target, blocked)[0]
    none = torch.full((9,), -100)                                 # no counted row: what torch gives on the CPU
    got, want = ht.head_reference(logit, none, blocked).loss, _torch_head(logit, none, blocked)[0]
    assert math.isnan(want) and math.isnan(got)
    other = torch.where(target == 2, torch.full_like(target, 7), target)      # another ignore_index
    ref = ht.head_reference(logit, other, None, ignore_index=7)
    assert abs(ref.loss - _torch_head(logit, other, None, 7)[0]) <= 1e-12
    tie = torch.zeros(3, 6)
    tie[1, 2] = tie[1, 4] = 1.0
    assert ht.head_argmax(tie, None).tolist() == [0, 2, 0]
    bl = torch.zeros(3, 6, dtype=torch.bool)
    bl[0, 0] = bl[1, 2] = True
    assert ht.head_argmax(tie, bl).tolist() == [1, 4, 0]


def test_sampling_inputs_leave_few_rows_out():
    """64 rows x 8 seeds: the rows whose u lies within 1e-5 of a CDF step are at most 1 %, the picks are never blocked, and
    the fp32 statement of the rule (smallest a with cum > u * total) agrees on every other row."""
    logit, _, blocked = _head_case(*ht.SAMPLE_CASE)
    left_out = 0
    for seed in ht.SAMPLE_SEEDS:
        a, safe = ht.head_sample(logit, blocked, seed)
        left_out += int((~safe).sum())
        assert not bool(blocked[torch.arange(64), a][safe].any())
        l = logit.clone()
        l[blocked] = -math.inf
        e = torch.exp(l - l.max(1, keepdim=True).values)          # fp32
        cum = e.cumsum(1)
        u = torch.from_numpy(ht.sample_u(seed, 64)).float()
        pick = (cum <= (u * cum[:, -1])[:, None]).sum(1).clamp(max=5)
        assert torch.equal(pick[safe], a[safe])
        assert 0.0 <= float(u.min()) and float(u.max()) < 1.0
    assert left_out <= 0.01 * 64 * 8
    u = ht.sample_u(5, 4096)
    assert abs(float(u.mean()) - 0.5) < 0.02 and len(set(u.tolist())) > 4000
