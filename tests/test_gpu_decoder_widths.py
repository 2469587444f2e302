"""GPU: the panoramic decoder at widths that are no multiple of 4 -- the reference's default feature width 2058 = 2054 + 4
(tasks/viewpoint_select/params.py:163-167, agent.py:124) -- through every kernel that used to need the grid:
vt_softdot_attention_f32 and its two backward forms, vt_skinny_linear_f32, the decoder's cell route and autograd nodes, and
the feature store's two gathers.

Exact constructions first: integer data for which every result is exactly representable whatever the order of the sums, so
the comparison is EQUAL.  Every operand is a strided view inside a NaN-filled buffer (a load one element outside a row turns
the result into NaN), in three layouts: row strides of 1 mod 4 floats (rows walk all four residues mod 16 bytes), tight rows
on a 16-byte aligned base (the 8-byte path where D % 4 == 2) and even strides on a base at 8 mod 16.  Then random data
against float64 with the accumulation bound tests/helpers_gemm.py derives, the modules against the oracle (which is bitwise
the reference) with the tolerances of tests/test_gpu_rollout.py / test_gpu_rollout_train.py, and the feature store bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import check_close, maxabs, model_pair

pytestmark = pytest.mark.gpu

NAN = float("nan")
D_VALUES = [1, 2, 3, 5, 6, 130, 1026, 1027, 2058, 4094, 4095]
LAYOUTS = ("walk", "tight", "even")


def _geometry(layout, D, L):
    """-> (row stride, batch stride, offset of the context, offset of the target) in floats."""
    if layout == "walk":
        ld_row = D + 1 + (-D) % 4           # the smallest stride > D that is 1 mod 4
        return ld_row, L * ld_row + 3, 5, 1
    if layout == "tight":
        return D, L * D, 64, 64
    ld_row = D + 2 - D % 2                  # even, > D
    return ld_row, L * ld_row + 2, 2, 2


def _strided(values, layout, dev):
    """values [B, L, D] (CPU) -> the same numbers as a strided device view inside a NaN-filled buffer."""
    B, L, D = values.shape
    ld_row, ld_batch, off, _ = _geometry(layout, D, L)
    buf = torch.full((off + B * ld_batch + 64,), NAN, dtype=torch.float32, device=dev)
    view = buf.as_strided((B, L, D), (ld_batch, ld_row, 1), off)
    view.copy_(values.to(dev))
    return view


def _rows(values, layout, dev):
    """values [B, D] -> a contiguous device view inside a NaN-filled buffer, at the layout's target offset."""
    B, D = values.shape
    off = _geometry(layout, D, 1)[3]
    buf = torch.full((off + B * D + 64,), NAN, dtype=torch.float32, device=dev)
    view = buf[off:off + B * D].view(B, D)
    view.copy_(values.to(dev))
    return view


def _kept(L):
    """The largest power of two of keys that still leaves one masked (all of them at L = 1)."""
    n = 1
    while 2 * n < L:
        n *= 2
    return n


def _equal_logit_case(B, L, D, seed, all_masked_rows=(), most=1 << 30):
    """Small-integer context, NaN under the masked keys, a mask that leaves n = 2^k <= most keys per row."""
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randint(-4, 5, (B, L, D), generator=g).float()
    n = min(_kept(L), most)
    mask = torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        if b not in all_masked_rows:
            mask[b, torch.randperm(L, generator=g)[:n]] = False
    ctx[mask] = NAN
    return ctx, mask, n


def _eq(got, want):
    """EQUAL, with NaN equal to NaN."""
    got, want = got.detach().cpu(), want.detach().cpu().to(got.dtype)
    return got.shape == want.shape and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all())


# ---- the soft-dot forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", D_VALUES)
def test_softdot_column_census(dev, D):
    """target one-hot at column j: logit[b, l] == context[b, l, j] exactly.  j at both ends of the row: the tail past the last
    multiple of 4 (or 2) is where a path with wide loads goes wrong."""
    from visitron_amd import ops

    for L in (1, 8, 36):
        for B in (1, 3):
            g = torch.Generator().manual_seed(1000 * D + 10 * L + B)
            ctx = torch.randint(-8, 9, (B, L, D), generator=g).float()
            for layout in LAYOUTS:
                c = _strided(ctx, layout, dev)
                for j in sorted({j for j in (0, 1, D - 3, D - 2, D - 1) if 0 <= j < D}):
                    t = torch.zeros(B, D)
                    t[:, j] = 1.0
                    weighted, logit = ops.softdot_attention(_rows(t, layout, dev), c, None, True, True, False)
                    assert _eq(logit, ctx[:, :, j]), (D, L, B, layout, j)
                    assert bool(torch.isfinite(weighted).all()), (D, L, B, layout, j)


@pytest.mark.parametrize("D", D_VALUES)
def test_softdot_equal_logits_and_masked_keys(dev, D):
    """target = 0 and 2^k unmasked keys: p == 2^-k exactly and weighted[d] is the exact mean of small integers.  The masked
    keys hold NaN: they are never multiplied into the sum.  A row with every key masked is NaN."""
    from visitron_amd import ops

    for L in (1, 8, 36):
        for B in (1, 3):
            ctx, mask, n = _equal_logit_case(B, L, D, 7 * D + L + B, all_masked_rows=(1,))
            live = ~mask.all(1)
            p = torch.where(mask, torch.zeros(()), torch.full((), 1.0 / n))
            p[~live] = NAN
            w = torch.where(mask[:, :, None], torch.zeros(()), ctx).double().sum(1) / n     # exact: |sum| <= 4 * 32
            w[~live] = NAN
            for layout in LAYOUTS:
                c, t = _strided(ctx, layout, dev), _rows(torch.zeros(B, D), layout, dev)
                weighted, prob = ops.softdot_attention(t, c, mask.to(dev), True, True, True)
                assert _eq(prob, p), (D, L, B, layout)
                assert _eq(weighted, w.float()), (D, L, B, layout)
                _, logit = ops.softdot_attention(t, c, mask.to(dev), False, True, False)
                want = torch.where(mask, torch.full((), -float("inf")), torch.zeros(()))
                assert _eq(logit, want), (D, L, B, layout)


# ---- the soft-dot backward, both forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", D_VALUES)
def test_softdot_backward_exact_with_equal_logits(dev, D):
    """The same data with integer d_weighted and d_attn, masked logits returned: p = 1/n on the n = 2^k kept keys, so
       dp = ctx . d_weighted,  dlog = (dp - mean dp) / n + d_attn on the kept keys and 0 on the masked ones,
       d_target = sum_l dlog[l] ctx[l],  d_context[l] = p[l] d_weighted        (target = 0)
    are exact in any order of the sums (asserted on the data below).  L = 8, 36: the single-workgroup form; L = 132: the split pair."""
    from visitron_amd import ops

    assert 36 < ops.SOFTDOT_SPLIT_KEYS <= 132
    for L in (8, 36, 132):
        for B in (1, 3):
            # (at most 32 kept keys: 128 of L = 132 would take the d_target sums past what fp32 holds exactly)
            ctx, mask, n = _equal_logit_case(B, L, D, 11 * D + L + B, most=32)
            g = torch.Generator().manual_seed(D + L)
            dw = torch.randint(-1, 2, (B, D), generator=g).float()
            da = torch.randint(-2, 3, (B, L), generator=g).float()
            c0 = torch.where(mask[:, :, None], torch.zeros(()), ctx).double()
            dp = (c0 * dw.double()[:, None, :]).sum(2)
            keep = (~mask).double()
            dlog = keep * ((dp - (dp * keep).sum(1, keepdim=True) / n) / n + da.double())
            d_t = (dlog[:, :, None] * c0).sum(1)
            d_c = keep[:, :, None] / n * dw.double()[:, None, :]
            # exactness in any order: every partial sum, in units of the finest term (1 / n^2), stays below 2^24
            assert float((c0.abs() * dw.abs().double()[:, None, :]).sum(2).max()) < 2 ** 24
            assert float((dlog.abs()[:, :, None] * c0.abs()).sum(1).max()) * n * n < 2 ** 24
            assert float(dp.abs().sum(1).max()) * n < 2 ** 24
            for layout in LAYOUTS:
                c, t = _strided(ctx, layout, dev), _rows(torch.zeros(B, D), layout, dev)
                got_t, got_c = ops.softdot_attention_bwd(t, c, mask.to(dev), _rows(dw, layout, dev), da.to(dev), False, True)
                assert _eq(got_t, d_t.float()), (D, L, B, layout)
                assert _eq(got_c, d_c.float()), (D, L, B, layout)


@pytest.mark.parametrize("D,L", [(2058, 36), (2058, 160), (1027, 36), (1027, 160), (134, 7)])
def test_softdot_backward_matches_float64_autograd(dev, D, L):
    """Random data through both backward forms against torch autograd in float64 (the bound of
    test_gpu_rollout_train.test_softdot_backward_matches_autograd: 1e-4 relative L2)."""
    from visitron_amd import ops

    g = torch.Generator().manual_seed(D + L)
    B = 3
    t, c = torch.randn(B, D, generator=g) * 0.2, torch.randn(B, L, D, generator=g) * 0.5
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[1, L // 2:] = True
    dw, da = torch.randn(B, D, generator=g), torch.randn(B, L, generator=g)
    for prob in (True, False):
        tr, cr = t.double().requires_grad_(True), c.double().requires_grad_(True)
        logit = torch.bmm(cr, tr.unsqueeze(2)).squeeze(2).masked_fill(mask, -float("inf"))
        p = torch.softmax(logit, 1)
        out_a = p if prob else logit
        fin = torch.isfinite(out_a)
        ((torch.bmm(p.unsqueeze(1), cr).squeeze(1) * dw).sum() + (torch.where(fin, out_a, torch.zeros_like(out_a)) * da).sum()).backward()
        for layout in ("tight", "walk"):
            d_t, d_c = ops.softdot_attention_bwd(_rows(t, layout, dev), _strided(c, layout, dev), mask.to(dev), dw.to(dev), da.to(dev), prob, True)
            for name, got, want in (("d_target", d_t, tr.grad), ("d_context", d_c, cr.grad)):
                rel = float((got.cpu().double() - want).norm() / want.norm())
                check_close("softdot bwd D%d L%d %s %s %s rel-L2" % (D, L, "prob" if prob else "logit", layout, name), rel, 0.0, 1e-4)


# ---- the soft-dot forward on random data ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 130, 1027, 2058, 4094, 4095])
def test_softdot_random_against_float64(dev, D):
    """logit: |got - y| <= (D + 8) 2^-23 sum |c t| per element, the accumulation form of tests/helpers_gemm.py (D products, any
    summation tree, fp32 operands that are exact in float64); probabilities 2e-2, weighted context 5e-2 as in
    tests/test_gpu_rollout.py."""
    from visitron_amd import ops

    B, L = 3, 36
    g = torch.Generator().manual_seed(D)
    t, c = torch.randn(B, D, generator=g) * 0.2, torch.randn(B, L, D, generator=g) * 0.5
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[1, 20:] = True
    prod = c.double() * t.double()[:, None, :]
    y, bound = prod.sum(2), (D + 8) * 2.0 ** -23 * prod.abs().sum(2)
    p = torch.softmax(y.masked_fill(mask, -float("inf")), 1)
    w = torch.bmm(p.unsqueeze(1), c.double()).squeeze(1)
    for layout in LAYOUTS:
        td, cd = _rows(t, layout, dev), _strided(c, layout, dev)
        weighted, logit = ops.softdot_attention(td, cd, mask.to(dev), True, True, False)
        err = (logit.cpu().double() - y).abs()
        worst = float((err / bound)[~mask].max())
        print("SOFTDOT D%d %s: worst logit error / bound = %.3f" % (D, layout, worst))
        assert bool((err <= bound)[~mask].all()) and bool(torch.isinf(logit.cpu()[mask]).all()), (D, layout, worst)
        _, prob = ops.softdot_attention(td, cd, mask.to(dev), False, True, True)
        check_close("softdot D%d %s probabilities" % (D, layout), prob, p.float(), 2e-2)
        check_close("softdot D%d %s weighted" % (D, layout), weighted, w.float(), 5e-2)


@pytest.mark.parametrize("D,L", [(2058, 36), (1027, 8), (134, 7)])
def test_softdot_module_matches_oracle_off_the_grid(dev, D, L):
    """SoftDotAttention.forward in its four output modes, with and without a mask, against the oracle: the bounds of
    test_gpu_rollout.test_softdot_attention_module (5e-2 on h_tilde / weighted, 2e-2 on probabilities, 2e-2 relative on logits)."""
    from oracle.rollout import SoftDotAttention as OSoft
    from visitron_amd.rollout import SoftDotAttention

    Q, B = 128, 5
    torch.manual_seed(1)
    ref = OSoft(Q, D).eval()
    prod = SoftDotAttention(Q, D).eval()
    prod.load_state_dict(ref.state_dict())
    prod = prod.to(dev)
    g = torch.Generator().manual_seed(D + L)
    h, ctx = torch.randn(B, Q, generator=g), torch.randn(B, L, D, generator=g) * 0.5
    mask = torch.zeros(B, L, dtype=torch.bool)
    mask[1, L // 2:] = True
    mask[3, :2] = True
    for m in (None, mask):
        for tilde in (True, False):
            for prob in (True, False):
                with torch.no_grad():
                    w0, w1 = ref(h, ctx, None if m is None else m.clone(), output_tilde=tilde, output_prob=prob)
                    g0, g1 = prod(h.to(dev), ctx.to(dev), None if m is None else m.to(dev), output_tilde=tilde, output_prob=prob)
                assert g0.shape == w0.shape and g1.shape == w1.shape
                assert maxabs(g0, w0) < 5e-2
                if prob:
                    assert maxabs(g1, w1) < 2e-2
                else:
                    fin = torch.isfinite(w1)
                    assert bool((torch.isfinite(g1.cpu()) == fin).all())
                    assert float(((g1.cpu() - w1)[fin]).abs().max()) < 2e-2 * max(1.0, float(w1[fin].abs().max()))


def test_softdot_module_trains_at_width_134(dev):
    """SoftDotAttention(128, 134) with output_tilde: linear_out has K = 262 and linear_in N = 134, the two padded
    weight-gradient problems of rollout_autograd._Dense, against autograd through the oracle."""
    from oracle.rollout import SoftDotAttention as OSoft
    from visitron_amd.rollout import SoftDotAttention
    from test_gpu_rollout_train import _grads_close, _rel

    Q, D, B, L = 128, 134, 5, 7
    torch.manual_seed(2)
    ref = OSoft(Q, D).train()
    prod = SoftDotAttention(Q, D).train()
    prod.load_state_dict(ref.state_dict())
    prod = prod.to(dev)
    g = torch.Generator().manual_seed(3)
    h, ctx = torch.randn(B, Q, generator=g), torch.randn(B, L, D, generator=g) * 0.5
    gh, ga = torch.randn(B, Q, generator=g), torch.randn(B, L, generator=g)
    hr, cr = h.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    w0, w1 = ref(hr, cr)
    ((w0 * gh).sum() + (w1 * ga).sum()).backward()
    hd, cd = h.to(dev).requires_grad_(True), ctx.to(dev).requires_grad_(True)
    g0, g1 = prod(hd, cd)
    check_close("softdot 134 train h_tilde", g0, w0, 5e-2)
    check_close("softdot 134 train probabilities", g1, w1, 2e-2)
    ((g0 * gh.to(dev)).sum() + (g1 * ga.to(dev)).sum()).backward()
    check_close("softdot 134 train dh rel-L2", _rel(hd.grad, hr.grad), 0.0, 2e-2)
    check_close("softdot 134 train dctx rel-L2", _rel(cd.grad, cr.grad), 0.0, 2e-2)
    for p in prod.parameters():
        assert p.grad.shape == p.shape
    _grads_close("softdot 134 train", prod, ref, 2e-2)


# ---- skinny_linear -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K1", [0, 3, 2058])
def test_skinny_linear_exact_on_integers(dev, K1):
    """Integer activations and weights with |v| <= 16 (exact in bf16): the largest partial sum stays below 2^24, so the fp32
    outputs are exact.  Column c of [x0 | x1] straddles the two sources wherever K0 % 4 != 0."""
    from visitron_amd import ops
    from visitron_amd.ops import round_up

    for K0 in (2, 6, 64):
        K = K0 + K1
        Kpad = round_up(K, 64)
        for M in (1, 7, 17):
            for N in (1, 5, 18):
                g = torch.Generator().manual_seed(K + 100 * M + N)
                x = torch.randint(-16, 17, (M, K), generator=g).float()
                w = torch.randint(-16, 17, (N, K), generator=g).float()
                bias = torch.randint(-16, 17, (N,), generator=g).float()
                assert float((x.abs().double() @ w.abs().double().t()).max()) + 16 < 2 ** 24     # every partial sum
                w_pad = torch.zeros(N, Kpad, dtype=torch.bfloat16)
                w_pad[:, :K] = w.to(torch.bfloat16)
                assert torch.equal(w_pad[:, :K].float(), w)
                w_pad = w_pad.to(dev)
                y = x.double() @ w.double().t()
                for layout in LAYOUTS:
                    x0 = _strided(x[None, :, :K0], layout, dev)[0]
                    x1 = _strided(x[None, :, K0:], layout, dev)[0] if K1 else None
                    for b in (None, bias):
                        got = ops.skinny_linear(x0, w_pad, None if b is None else b.to(dev), x1)
                        want = y if b is None else y + b.double()
                        assert _eq(got, want.float()), (K0, K1, M, N, layout, b is not None)


def test_skinny_linear_tanh_straddling_the_seam_matches_float64(dev):
    """act = tanh over [weighted | h] as SoftDotAttention.linear_out calls it at 2058 + 512, random data: 5e-2 (the bf16 path)."""
    from visitron_amd import ops
    from visitron_amd.ops import ACT_TANH

    g = torch.Generator().manual_seed(5)
    M, K0, K1, N = 7, 2058, 512, 512
    x0, x1 = torch.randn(M, K0, generator=g) * 0.3, torch.randn(M, K1, generator=g) * 0.3
    w = (torch.randn(N, K0 + K1, generator=g) * 0.02).to(torch.bfloat16)
    w_pad = torch.zeros(N, 2624, dtype=torch.bfloat16)
    w_pad[:, :K0 + K1] = w
    want = torch.tanh(torch.cat((x0, x1), 1).double() @ w.double().t())
    got = ops.skinny_linear(_strided(x0[None], "walk", dev)[0], w_pad.to(dev), None, _strided(x1[None], "even", dev)[0], ACT_TANH)
    check_close("skinny_linear 2058 + 512 tanh", got, want.float(), 5e-2)


# ---- the decoder modules against the oracle ------------------------------------------------------------------------------------
def _decoder_pair(dev, hs, feat, seed=2):
    from oracle.rollout import AttnDecoderLSTM as ODec
    from visitron_amd.rollout import AttnDecoderLSTM

    torch.manual_seed(seed)
    ref = ODec(4, 64, hs, 0.5, feature_size=feat).eval()
    prod = AttnDecoderLSTM(4, 64, hs, 0.5, feature_size=feat).eval()
    prod.load_state_dict(ref.state_dict())
    return ref, prod.to(dev)


def _decoder_inputs(hs, feat, B=3, L=5, C=4, seed=5):
    g = torch.Generator().manual_seed(seed)
    action = torch.randn(B, 4, generator=g)
    feature = torch.randn(B, 36, feat, generator=g).abs() * 0.3
    cand = torch.randn(B, C, feat, generator=g).abs() * 0.3
    h1, c0 = torch.randn(B, hs, generator=g) * 0.3, torch.randn(B, hs, generator=g) * 0.3
    ctx = torch.randn(B, L, hs, generator=g) * 0.5
    cmask = torch.zeros(B, L, dtype=torch.bool)
    cmask[1, 3:] = True                     # a ragged instruction mask
    cmask[2, 1:] = True
    return action, feature, cand, h1, c0, ctx, cmask


OLD_ROUTE = ["skinny_linear", "skinny_linear", "softdot_attention", "skinny_linear", "lstm_step", "skinny_linear",
             "softdot_attention", "skinny_linear", "skinny_linear", "softdot_attention"]
FUSED_ROUTE = OLD_ROUTE[:3] + ["turn_lstm_cell"] + OLD_ROUTE[5:]


def _launches(dec, args):
    """The launch record of one direct inference step."""
    from visitron_amd import ops

    ops.profile_begin()
    try:
        with torch.no_grad():
            dec(*args)
        names = [rec[0] for rec in ops._prof]
    finally:
        ops.profile_end()
    return names


@pytest.mark.parametrize("hs,feat", [(128, 134), (512, 2058)])
def test_decoder_step_off_the_grid_matches_oracle_and_its_graph_replay(dev, hs, feat):
    """AttnDecoderLSTM.forward at feature widths 134 and 2058 (the reference's default): two chained steps against the oracle
    with the bounds of test_gpu_rollout.test_decoder_step_matches_oracle, the graph replay equal to the direct step bit for
    bit, and the launch record of the fused-cell route."""
    ref, prod = _decoder_pair(dev, hs, feat)
    action, feature, cand, h1, c0, ctx, cmask = _decoder_inputs(hs, feat)
    to = lambda t: t.to(dev)
    want_state, got_state, graph_state = (h1, c0), (to(h1), to(c0)), (to(h1), to(c0))
    for _ in range(2):
        with torch.no_grad():
            want = ref(action, feature, cand, None, want_state[0], want_state[1], ctx, cmask.clone())
            prod.use_graph = False
            got = prod(to(action), to(feature), to(cand), None, got_state[0], got_state[1], to(ctx), to(cmask))
            prod.use_graph = True
            rep = prod(to(action), to(feature), to(cand), None, graph_state[0], graph_state[1], to(ctx), to(cmask))
            prod.use_graph = False
        assert len(got) == len(want) == len(rep) == 4
        for gi, wi, ri in zip(got, want, rep):
            assert gi.shape == wi.shape and torch.equal(gi, ri)
        assert maxabs(got[0], want[0]) < 5e-2 and maxabs(got[1], want[1]) < 5e-2 and maxabs(got[3], want[3]) < 5e-2
        assert maxabs(got[2], want[2]) < 2e-2 * max(1.0, float(want[2].abs().max()))
        want_state, got_state, graph_state = (want[3], want[1]), (got[3], got[1]), (rep[3], rep[1])
    assert len(prod._graphs) == 1
    assert float(to(c0).sub(got_state[1]).abs().max()) > 0        # the caller's c_0 was not updated in place
    args = (to(action), to(feature), to(cand), None, to(h1), to(c0), to(ctx), to(cmask))
    assert _launches(prod, args) == FUSED_ROUTE


@pytest.mark.parametrize("hs,feat", [(128, 132), (512, 2052)])
def test_decoder_step_on_the_grid_keeps_its_launch_sequence(dev, hs, feat):
    """At multiples of 4 nothing moved: the ten launches of the shipped step, in their order."""
    _, prod = _decoder_pair(dev, hs, feat)
    action, feature, cand, h1, c0, ctx, cmask = (t.to(dev) for t in _decoder_inputs(hs, feat))
    assert _launches(prod, (action, feature, cand, None, h1, c0, ctx, cmask)) == OLD_ROUTE


def test_rollout_training_at_width_134_matches_oracle(dev):
    """test_gpu_rollout_train.test_rollout_training_matches_oracle at feature width 134: encoder + two teacher-forced decoder
    steps + cross entropy; every parameter gradient of encoder and decoder and the gradients of the feature and candidate
    tensors against the oracle, with that test's tolerances."""
    from oracle.modeling import PreTrainOscar as OModel
    from oracle.rollout import AttnDecoderLSTM as ODec, OscarEncoder as OEnc
    from test_gpu_rollout_train import _grads_close, _rel
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.rollout import AttnDecoderLSTM, OscarEncoder
    from visitron_amd.training import _bridge_engine

    cfg = mini_config(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref_m, prod_m = model_pair(OModel, PreTrainOscar, cfg, seed=43, device=dev)
    hs, feat = 128, 134
    torch.manual_seed(6)
    r_enc = OEnc(None, ref_m.bert, hs, hs, 0.0)
    p_enc = OscarEncoder(None, prod_m.bert, hs, hs, 0.0)
    p_enc.load_state_dict({k: v for k, v in r_enc.state_dict().items() if not k.startswith("bert.")}, strict=False)
    r_dec = ODec(4, 64, hs, 0.0, feature_size=feat)
    p_dec = AttnDecoderLSTM(4, 64, hs, 0.0, feature_size=feat)
    p_dec.load_state_dict(r_dec.state_dict())
    p_enc, p_dec = p_enc.to(dev), p_dec.to(dev)
    for m in (r_enc, p_enc, r_dec, p_dec):
        m.train()
    _bridge_engine(p_enc.bert).compact_min_rows = 1 << 30
    B, S, C = 5, 24, 6
    g = torch.Generator().manual_seed(9)
    lens = [24, 20, 13, 13, 6]
    ids = torch.randint(1, cfg.vocab_size, (B, S), generator=g)
    pad = torch.zeros(B, S, dtype=torch.bool)
    for i, n in enumerate(lens):
        pad[i, n:] = True
        ids[i, n:] = 0
    action = torch.randn(B, 4, generator=g)
    feature = torch.randn(B, 36, feat, generator=g).abs() * 0.3
    cand = torch.randn(B, C, feat, generator=g).abs() * 0.3
    target = torch.randint(0, C, (2, B), generator=g)

    def run(enc, dec, to):
        f, c = to(feature).requires_grad_(True), to(cand).requires_grad_(True)
        ctx, h_t, c_t = enc(to(ids), lens, to(pad))
        ctx_mask = to(pad)[:, : ctx.shape[1]]
        loss, h1 = 0.0, h_t
        for step in range(2):
            h_t, c_t, logit, h1 = dec(to(action), f, c, h1, h_t, c_t, ctx, ctx_mask)
            loss = loss + nn.functional.cross_entropy(logit, to(target[step]))
        return loss, ctx, logit, f, c

    wl, wctx, wlogit, wf, wc = run(r_enc, r_dec, lambda t: t.clone())
    wl.backward()
    gl, gctx, glogit, gf, gc = run(p_enc, p_dec, lambda t: t.to(dev))
    check_close("rollout train 134 ctx", gctx, wctx, 5e-2)
    check_close("rollout train 134 logit", glogit, wlogit, 5e-2)
    check_close("rollout train 134 loss", float(gl.detach()), float(wl.detach()), 5e-2)
    gl.backward()
    _grads_close("rollout train 134 encoder", p_enc, r_enc, 4e-2)
    _grads_close("rollout train 134 decoder", p_dec, r_dec, 4e-2)
    assert p_dec.lstm.weight_ih.grad.shape == (4 * hs, 64 + feat)
    check_close("rollout train 134 d_feature rel-L2", _rel(gf.grad, wf.grad), 0.0, 4e-2)
    check_close("rollout train 134 d_candidate rel-L2", _rel(gc.grad, wc.grad), 0.0, 4e-2)


# ---- the feature store ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [6, 2054])
def test_feature_store_gathers_bit_for_bit_at_even_widths(dev, D):
    """Both kernels at D = 2 mod 4 (8-byte pieces; 2054 is the reference's default): store rows and output rows land on both
    residues mod 16 bytes, outputs are the numpy gather bit for bit inside sentinel-filled buffers, the store inside NaN."""
    import helpers_observations as ho
    from test_gpu_observations import PAD, SENTINEL, _check, _gather, _inputs, _nan_store, _untouched
    from visitron_amd import ops

    slots, views = [2, 0, 1, 0, 2], [0, 13, 35, 7, 24]
    inp = _inputs(3, D, slots, views, [0, 1, 3, 0, 2], seed=D)
    rows_read = {(s * 36 + v) % 2 for s in slots for v in range(36)}
    assert rows_read == {0, 1} and (D * 4) % 16 == 8              # store rows at 0 and at 8 mod 16 bytes are both read
    got, err = _gather(inp, dev)
    assert err == 0
    _check(got, inp)
    # the view gather, output rows tight (both residues) and with an even stride, on bases at 0 and at 8 mod 16 bytes
    store_np = ho.make_store(3, D, 100 + D)
    sbuf, store = _nan_store(store_np, dev)
    vs, vv = [2, 0, 1, 0, 2, 1], [0, 35, 13, 35, 7, 24]
    assert {(s * 36 + v) % 2 for s, v in zip(vs, vv)} == {0, 1}
    rows = torch.tensor(list(zip(vs, vv)), dtype=torch.int32, device=dev)
    want = store_np[vs, vv]
    for shift, ld in ((0, D), (2, D), (2, D + 6)):
        buf = torch.full((2 * PAD + shift + 6 * ld,), SENTINEL, dtype=torch.float32, device=dev)
        out = buf.as_strided((6, D), (ld, 1), PAD + shift)
        e = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.obs_gather_view(store, rows, 6, out=out, err_flag=e)
        torch.cuda.synchronize()
        assert int(e.item()) == 0 and _untouched(sbuf, store_np.size, NAN)
        assert bool((out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()), (shift, ld)
        touched = torch.ones_like(buf, dtype=torch.bool)
        touched.as_strided((6, D), (ld, 1), PAD + shift).fill_(False)
        assert bool((buf[touched] == SENTINEL).all()), (shift, ld)
