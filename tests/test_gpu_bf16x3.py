"""GPU: the "bf16x3" precision -- the fp32 route with every matrix product formed on the bf16 matrix cores from two bf16
terms per fp32 operand (csrc/bf16x3_path.hip).  The GEMM is pinned to the emulated arithmetic (A) and to fp64 within the
derived bound (B) of tests/helpers_bf16x3.py; the model-level tests are those of tests/test_gpu_fp32.py under "bf16x3":
outputs within 1e-3 of the reference's fp32 CPU forward (BASELINE north_star)."""
import os

import numpy as np
import pytest
import torch

import helpers_bf16x3 as hx
from helpers import check_close, model_pair, same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-3
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRUNK_KEYS = ("input_ids", "attention_mask", "img_feats", "img_location_embeddings")


def _to(b, dev):
    return {k: v.to(dev) for k, v in b.items()}


def _run(dev, a, w, b, r, act, kn, alpha=hx.ALPHA):
    from visitron_amd import ops

    got = ops.linear_f32(a.to(dev), w.to(dev), None if b is None else b.to(dev), residual=None if r is None else r.to(dev),
                         act=act, w_is_kn=kn, alpha=alpha, products="bf16x3")
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("M,N,K,act,res,kn", hx.GEMM_CASES)
def test_linear_bf16x3_matches_emulation_and_fp64(dev, M, N, K, act, res, kn):
    a, w, b, r = hx.gemm_inputs(M, N, K, res, kn)
    got = _run(dev, a, w, b, r, act, kn)
    assert got.shape == (M, N)
    hx.check_gemm("linear_bf16x3 M%d N%d K%d act%d kn%d" % (M, N, K, act, kn), got, a, w.t().contiguous() if kn else w, b, r,
                  act, hx.ALPHA)


def test_linear_bf16x3_unaligned_operands_take_the_scalar_loads(dev):
    """Bases 4 bytes off a 16-byte boundary and odd row strides: the scalar-load path of both operand forms."""
    from visitron_amd import ops

    g = torch.Generator().manual_seed(11)
    M, N, K = 70, 45, 67
    a_buf, w_buf, kn_buf = torch.randn(M, K + 2, generator=g), torch.randn(N, K + 2, generator=g) * 0.05, torch.randn(K, N + 2, generator=g) * 0.05
    a_d, w_d, kn_d = a_buf.to(dev)[:, 1:K + 1], w_buf.to(dev)[:, 1:K + 1], kn_buf.to(dev)[:, 1:N + 1]
    got = ops.linear_f32(a_d, w_d, None, products="bf16x3")
    hx.check_gemm("linear_bf16x3 unaligned [N,K]", got, a_buf[:, 1:K + 1], w_buf[:, 1:K + 1])
    got = ops.linear_f32(a_d, kn_d, None, w_is_kn=True, products="bf16x3")
    hx.check_gemm("linear_bf16x3 unaligned [K,N]", got, a_buf[:, 1:K + 1], kn_buf[:, 1:N + 1].t().contiguous())


def test_exact_constructions_are_bit_for_bit(dev):
    """A = I with an asymmetric 16-bit W gives W^T (a row/column swap or a dropped hi.lo shows); W = I with such an A gives A
    (a dropped lo.hi shows); integers in +-4095 (which need lo) times integers in +-3 give the integer product."""
    eye = torch.eye(96)
    w = hx.sixteen_bit_values((80, 96), 5)
    got = _run(dev, eye, w, None, None, 0, False, alpha=1.0)
    assert torch.equal(got.cpu(), w.t()), float((got.cpu() - w.t()).abs().max())
    got = _run(dev, eye, w.t().contiguous(), None, None, 0, True, alpha=1.0)      # the same W given as [K, N]
    assert torch.equal(got.cpu(), w.t())
    a = hx.sixteen_bit_values((70, 96), 6)
    got = _run(dev, a, eye, None, None, 0, False, alpha=1.0)
    assert torch.equal(got.cpu(), a), float((got.cpu() - a).abs().max())
    g = torch.Generator().manual_seed(7)
    ai = torch.randint(-4095, 4096, (150, 64), generator=g).float()
    ai[0, :4] = torch.tensor([4095.0, -4095.0, 4095.0, 257.0])
    wi = torch.randint(-3, 4, (131, 64), generator=g).float()
    want = (ai.double() @ wi.double().t()).float()
    got = _run(dev, ai, wi, None, None, 0, False, alpha=1.0)
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    got = _run(dev, ai, wi.t().contiguous(), None, None, 0, True, alpha=1.0)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("sa,sw", [(40, -40), (-40, 40)])
def test_scaled_operands_stay_finite_and_inside_the_bound(dev, sa, sw):
    M, N, K, act, res, kn = hx.GEMM_CASES[1]
    assert (M, N, K) == (77, 768, 768)
    a, w, b, r = hx.gemm_inputs(M, N, K, res, kn)
    a, w = a * 2.0 ** sa, w * 2.0 ** sw
    got = _run(dev, a, w, b, r, act, kn)
    assert bool(torch.isfinite(got).all())
    ra, rb = hx.gemm_ratios(got, a, w, b, r, act, hx.ALPHA)
    check_close("linear_bf16x3 A*2^%d W*2^%d (B) / bound" % (sa, sw), rb, 0.0, 1.0)


def test_linear_bf16x3_row_remap_and_strided_input(dev):
    from visitron_amd import ops

    g = torch.Generator().manual_seed(3)
    B, R, S, H, K = 3, 5, 12, 64, 70
    a = torch.randn(B * R, K, generator=g)
    w = torch.randn(H, K, generator=g) * 0.1
    out = torch.zeros(B * S, H, device=dev)
    ops.linear_f32(a.to(dev), w.to(dev), None, out=out[7:], ldc=H, grp_rows=R, grp_stride=S, products="bf16x3")
    got = out.view(B, S, H).cpu()
    assert not bool(got[:, :7].any()), "rows outside the remap were written"
    hx.check_gemm("linear_bf16x3 row remap", got[:, 7:].reshape(B * R, H), a, w)
    # token 0 of every sequence through the row stride (the pooler's read)
    seq = torch.randn(B * S, H, generator=g)
    got = ops.linear_f32(seq.to(dev), w[:, :H].contiguous().to(dev), None, act=2, M=B, lda=S * H, products="bf16x3")
    hx.check_gemm("linear_bf16x3 strided rows", got, seq.view(B, S, H)[:, 0].contiguous(), w[:, :H].contiguous(), act=2)


@pytest.mark.parametrize("S,mode", [(37, "raw"), (228, "raw"), (300, "additive"), (45, "per_query"), (64, "none")])
def test_attention_bf16x3_within_the_derived_bounds(dev, S, mode):
    """The inputs of test_attention_f32_matches_reference_arithmetic; both products on bf16x3, the softmax unchanged."""
    from visitron_amd import ops

    g = torch.Generator().manual_seed(S)
    B, nh = 2, 3
    H = nh * 64
    qkv = torch.randn(B * S, 3 * H, generator=g)
    keep = (torch.rand(B, S, generator=g) > 0.3).float()
    keep[:, 0] = 1
    hm = torch.tensor([1.0, 0.0, 0.5])
    if mode == "raw":
        mask, add, ext = keep, False, ((1.0 - keep) * -10000.0)[:, None, None, :]
    elif mode == "additive":
        bias = (1.0 - keep) * -10000.0
        mask, add, ext = bias, True, bias[:, None, None, :]
    elif mode == "per_query":
        m3 = (torch.rand(B, S, S, generator=g) > 0.3).float()
        m3[:, :, 0] = 1
        bias = (1.0 - m3) * -10000.0
        mask, add, ext = bias, True, bias[:, None]
    else:
        mask, add, ext = None, False, 0.0
    pr, want, dp, dc = hx.attention_reference(qkv, B, S, nh, ext, hm)
    ctx, probs = ops.attention_f32(qkv.to(dev), B, S, nh, mask=None if mask is None else mask.contiguous().to(dev),
                                   mask_additive=add, head_scale=hm.to(dev), want_probs=True, products="bf16x3")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(probs).all())
    check_close("attention_bf16x3 S=%d %s probs max error" % (S, mode), probs, pr.float(), float(dp.max()))
    check_close("attention_bf16x3 S=%d %s ctx max error" % (S, mode), ctx, want.float(), float(dc.max()))
    check_close("attention_bf16x3 S=%d %s probs / bound" % (S, mode), float(((probs.cpu().double() - pr).abs() / dp).max()), 0.0, 1.0)
    check_close("attention_bf16x3 S=%d %s ctx / bound" % (S, mode), float(((ctx.cpu().double() - want).abs() / dc).max()), 0.0, 1.0)


def test_bf16x3_mode_mini_model_and_golden(dev):
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd import set_precision
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict, make_batch

    cfg = mini_config(use_img_layernorm=True, img_layer_norm_eps=1e-12, output_hidden_states=True)
    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=6, device=dev)
    set_precision(prod, "bf16x3")
    b = make_batch(cfg, 5, text_len=24, region_len=11, seed=3)
    with torch.no_grad():
        want = ref(**b)
        got = prod(**_to(b, dev))
        w_tr = ref.bert(**{k: b[k] for k in TRUNK_KEYS})
        g_tr = prod.bert(**{k: b[k].to(dev) for k in TRUNK_KEYS})
    for i in range(4):
        check_close("bf16x3 mini tuple7[%d]" % i, float(got[i]), float(want[i]), TOL)
    for i in range(4, 7):
        check_close("bf16x3 mini tuple7[%d]" % i, float(got[i]), float(want[i]), 1e-6)
    check_close("bf16x3 mini sequence_output", g_tr[0], w_tr[0], TOL)
    check_close("bf16x3 mini pooled_output", g_tr[1], w_tr[1], TOL)
    assert len(g_tr[2]) == len(w_tr[2]) == cfg.num_hidden_layers + 1
    for i, (a, c) in enumerate(zip(g_tr[2], w_tr[2])):
        check_close("bf16x3 mini hidden[%d]" % i, a, c, TOL)
    # golden fixture: the REFERENCE's own outputs (tests/golden/make_golden_from_reference.py), no oracle call
    g = np.load(os.path.join(GOLD, "ref_mini.npz"))
    m = PreTrainOscar(mini_config()).eval()
    m.load_state_dict(deterministic_state_dict(m, seed=3, weight_std=0.05))
    m.tie_weights()
    m = set_precision(m.to(dev), "bf16x3")
    gb = {k: torch.from_numpy(g["in_" + k]).to(dev) for k in TRUNK_KEYS}
    with torch.no_grad():
        outs, pooled, _, B, S = m.bert.run_trunk(gb["input_ids"], attention_mask=gb["attention_mask"], img_feats=gb["img_feats"],
                                                 img_location_embeddings=gb["img_location_embeddings"])
        scores, tokp, act = m.head_outputs(outs[-1], pooled)
    check_close("bf16x3 golden mini sequence_output", outs[-1], g["sequence_output"], TOL)
    check_close("bf16x3 golden mini prediction_scores", scores, g["prediction_scores"], TOL)
    check_close("bf16x3 golden mini token_probs", tokp, g["token_probs"], TOL)
    check_close("bf16x3 golden mini action_scores", act, g["action_scores"], TOL)


def _base_outputs(ref, prod, b, dev, cfg):
    with torch.no_grad():
        w_seq, w_pool = ref.bert(**{k: b[k] for k in TRUNK_KEYS})[:2]
        g_seq, g_pool = prod.bert(**{k: b[k].to(dev) for k in TRUNK_KEYS})[:2]
        w_heads = ref.heads(w_seq, w_pool)
        g_heads = prod.head_outputs(g_seq.reshape(-1, cfg.hidden_size), g_pool)
    return (w_seq, w_pool) + tuple(w_heads), (g_seq, g_pool) + tuple(g_heads)


def test_bf16x3_mode_base_config_cfg0_within_1e_3(dev):
    """BASELINE configs[0] (the inputs of the fp32 test) against the CPU fp32 oracle and the reference's own fixture; and
    against the "fp32" mode of the same module."""
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd import set_precision
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch

    cfg = BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=0, device=dev, weight_std=0.03)
    set_precision(prod, "bf16x3")
    b = make_batch(cfg, 2, seed=1234)
    with torch.no_grad():
        want = ref(**b)
        got = prod(**_to(b, dev))
    (w_seq, w_pool, w_scores, w_tok, w_act), (g_seq, g_pool, g_scores, g_tok, g_act) = _base_outputs(ref, prod, b, dev, cfg)
    check_close("bf16x3 base cfg0 sequence_output", g_seq, w_seq, TOL)
    check_close("bf16x3 base cfg0 pooled_output", g_pool, w_pool, TOL)
    check_close("bf16x3 base cfg0 prediction_scores", g_scores, w_scores, TOL)
    check_close("bf16x3 base cfg0 token_probs", g_tok, w_tok, TOL)
    check_close("bf16x3 base cfg0 action_scores", g_act, w_act, TOL)
    for i in range(4):
        check_close("bf16x3 base cfg0 tuple7[%d]" % i, float(got[i]), float(want[i]), TOL)
    g = np.load(os.path.join(GOLD, "ref_base_cfg0.npz"))
    check_close("bf16x3 golden base cfg1 sequence_output slice", g_seq.cpu()[:, ::19, ::31], g["sequence_output_slice"], TOL)
    check_close("bf16x3 golden base cfg1 prediction_scores slice", g_scores.cpu().view(2, 228, -1)[:, ::19, ::1009],
                g["prediction_scores_slice"], TOL)
    check_close("bf16x3 golden base cfg1 action_scores", g_act, g["action_scores"], TOL)
    set_precision(prod, "fp32")
    with torch.no_grad():
        f_seq = prod.bert(**{k: b[k].to(dev) for k in TRUNK_KEYS})[0]
    check_close("bf16x3 base cfg0 sequence_output against the fp32 mode", g_seq, f_seq, TOL)


def test_bf16x3_mode_base_config_harsher_weights_within_1e_3(dev):
    """weight_std 0.05, seed 3, batch seed 7: the CPU emulation of this arithmetic measures 1.9e-4 on prediction_scores."""
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd import set_precision
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch

    cfg = BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=3, device=dev, weight_std=0.05)
    set_precision(prod, "bf16x3")
    b = make_batch(cfg, 2, seed=7)
    (w_seq, w_pool, w_scores, w_tok, w_act), (g_seq, g_pool, g_scores, g_tok, g_act) = _base_outputs(ref, prod, b, dev, cfg)
    check_close("bf16x3 base harsh sequence_output", g_seq, w_seq, TOL)
    check_close("bf16x3 base harsh pooled_output", g_pool, w_pool, TOL)
    check_close("bf16x3 base harsh prediction_scores", g_scores, w_scores, TOL)
    check_close("bf16x3 base harsh token_probs", g_tok, w_tok, TOL)
    check_close("bf16x3 base harsh action_scores", g_act, w_act, TOL)


def test_bf16x3_mode_rollout_caller_text_only_with_history_and_head_mask(dev):
    """The text-only call of the rollout caller (agent_models.py:270-275), history states and head_mask under bf16x3."""
    from oracle.modeling import BertImgModelwithLocationEmbeds as OTrunk
    from visitron_amd import set_precision
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import BertImgModelwithLocationEmbeds

    cfg = mini_config(output_attentions=True)
    ref, prod = model_pair(OTrunk, BertImgModelwithLocationEmbeds, cfg, seed=5, device=dev)
    set_precision(prod, "bf16x3")
    g = torch.Generator().manual_seed(2)
    B, T, Sh = 3, 14, 6
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g)
    pad = torch.zeros(B, T, dtype=torch.uint8)
    pad[1, 9:] = 1
    hm = torch.tensor([[1.0, 0.5], [0.0, 1.0]])
    with torch.no_grad():
        want = ref(ids, attention_mask=~pad, head_mask=hm)       # the uint8 ~mask quirk: values 255 / 254
        got = prod(ids.to(dev), attention_mask=(~pad).to(dev), head_mask=hm.to(dev))
    check_close("bf16x3 text-only uint8-mask sequence_output", got[0], want[0], TOL)
    for i, (a, c) in enumerate(zip(got[2], want[2])):
        check_close("bf16x3 text-only attentions[%d]" % i, a, c, 1e-4)
    hist = [torch.randn(B, Sh, cfg.hidden_size, generator=g) for _ in range(cfg.num_hidden_layers)]
    m = torch.ones(B, Sh + T)
    m[2, 3] = 0
    with torch.no_grad():
        want = ref(ids, attention_mask=m, encoder_history_states=hist)
        got = prod(ids.to(dev), attention_mask=m.to(dev), encoder_history_states=[h.to(dev) for h in hist])
    check_close("bf16x3 history sequence_output", got[0], want[0], TOL)


def test_bf16x3_refuses_training_and_leaves_bf16_untouched(dev):
    from visitron_amd import set_precision
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict, make_batch
    from visitron_amd.training import PretrainEngine

    cfg = mini_config()
    b = _to(make_batch(cfg, 3, text_len=20, region_len=9, seed=4), dev)

    def build():
        m = PreTrainOscar(cfg).eval()
        m.load_state_dict(deterministic_state_dict(m, seed=2, weight_std=0.05))
        m.tie_weights()
        return m.to(dev)

    plain, m = build(), build()
    set_precision(m, "bf16x3")
    m.train()
    with pytest.raises(NotImplementedError, match="bf16x3"):
        m(**b)                                   # with grad, train(): served by neither fp32-route mode
    m.eval()
    with pytest.raises(ValueError, match="'bf16' or 'fp32'"):
        PretrainEngine(m, precision="bf16x3")
    with torch.no_grad():
        x3 = [t.clone() for t in m(**b)]
    set_precision(m, "bf16")
    with torch.no_grad():
        back, want = m(**b), plain(**b)
    assert same_bits(back, want), "set_precision(m, 'bf16') after 'bf16x3' is not the default path"
    assert not same_bits(x3, want)               # (and bf16x3 was a different arithmetic)
