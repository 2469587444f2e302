"""GPU: PretrainEngine(..., precision="fp32") -- the reference's fp32 training arithmetic on the fp32 matrix cores -- against
fp64 torch (kernel level) and the CPU oracle's autograd (model level)."""
import os

import numpy as np
import pytest
import torch

import helpers
from helpers import check_close, inject_dropout_masks, model_pair

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4   # relative L2 per parameter, with the absolute floor of _rel (tests/test_gpu_train.py)
LOSS_TOL = 1e-4   # relative, on the four losses


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    floor = 2e-3 * (b.numel() ** 0.5)
    return float((a - b).norm() / (b.norm() + floor))


def _engine(cfg, seed, dev, untie=False, **kw):
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.training import PretrainEngine

    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=seed, device=dev)
    if untie:   # a decoder weight of its own (the word table then gets the embedding gradient only)
        w = ref.mlmhead.predictions.decoder.weight.detach().clone() * 0.5
        ref.mlmhead.predictions.decoder.weight = torch.nn.Parameter(w.clone())
        prod.mlmhead.predictions.decoder.weight = torch.nn.Parameter(w.clone().to(dev))
    prod.train()
    return ref, prod, PretrainEngine(prod, precision="fp32", **kw)


def _check_grads(tag, prod, want, bound=GRAD_TOL):
    errs = {}
    for n, p in prod.named_parameters():
        w = want.get(n)
        if w is None:
            continue
        assert p.grad is not None and p.grad.shape == w.shape, n
        errs[n] = _rel(p.grad, w)
    vals = sorted(errs.values())
    worst = max(errs, key=errs.get)
    helpers._MEASURED.append((tag + " grads worst rel-L2 (" + worst + ")", "rel_l2", errs[worst], bound))
    helpers._MEASURED.append((tag + " grads median rel-L2", "rel_l2", vals[len(vals) // 2], bound))
    print("PARITY %-58s rel_l2  worst %.3e (%s)  median %.3e  bound %.3e" % (tag + " grads", errs[worst], worst,
                                                                              vals[len(vals) // 2], bound))
    bad = {n: e for n, e in errs.items() if e > bound}
    assert not bad, (tag, sorted(bad.items(), key=lambda kv: -kv[1])[:10])


def _same_or_both_nan(a, b, rel):
    a, b = float(a), float(b)
    if np.isnan(b):
        return np.isnan(a)
    return abs(a - b) <= rel * max(1.0, abs(b))


def _check_losses(tag, got, want):
    names = ("loss", "mask_loss", "next_loss", "token_loss", "words_acc", "action_acc", "token_acc")
    for i in range(4):
        w = float(want[i])
        check_close("fp32 %s %s" % (tag, names[i]), float(got[i]), w, LOSS_TOL * max(1.0, abs(w)))
    for i in range(4, 7):
        check_close("fp32 %s %s" % (tag, names[i]), float(got[i]), float(want[i]), 1e-6)


def _ref_grads(ref):
    return {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}


def _dev(b, dev):
    return {k: v.to(dev) for k, v in b.items()}


# ---------------------------------------------------------------------------------------------- kernel level
def test_weight_gradient_gemm_against_fp64(dev):
    from visitron_amd import ops

    g = torch.Generator().manual_seed(1)
    for rows, N, K in ((1000, 77, 130), (5003, 128, 64), (37, 5, 3)):
        dy = torch.randn(rows, N, generator=g)
        x = torch.randn(rows, K, generator=g)
        want_w = dy.double().t() @ x.double()
        want_b = dy.double().sum(0)
        dw = torch.empty(N, K, device=dev)
        db = torch.empty(N, device=dev)
        for split in (1, 0, 3):
            ops.wgrad_f32(dy.to(dev), x.to(dev), dw, db, split=split)
            check_close("fp32 wgrad %dx%dx%d split %d" % (rows, N, K, split), dw.double().cpu(), want_w, 1e-5, kind="rel_l2")
            check_close("fp32 bias grad %dx%d" % (rows, N), db.double().cpu(), want_b, 1e-5, kind="rel_l2")
        ops.wgrad_f32(dy.to(dev), x.to(dev), dw, db, split=1)
        ops.wgrad_f32(dy.to(dev), x.to(dev), dw, db, accumulate=True, split=0)
        check_close("fp32 wgrad accumulate %d" % rows, dw.double().cpu(), 2 * want_w, 1e-5, kind="rel_l2")
    # the split is a fixed-order sum: the same call twice is bitwise equal
    dy, x = torch.randn(20000, 96, generator=g).to(dev), torch.randn(20000, 64, generator=g).to(dev)
    a, b = torch.empty(96, 64, device=dev), torch.empty(96, 64, device=dev)
    ops.wgrad_f32(dy, x, a, split=0)
    ops.wgrad_f32(dy, x, b, split=0)
    assert torch.equal(a, b)
    # batched / strided with the A-transposed operand: dK = dS^T q per (batch, head) on a packed [B*S, 3H] buffer
    B, nh, S = 2, 3, 37
    H = 64 * nh
    ds = torch.randn(B * nh * S, S, generator=g)
    qkv = torch.randn(B * S, 3 * H, generator=g)
    out = torch.zeros(B * S, 3 * H, device=dev)
    ops.gemm_f32_ex(ds.to(dev), qkv.to(dev), S, 64, S, out[:, H:], a_is_km=True, w_is_kn=True, batch=B, heads=nh,
                    strides=((nh * S * S, S * S), (S * 3 * H, 64), (S * 3 * H, 64)))
    q = qkv[:, :H].double().view(B, S, nh, 64).permute(0, 2, 1, 3)
    want = ds.double().view(B, nh, S, S).transpose(-1, -2) @ q
    check_close("fp32 batched dK = dS^T q", out[:, H:2 * H].double().cpu().view(B, S, nh, 64).permute(0, 2, 1, 3), want, 1e-5,
                kind="rel_l2")
    assert float(out[:, :H].abs().max()) == 0 and float(out[:, 2 * H:].abs().max()) == 0


def test_attention_softmax_forward_backward_against_fp64(dev):
    from visitron_amd import ops

    g = torch.Generator().manual_seed(2)
    B, nh, S = 2, 3, 29
    hs = torch.tensor([1.0, 0.0, 0.5])
    for mode, p in ((0, 0.0), (0, 0.2), (2, 0.1), (-1, 0.3)):
        x = torch.randn(B * nh * S, S, generator=g) * 3
        if mode == 0:
            mask = (torch.rand(B, S, generator=g) > 0.3).float()
            add = ((1.0 - mask) * -10000.0).double().view(B, 1, 1, S)
        elif mode == 2:
            raw = (torch.rand(B, S, S, generator=g) > 0.3).float()
            mask = ((1.0 - raw) * -10000.0)
            add = mask.double().view(B, 1, S, S)
        else:
            mask, add = None, 0.0
        seed = 1234 + mode
        keep = torch.stack([ops.attn_dropout_mask(S, (p, seed, ops.site_attn(1)), i, device=dev).cpu()
                            for i in range(B * nh)]).view(B, nh, S, S).double() if p > 0 else 1.0
        pe = ops.attn_drop_p(p)
        xd = x.double().view(B, nh, S, S).requires_grad_(True)
        P = torch.softmax(xd * 0.125 + add, -1)
        Pd = (P * keep / (1.0 - pe)) * hs.double().view(1, nh, 1, 1)
        dy = torch.randn(B, nh, S, S, generator=g).double()
        Pd.backward(dy)
        probs, pd = x.clone().to(dev), torch.empty(B * nh * S, S, device=dev)
        ops.attn_softmax_train_f32(probs, pd, B, nh, S, mask=None if mask is None else mask.to(dev).contiguous(),
                                   mask_mode=mode, head_scale=hs.to(dev), drop=(p, seed, ops.site_attn(1)))
        tag = "fp32 attn softmax mode %d p %.1f" % (mode, p)
        check_close(tag + " P", probs.double().cpu().view(B, nh, S, S), P.detach(), 1e-5, kind="rel_l2")
        check_close(tag + " Pd", pd.double().cpu().view(B, nh, S, S), Pd.detach(), 1e-5, kind="rel_l2")
        d = dy.float().reshape(B * nh * S, S).to(dev).contiguous()
        ops.attn_softmax_train_f32(probs, d, B, nh, S, mask=None if mask is None else mask.to(dev).contiguous(),
                                   mask_mode=mode, head_scale=hs.to(dev), drop=(p, seed, ops.site_attn(1)), backward=True)
        check_close(tag + " dS", d.double().cpu().view(B, nh, S, S), xd.grad, 1e-5, kind="rel_l2")


def test_layernorm_backward_and_embedding_layernorm_backward_against_fp64(dev):
    from visitron_amd import ops

    g = torch.Generator().manual_seed(3)
    for M, H, p in ((300, 128, 0.0), (77, 768, 0.2)):
        x = torch.randn(M, H, generator=g) * 2 + 0.5
        gam, bet = torch.randn(H, generator=g), torch.randn(H, generator=g)
        dy = torch.randn(M, H, generator=g)
        xd = x.double().requires_grad_(True)
        gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
        y = torch.nn.functional.layer_norm(xd, (H,), gd, bd, 1e-12)
        y.backward(dy.double())
        seed, site = 99, ops.site_out(2)
        dx, dxd = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
        dg, db = torch.empty(H, device=dev), torch.empty(H, device=dev)
        ops.layernorm_bwd_f32(x.to(dev), dy.to(dev), gam.to(dev), 1e-12, dg, db, dx=dx, dx_drop=dxd,
                              drop_out=(p, seed, site))
        tag = "fp32 LN bwd %dx%d" % (M, H)
        check_close(tag + " dx", dx.double().cpu(), xd.grad, 1e-5, kind="rel_l2")
        check_close(tag + " dgamma", dg.double().cpu(), gd.grad, 1e-5, kind="rel_l2")
        check_close(tag + " dbeta", db.double().cpu(), bd.grad, 1e-5, kind="rel_l2")
        keep = ops.dropout_mask(M * H, (p, seed, site), device=dev).cpu().view(M, H).double() if p > 0 else 1.0
        check_close(tag + " dx_dropped", dxd.double().cpu(), xd.grad * keep / (1.0 - p), 1e-5, kind="rel_l2")
    # the embedding LayerNorm's backward: gradient rows b*S + t of a padded buffer, the SITE_EMB mask on them first
    B, T, S, H, p = 3, 11, 16, 128, 0.1
    e = torch.randn(B * T, H, generator=g)
    gam = torch.randn(H, generator=g)
    G = torch.randn(B * S, H, generator=g)
    seed = 7
    keep = ops.dropout_mask(B * T * H, (p, seed, ops.SITE_EMB), device=dev).cpu().view(B * T, H).double()
    ed = e.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(ed, (H,), gam.double(), None, 1e-12)
    gy = G.view(B, S, H)[:, :T].reshape(B * T, H).double() * keep / (1.0 - p)
    y.backward(gy)
    de = torch.empty(B * T, H, device=dev)
    dg, db = torch.zeros(H, device=dev), torch.zeros(H, device=dev)
    ops.layernorm_bwd_f32(e.to(dev), G.to(dev), gam.to(dev), 1e-12, dg, db, dx=de, M=B * T, grp_rows=T, grp_stride=S,
                          drop_in=(p, seed, ops.SITE_EMB))
    check_close("fp32 embedding LN bwd de", de.double().cpu(), ed.grad, 1e-5, kind="rel_l2")
    check_close("fp32 embedding LN bwd dbeta", db.double().cpu(), gy.sum(0), 1e-5, kind="rel_l2")


def test_loss_kernels_fp32_gradients_against_fp64(dev):
    from visitron_amd import ops

    g = torch.Generator().manual_seed(4)
    rows, V, C, A, B = 9, 1001, 37, 20, 6
    z = torch.randn(rows, V, generator=g) * 3
    y = torch.randint(0, V, (rows,), generator=g)
    zd = z.double().requires_grad_(True)
    torch.nn.functional.cross_entropy(zd, y, reduction="sum").mul(0.25).backward()
    Vp = (V + 7) // 8 * 8
    zz = torch.zeros(rows, Vp)
    zz[:, :V] = z
    dz = torch.empty(rows, Vp, device=dev)
    loss, amax = ops.ce_softmax_rows_g32(zz.to(dev), y.to(dev), V, dz, 0.25)
    check_close("fp32 CE dz", dz[:, :V].double().cpu(), zd.grad, 1e-5, kind="rel_l2")
    assert float(dz[:, V:].abs().max()) == 0.0
    # token head: softmax then cross entropy's log-softmax
    z = torch.randn(rows, C, generator=g) * 3
    y = torch.randint(0, C, (rows,), generator=g)
    zd = z.double().requires_grad_(True)
    torch.nn.functional.cross_entropy(torch.softmax(zd, -1), y, reduction="sum").mul(0.5).backward()
    Cp = (C + 7) // 8 * 8
    zz = torch.zeros(rows, Cp)
    zz[:, :C] = z
    dz = torch.empty(rows, Cp, device=dev)
    ops.ce_double_softmax_rows_g32(zz.to(dev), y.to(dev), C, dz, 0.5)
    check_close("fp32 double-softmax CE dz", dz[:, :C].double().cpu(), zd.grad, 1e-5, kind="rel_l2")
    # action head: LogSoftmax under CrossEntropy(ignore_index=-1), one target ignored
    z = torch.randn(B, A, generator=g) * 3
    y = torch.randint(0, A, (B,), generator=g)
    y[2] = -1
    zd = z.double().requires_grad_(True)
    torch.nn.functional.cross_entropy(torch.log_softmax(zd, -1), y, ignore_index=-1).mul(1.5).backward()
    Ap = (A + 7) // 8 * 8
    zz = torch.zeros(B, Ap)
    zz[:, :A] = z
    _, _, dl = ops.action_head_g32(zz.to(dev), y.to(dev), A, 1.5, Ap)
    check_close("fp32 action head dz", dl[:, :A].double().cpu(), zd.grad, 1e-5, kind="rel_l2")


# ---------------------------------------------------------------------------------------------- model level
def test_mini_against_oracle_and_reference_fixture(dev):
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    ref, prod, eng = _engine(cfg, 3, dev)
    b = make_batch(cfg, 3, text_len=20, region_len=17, seed=11)
    want = ref(**b)
    want[0].backward()
    got = eng.forward_backward(_dev(b, dev))
    torch.cuda.synchronize()
    assert eng.state_dict()["hyper"]["precision"] == "fp32"
    _check_losses("mini", got, want)
    _check_grads("fp32 mini", prod, _ref_grads(ref))
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mini.npz"))
    for i in range(4):
        w = float(g["tuple7"][i])
        check_close("fp32 mini vs reference fixture tuple7[%d]" % i, float(got[i]), w, LOSS_TOL * max(1.0, abs(w)))
    _check_grads("fp32 mini vs reference fixture", prod,
                 {n: torch.from_numpy(g["grad_%03d" % i]) for i, n in enumerate(list(g["grad_names"]))})


@pytest.mark.parametrize("p_h,p_a,bits", [(0.1, 0.1, 16), (0.3, 0.0, 16), (0.0, 0.25, 16), (0.1, 0.1, 8)])
def test_dropout_against_oracle_with_the_same_masks(dev, p_h, p_a, bits):
    from visitron_amd import ops
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = p_h, p_a
    old = ops.attn_dropout_bits()
    ops.set_attn_dropout_bits(bits)
    try:
        ref, prod, eng = _engine(cfg, 5, dev)
        B, T, R = 3, 20, 17
        b = make_batch(cfg, B, text_len=T, region_len=R, seed=21)
        got = eng.forward_backward(_dev(b, dev))
        torch.cuda.synchronize()
        ref.train()
        inject_dropout_masks(ref, p_h, p_a, eng.last_drop_seed, B, T, R, device=dev, layout=None)
    finally:
        ops.set_attn_dropout_bits(old)
    want = ref(**b)
    want[0].backward()
    tag = "mini dropout(%.2f,%.2f) %d-bit" % (p_h, p_a, bits)
    _check_losses(tag, got, want)
    _check_grads("fp32 " + tag, prod, _ref_grads(ref))


def test_same_masks_as_the_bf16_engine(dev):
    """The fp32 and the bf16 engine (padded rows) with the same seed draw the same dropout: their gradients then differ by
    the bf16 rounding only (mismatched masks would show as errors of order 1)."""
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch
    from visitron_amd.training import PretrainEngine

    cfg = mini_config()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    b = make_batch(cfg, 3, text_len=20, region_len=17, seed=21)
    grads = []
    for precision in ("bf16", "fp32"):
        _, prod = model_pair(OModel, PreTrainOscar, cfg, seed=5, device=dev)
        prod.train()
        eng = PretrainEngine(prod, precision=precision)
        eng.compact_rows = False
        eng.drop_seed_base, eng.fb_count = 0x1234567, 3
        eng.forward_backward(_dev(b, dev))
        torch.cuda.synchronize()
        assert eng.last_drop_seed == 0x1234567 + 3
        grads.append({n: p.grad.detach().clone() for n, p in prod.named_parameters()})
    errs = {n: _rel(grads[0][n], grads[1][n]) for n in grads[1]}
    worst = max(errs, key=errs.get)
    helpers._MEASURED.append(("fp32 vs bf16 padded, same masks, worst rel-L2 (" + worst + ")", "rel_l2", errs[worst], 2e-2))
    assert errs[worst] < 2e-2, sorted(errs.items(), key=lambda kv: -kv[1])[:5]


def test_determinism_and_accumulate(dev):
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    _, prod, eng = _engine(cfg, 6, dev)
    b = _dev(make_batch(cfg, 3, text_len=20, region_len=17, seed=4), dev)
    eng.fb_count = 0
    eng.forward_backward(b)
    s1 = eng.flat.g.clone()
    eng.fb_count = 0
    eng.forward_backward(b)
    assert torch.equal(s1, eng.flat.g)
    b2 = _dev(make_batch(cfg, 3, text_len=20, region_len=17, seed=5), dev)
    eng.fb_count = 1
    eng.forward_backward(b2)
    s2 = eng.flat.g.clone()
    eng.fb_count = 0
    eng.forward_backward(b)
    eng.forward_backward(b2, accumulate=True)   # (fb_count is 1 again: the second call draws b2's masks)
    assert _rel(eng.flat.g, s1 + s2) < 1e-6


def test_edge_cases(dev):
    """No MLM row (NaN loss, zeroed head gradients), no region-token row, partially ignored actions, one sequence."""
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    ref, prod, eng = _engine(cfg, 31, dev)
    b = make_batch(cfg, 4, text_len=12, region_len=6, seed=2)
    cases = []
    c = {k: v.clone() for k, v in b.items()}
    c["labels"].fill_(-1)
    cases.append(("no_mlm", c))
    c = {k: v.clone() for k, v in b.items()}
    c["token_labels"].fill_(-1)
    cases.append(("no_tok", c))
    c = {k: v.clone() for k, v in b.items()}
    c["next_action"][1] = -1
    c["next_action"][3] = -1
    cases.append(("part_act", c))
    one = make_batch(cfg, 1, text_len=9, region_len=3, seed=5)
    one["labels"].fill_(-1)
    one["labels"][0, 4] = int(one["input_ids"][0, 4])
    cases.append(("single", one))
    for name, c in cases:
        ref.zero_grad()
        eng.flat.g.fill_(7.0)   # stale values that a zeroing step must clear
        want = ref(**c)
        got = eng.forward_backward(_dev(c, dev))
        torch.cuda.synchronize()
        for i in range(7):
            assert _same_or_both_nan(got[i], want[i], LOSS_TOL), (name, i, float(got[i]), float(want[i]))
        if name == "no_mlm":
            pr = prod.mlmhead.predictions
            for p in (pr.transform.dense.weight, pr.transform.dense.bias, pr.transform.LayerNorm.weight, pr.bias):
                assert float(p.grad.abs().max()) == 0.0
            continue
        want[0].backward()
        _check_grads("fp32 mini edge " + name, prod, _ref_grads(ref))


def test_head_mask_3d_mask_img_layernorm_untied_decoder(dev):
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    cfg.use_img_layernorm, cfg.img_layer_norm_eps = 1, 1e-12
    cfg.hidden_dropout_prob = 0.1
    ref, prod, eng = _engine(cfg, 9, dev, untie=True)
    assert prod.mlmhead.predictions.decoder.weight is not prod.bert.embeddings.word_embeddings.weight
    B, T, R = 3, 14, 9
    S = T + R
    b = make_batch(cfg, B, text_len=T, region_len=R, seed=31)
    m2 = b["attention_mask"].float()
    m3 = m2[:, None, :].repeat(1, S, 1)
    m3[:, :, 3] = 0.0
    m3[1, 5, :] = 1.0
    b["attention_mask"] = m3
    L, nh = cfg.num_hidden_layers, cfg.num_attention_heads
    hm = torch.ones(L, nh)
    hm[0, 1] = 0.0
    hm[-1, 0] = 0.5
    got = eng.forward_backward(_dev(b, dev), head_mask=hm.to(dev))
    torch.cuda.synchronize()
    ref.train()
    inject_dropout_masks(ref, 0.1, 0.0, eng.last_drop_seed, B, T, R, device=dev, layout=None)
    want = ref(**b, head_mask=hm)
    want[0].backward()
    _check_losses("head_mask + 3-D mask + img-LN + untied", got, want)
    _check_grads("fp32 head_mask + 3-D mask + img-LN + untied", prod, _ref_grads(ref))


def test_training_tracks_the_oracle_loop(dev):
    from oracle.optim import AdamW, grouped_parameters
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    ref, prod, eng = _engine(cfg, 8, dev, lr=1e-3, weight_decay=0.05, schedule="constant", warmup_steps=0)
    opt = AdamW(grouped_parameters(ref, 0.05), lr=1e-3, eps=1e-8)
    b = make_batch(cfg, 4, text_len=16, region_len=8, seed=2)
    bd = _dev(b, dev)
    lr_, lh = [], []
    for _ in range(6):
        ref.zero_grad()
        out = ref(**b)
        out[0].backward()
        opt.step()
        lr_.append(float(out[0]))
        lh.append(float(eng.train_step(bd)[0]))
    err = max(abs(a - c) for a, c in zip(lr_, lh))
    check_close("fp32 six train_steps vs oracle AdamW loop, worst loss", err, 0.0, 1e-3)
    assert lh[-1] < lh[0] - 0.5


def test_trunk_engine_against_oracle_trunk(dev):
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch
    from visitron_amd.training import PretrainEngine

    cfg = mini_config()
    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=12, device=dev)
    eng = PretrainEngine(prod.bert, precision="fp32")
    b = make_batch(cfg, 2, text_len=10, region_len=5, seed=3)
    keys = ("input_ids", "token_type_ids", "attention_mask", "position_ids", "img_feats", "img_location_embeddings")
    tb = {k: b[k] for k in keys if k in b}
    with pytest.raises(NotImplementedError):
        eng.trunk_forward(_dev(tb, dev), training=False, want_hidden=True)
    seq, pooled, st = eng.trunk_forward(_dev(tb, dev), training=False)
    ref.eval()
    rs, rp = ref.bert(**tb)[:2]
    g = torch.Generator().manual_seed(0)
    d_seq, d_pool = torch.randn(rs.shape, generator=g), torch.randn(rp.shape, generator=g)
    (rs * d_seq).sum().add_((rp * d_pool).sum()).backward()
    eng.trunk_backward(st, d_seq.to(dev), d_pool.to(dev))
    torch.cuda.synchronize()
    check_close("fp32 trunk sequence_output", seq.cpu(), rs.detach(), 1e-4)
    check_close("fp32 trunk pooled_output", pooled.cpu(), rp.detach(), 1e-4)
    _check_grads("fp32 trunk", prod.bert, {n: p.grad for n, p in ref.bert.named_parameters() if p.grad is not None})


def test_base_cfg0_against_reference_fixture_and_oracle(dev):
    """BASELINE configs[0] (12 layers, 30 522 words, B = 2, 128 + 100): the reference's own tuple and gradient slices / norms
    (tests/golden/ref_base_cfg0.npz), and the oracle's autograd on whole tensors."""
    from test_gpu_train import _check_grad_slices
    from visitron_amd.config import BertConfig
    from visitron_amd.synth import make_batch

    cfg = BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    from oracle.modeling import PreTrainOscar as OModel
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.training import PretrainEngine

    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=0, device=dev, weight_std=0.03)
    prod.train()
    eng = PretrainEngine(prod, precision="fp32")
    b = make_batch(cfg, 2, seed=1234)
    got = eng.forward_backward(_dev(b, dev))
    torch.cuda.synchronize()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_base_cfg0.npz"))
    for i in range(4):
        w = float(g["tuple7"][i])
        check_close("fp32 base cfg0 vs reference fixture tuple7[%d]" % i, float(got[i]), w, LOSS_TOL * max(1.0, abs(w)))
    _check_grad_slices("fp32 base cfg0 vs reference fixture", prod, g, bound=GRAD_TOL)
    want = ref(**b)
    want[0].backward()
    _check_losses("base cfg0", got, want)
    _check_grads("fp32 base cfg0", prod, _ref_grads(ref))
