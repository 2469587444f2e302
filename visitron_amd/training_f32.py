"""The fp32 training step of ``PretrainEngine(model, precision="fp32")``: the reference's own training arithmetic.

The reference trains in fp32 (tasks/viewpoint_select/pretrain.py:191 back-propagates fp32; no AMP anywhere).  Here every
operand, activation, gradient and accumulator is fp32 and every product runs on the fp32 matrix cores
(``ops.gemm_f32_ex``: the forward GEMMs, the dgrad GEMMs, the weight gradients with the A-transposed operand and a
fixed-order K split over the token rows, the attention's four batched products).  The row work is HIP as well
(csrc/fp32_train.hip): the attention softmax with its dropout and its backward, the LayerNorm backward, GELU', the
embedding sum and the loss kernels' fp32 gradients.  No float atomics: two steps with the same seed write bitwise-equal
gradient slabs.

The step runs on the padded [B*S, H] rows (no row compaction), with the reference's literal mask arithmetic
(1 - m) * -10000, and draws the bf16 engine's dropout decisions on that layout: the seed is drop_seed_base + fb_count, the
sites are ops.SITE_EMB / SITE_IMG / site_attn / site_selfout / site_out, and the element indices are those of the bf16
kernels (tests/helpers.py, inject_dropout_masks(..., layout=None)).  An fp32 engine built over the same parameters with the
same seed is therefore an on-device reference for the bf16 engine's gradients at any shape (tools/grad_drift.py).

Served: forward_backward (2-D / 3-D masks, head_mask, use_img_layernorm, tied or untied decoder, batches without a
supervised row), train_step / optimizer_step (the same fused AdamW over the fp32 slab), trunk_forward / trunk_backward in
their plain form.  Not served: several ranks, row compaction, intermediate hidden states / attentions of the trunk.
"""
import torch

from . import ops, training
from .modeling import _head_scale, _i64
from .ops import ACT_GELU, ACT_TANH, round_up

F32 = torch.float32


def setup(eng):
    """The padded head widths the fp32 loss kernels write (rows 16-byte aligned, widths a multiple of 8)."""
    m = eng.model
    if eng.has_heads:
        eng.Vp = round_up(m.mlmhead.predictions.decoder.weight.shape[0], 8)
        eng.Cp = round_up(m.token_head[0].weight.shape[0], 8)
        eng.Ap = round_up(m.next_action.linear.weight.shape[0], 8)


def _d(p):
    return p.detach()


def _linear(x, w, bias=None, out=None, M=None, N=None, lda=None, ldc=None, **kw):
    """out = x . w^T (+ bias ...) with w = nn.Linear.weight [N, K]."""
    M = x.shape[0] if M is None else M
    N = w.shape[0] if N is None else N
    if out is None:
        out = torch.empty((M, N), dtype=F32, device=x.device)
    return ops.gemm_f32_ex(x, w, M, N, w.shape[1], out, lda=lda, ldc=ldc, bias=bias, **kw)


def _dgrad(dy, w, K=None, lda=None, residual=None):
    """dy [M, N] . w [N, K]: the gradient of the input of x . w^T."""
    N, Kw = w.shape
    out = torch.empty((dy.shape[0], Kw), dtype=F32, device=dy.device)
    return ops.gemm_f32_ex(dy, w, dy.shape[0], Kw, N if K is None else K, out, lda=lda, w_is_kn=True, residual=residual)


def _layer_params(eng, l):
    """(parameters, gradients) of encoder layer l as {field: fp32 view} (training._LAYER_FIELDS, the packed projection)."""
    f = eng.flat
    return training._layer_views(f, l, f.p, f.p), training._layer_views(f, l, f.g, f.g)


def trunk_forward(eng, batch, head_mask, is_training):
    """Embeddings, region projection, encoder layers and pooler in fp32, every activation the backward reads kept."""
    m, cfg = eng.model, eng.cfg
    eng._require_ownership()
    eng.flat.reattach_grads()
    ids = _i64(batch["input_ids"])
    dev = ids.device
    B, T = ids.shape
    if batch.get("img_packed") is not None:
        raise NotImplementedError("PretrainEngine(precision='fp32') does not take img_packed (a bf16 operand): build the batch "
                                  "with RegionStore(..., dtype=torch.float32).pretrain_batch(..., packed=False)")
    img = batch.get("img_feats")
    R = 0 if img is None else img.shape[1]
    S, H, nh, L = T + R, cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers
    M = B * S
    am = batch.get("attention_mask")
    mask, mode = None, -1
    if am is not None:
        mask = am.to(F32).contiguous()
        if mask.dim() == 3:   # the reference's per-query mask (encoder.py:228-229) -> its additive bias, same arithmetic
            if mask.shape != (B, S, S):
                raise RuntimeError("3-D attention_mask must be [batch, text+region, text+region]")
            mask, mode = ((1.0 - mask) * -10000.0).contiguous(), 2
        elif mask.shape != (B, S):
            raise RuntimeError("attention_mask must be [batch, text+region]")
        else:
            mode = 0          # (1 - m) * -10000 inside the softmax kernel (encoder.py:238-241)
    hs = _head_scale(head_mask, L, nh, dev)
    tt, pos_ids = _i64(batch.get("token_type_ids")), _i64(batch.get("position_ids"))
    p_h = float(cfg.hidden_dropout_prob) if is_training else 0.0
    p_a = float(cfg.attention_probs_dropout_prob) if is_training else 0.0
    seed = (eng.drop_seed_base + eng.fb_count) & 0xFFFFFFFFFFFFFFFF
    eng.fb_count += 1
    eng.last_drop_seed = seed
    eng.last_rows, eng.last_layout = M, None

    emb = m.bert.embeddings
    eps = emb.LayerNorm.variance_epsilon
    x0 = torch.empty((M, H), dtype=F32, device=dev)
    e = torch.empty((B * T, H), dtype=F32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.embed_sum_f32(ids, tt, pos_ids, _d(emb.word_embeddings.weight), _d(emb.position_embeddings.weight),
                      _d(emb.token_type_embeddings.weight), e, err_flag=err)
    if int(err.item()) != 0:
        raise IndexError("index out of range in BertEmbeddings (input_ids / position_ids / token_type_ids)")
    ops.layernorm_drop_f32(e, _d(emb.LayerNorm.weight), _d(emb.LayerNorm.bias), eps, x0, M=B * T, grp_rows=T, grp_stride=S,
                           drop=(p_h, seed, ops.SITE_EMB))
    a_img = img_pre = None
    if img is not None:
        # img_embedding(img_feats) + location_embeds(loc) (encoder.py:277-279) as one product over the K-concatenated
        # operands (as the fp32 inference path), LayerNorm (optional) and dropout, into rows b*S + T + r
        bt = m.bert
        a_img = torch.cat([img.reshape(B * R, -1).float(), batch["img_location_embeddings"].reshape(B * R, -1).float()],
                          1).contiguous()
        w = torch.cat([_d(bt.img_embedding.weight), _d(bt.location_embeds.weight)], 1).contiguous()
        b = _d(bt.img_embedding.bias) + _d(bt.location_embeds.bias)
        if getattr(bt, "use_img_layernorm", None):
            img_pre = _linear(a_img, w, b)
            ops.layernorm_drop_f32(img_pre, _d(bt.LayerNorm.weight), _d(bt.LayerNorm.bias), bt.LayerNorm.variance_epsilon,
                                   x0[T:], M=B * R, grp_rows=R, grp_stride=S, drop=(p_h, seed, ops.SITE_IMG))
        else:
            _linear(a_img, w, b, out=x0[T:], M=B * R, ldc=H, grp_rows=R, grp_stride=S, drop=(p_h, seed, ops.SITE_IMG))

    layers, cur = [], x0
    for l in range(L):
        w, _ = _layer_params(eng, l)
        a = dict(x=cur)
        a["qkv"] = qkv = _linear(cur, w["w_qkv"], w["b_qkv"])
        ld = 3 * H
        probs = torch.empty((B * nh * S, S), dtype=F32, device=dev)
        ops.gemm_f32_ex(qkv, qkv[:, H:], S, S, 64, probs, batch=B, heads=nh,
                        strides=((S * ld, 64), (S * ld, 64), (nh * S * S, S * S)))
        pd = torch.empty_like(probs)
        ops.attn_softmax_train_f32(probs, pd, B, nh, S, mask=mask, mask_mode=mode,
                                   head_scale=None if hs is None else hs[l].contiguous(), drop=(p_a, seed, ops.site_attn(l)))
        ctx = torch.empty((M, H), dtype=F32, device=dev)
        ops.gemm_f32_ex(pd, qkv[:, 2 * H:], S, 64, S, ctx, w_is_kn=True, batch=B, heads=nh,
                        strides=((nh * S * S, S * S), (S * ld, 64), (S * H, 64)))
        a.update(probs=probs, pd=pd, ctx=ctx)
        a["attn_pre"] = _linear(ctx, w["w_ao"], w["b_ao"], residual=cur, drop=(p_h, seed, ops.site_selfout(l)))
        a["attn_out"] = ops.layernorm_rows(a["attn_pre"], w["ln1_g"], w["ln1_b"], cfg.layer_norm_eps)
        a["mid_pre"] = torch.empty((M, w["w_in"].shape[0]), dtype=F32, device=dev)
        a["mid"] = _linear(a["attn_out"], w["w_in"], w["b_in"], act=ACT_GELU, pre_act=a["mid_pre"])
        a["out_pre"] = _linear(a["mid"], w["w_out"], w["b_out"], residual=a["attn_out"], drop=(p_h, seed, ops.site_out(l)))
        cur = ops.layernorm_rows(a["out_pre"], w["ln2_g"], w["ln2_b"], cfg.layer_norm_eps)
        layers.append(a)
    pool = m.bert.pooler.dense
    pooled = _linear(cur, _d(pool.weight), _d(pool.bias), M=B, lda=S * H, act=ACT_TANH)
    eng._fwd_serial += 1
    return training.TrunkState(B=B, T=T, R=R, S=S, H=H, nh=nh, L=L, M=M, dev=dev, serial=eng._fwd_serial, mask=mask, mode=mode,
                               hs=hs, p_h=p_h, p_a=p_a, seed=seed, ids=ids, tt=tt, pos_ids=pos_ids, img=img, a_img=a_img,
                               img_pre=img_pre, e=e, x0=x0, layers=layers, seq=cur, pooled=pooled)


def pooler_backward(eng, st, g, d_pooled, acc):
    """dL/d(pooled) [B, H] -> the pooler's gradients and its rows' share of g (dL/d(sequence output) [M, H])."""
    pool = eng.model.bert.pooler.dense
    B, S, H = st.B, st.S, st.H
    g_z = (d_pooled * (1.0 - st.pooled * st.pooled)).contiguous()   # tanh' on [B, H]
    ops.gemm_f32_ex(g_z, st.seq, H, H, B, eng._grad(pool.weight), ldw=S * H, a_is_km=True, w_is_kn=True, accumulate=acc)
    ops.colsum_f32(g_z, eng._grad(pool.bias), accumulate=acc)
    g.view(B, S, H)[:, 0].add_(_dgrad(g_z, _d(pool.weight)))


def trunk_backward(eng, st, g, acc, word_grad_ready=False):
    """Back through the encoder layers, the embeddings and the region projection; g fp32 [M, H] = dL/d(sequence output)
    (overwritten).  The gradients land in the flat slab."""
    if st.serial != eng._fwd_serial:
        raise RuntimeError("the activations of this forward were overwritten by a later forward of the same engine; "
                           "run backward before the next forward")
    m, cfg = eng.model, eng.cfg
    B, T, R, S, H, nh, M = st.B, st.T, st.R, st.S, st.H, st.nh, st.M
    p_h, p_a, seed, eps = st.p_h, st.p_a, st.seed, cfg.layer_norm_eps
    dev = g.device
    for l in range(st.L - 1, -1, -1):
        w, gr = _layer_params(eng, l)
        a = st.layers[l]
        d_out_pre = torch.empty((M, H), dtype=F32, device=dev)
        d_dense = torch.empty((M, H), dtype=F32, device=dev)
        ops.layernorm_bwd_f32(a["out_pre"], g, w["ln2_g"], eps, gr["ln2_g"], gr["ln2_b"], dx=d_out_pre, dx_drop=d_dense,
                              accumulate=acc, drop_out=(p_h, seed, ops.site_out(l)))
        ops.wgrad_f32(d_dense, a["mid"], gr["w_out"], gr["b_out"], accumulate=acc)
        g_mid = ops.dgelu_f32(_dgrad(d_dense, w["w_out"]), a["mid_pre"])
        ops.wgrad_f32(g_mid, a["attn_out"], gr["w_in"], gr["b_in"], accumulate=acc)
        g_attn_out = _dgrad(g_mid, w["w_in"], residual=d_out_pre)
        d_attn_pre = torch.empty((M, H), dtype=F32, device=dev)
        d_ao = torch.empty((M, H), dtype=F32, device=dev)
        ops.layernorm_bwd_f32(a["attn_pre"], g_attn_out, w["ln1_g"], eps, gr["ln1_g"], gr["ln1_b"], dx=d_attn_pre,
                              dx_drop=d_ao, accumulate=acc, drop_out=(p_h, seed, ops.site_selfout(l)))
        ops.wgrad_f32(d_ao, a["ctx"], gr["w_ao"], gr["b_ao"], accumulate=acc)
        g_ctx = _dgrad(d_ao, w["w_ao"])
        # attention (oscar/modeling_bert.py:47-72): dPd = dC v^T, dV = Pd^T dC, dS = softmax' (row kernel), dQ = dS k, dK = dS^T q
        qkv, ld = a["qkv"], 3 * H
        dqkv = torch.empty((M, 3 * H), dtype=F32, device=dev)
        dp = torch.empty_like(a["probs"])
        sq, sp, sc = (S * ld, 64), (nh * S * S, S * S), (S * H, 64)
        ops.gemm_f32_ex(g_ctx, qkv[:, 2 * H:], S, S, 64, dp, batch=B, heads=nh, strides=(sc, sq, sp))
        ops.gemm_f32_ex(a["pd"], g_ctx, S, 64, S, dqkv[:, 2 * H:], a_is_km=True, w_is_kn=True, batch=B, heads=nh,
                        strides=(sp, sc, sq))
        ops.attn_softmax_train_f32(a["probs"], dp, B, nh, S, mask=st.mask, mask_mode=st.mode,
                                   head_scale=None if st.hs is None else st.hs[l].contiguous(),
                                   drop=(p_a, seed, ops.site_attn(l)), backward=True)
        ops.gemm_f32_ex(dp, qkv[:, H:], S, 64, S, dqkv, w_is_kn=True, batch=B, heads=nh, strides=(sp, sq, sq))
        ops.gemm_f32_ex(dp, qkv, S, 64, S, dqkv[:, H:], a_is_km=True, w_is_kn=True, batch=B, heads=nh, strides=(sp, sq, sq))
        ops.wgrad_f32(dqkv, a["x"], gr["w_qkv"], gr["b_qkv"], accumulate=acc)
        g = _dgrad(dqkv, w["w_qkv"], residual=d_attn_pre)

    emb = m.bert.embeddings
    word_grad = eng._grad(emb.word_embeddings.weight)
    pos_grad, type_grad = eng._grad(emb.position_embeddings.weight), eng._grad(emb.token_type_embeddings.weight)
    if not acc:
        if not word_grad_ready:
            word_grad.zero_()
        pos_grad.zero_()
        type_grad.zero_()
    de = torch.empty((B * T, H), dtype=F32, device=dev)
    ops.layernorm_bwd_f32(st.e, g, _d(emb.LayerNorm.weight), emb.LayerNorm.variance_epsilon, eng._grad(emb.LayerNorm.weight),
                          eng._grad(emb.LayerNorm.bias), dx=de, accumulate=acc, M=B * T, grp_rows=T, grp_stride=S,
                          drop_in=(p_h, seed, ops.SITE_EMB))
    # the three tables without float atomics (sorted ids, one workgroup per run); the default position / type ids spelled out
    ops.embed_table_grad(st.ids.reshape(-1), de, word_grad, skip_id=emb.word_embeddings.padding_idx)
    pos = st.pos_ids if st.pos_ids is not None else torch.arange(T, device=dev).repeat(B)
    ops.embed_table_grad(pos.reshape(-1), de, pos_grad)
    typ = st.tt if st.tt is not None else torch.zeros(B * T, dtype=torch.int64, device=dev)
    ops.embed_table_grad(typ.reshape(-1), de, type_grad)

    bt = m.bert
    if st.img is None:
        if not acc:
            eng._zero_head_grads("region")
        return
    d_img = torch.empty((B * R, H), dtype=F32, device=dev)
    if st.img_pre is not None:
        ops.layernorm_bwd_f32(st.img_pre, g[T:], _d(bt.LayerNorm.weight), bt.LayerNorm.variance_epsilon,
                              eng._grad(bt.LayerNorm.weight), eng._grad(bt.LayerNorm.bias), dx=d_img, accumulate=acc, M=B * R,
                              grp_rows=R, grp_stride=S, drop_in=(p_h, seed, ops.SITE_IMG))
    else:
        ops.dropout_rows_f32(g[T:], d_img, B * R, grp_rows=R, grp_stride=S, drop=(p_h, seed, ops.SITE_IMG))
    D = bt.img_dim
    ops.gemm_f32_ex(d_img, st.a_img, H, D, B * R, eng._grad(bt.img_embedding.weight), a_is_km=True, w_is_kn=True,
                    accumulate=acc, split=0)
    ops.gemm_f32_ex(d_img, st.a_img[:, D:], H, st.a_img.shape[1] - D, B * R, eng._grad(bt.location_embeds.weight),
                    a_is_km=True, w_is_kn=True, accumulate=acc, split=0)
    ops.colsum_f32(d_img, eng._grad(bt.img_embedding.bias), accumulate=acc)
    ops.colsum_f32(d_img, eng._grad(bt.location_embeds.bias), accumulate=acc)


def forward_backward(eng, batch, grad_scale, accumulate, head_mask, backward):
    """PretrainEngine.forward_backward in fp32: the reference's 7-tuple; gradients of grad_scale * loss in the flat slab."""
    m, cfg = eng.model, eng.cfg
    st = trunk_forward(eng, batch, head_mask, m.training)
    dev, B, S, H, M = st.dev, st.B, st.S, st.H, st.M
    seq = st.seq
    V, C, A = cfg.vocab_size, cfg.detector_classes, cfg.action_space
    pr = m.mlmhead.predictions
    gs = float(grad_scale)
    lab, tl = _i64(batch["labels"]).reshape(-1), _i64(batch["token_labels"]).reshape(-1)
    idx_w = torch.nonzero(lab != -1).reshape(-1)
    idx_t = torch.nonzero(tl != -1).reshape(-1)
    Ml, Mt = int(idx_w.numel()), int(idx_t.numel())
    zero = torch.zeros((), dtype=F32, device=dev)
    if Ml > 0:   # the MLM head on its supervised rows (encoder.py:377-389)
        seq_w = seq.index_select(0, idx_w)
        y_w = lab.index_select(0, idx_w)
        h_pre = torch.empty((Ml, H), dtype=F32, device=dev)
        t1 = _linear(seq_w, _d(pr.transform.dense.weight), _d(pr.transform.dense.bias), act=ACT_GELU, pre_act=h_pre)
        t2 = ops.layernorm_rows(t1, _d(pr.transform.LayerNorm.weight), _d(pr.transform.LayerNorm.bias),
                                pr.transform.LayerNorm.variance_epsilon)
        logits = torch.empty((Ml, eng.Vp), dtype=F32, device=dev)
        _linear(t2, _d(pr.decoder.weight), _d(pr.bias), out=logits, N=V)
        dl = torch.empty((Ml, eng.Vp), dtype=F32, device=dev)
        loss_rows, amax_w = ops.ce_softmax_rows_g32(logits, y_w, V, dl, gs / Ml)
        mask_loss = loss_rows.mean()
        words_acc = (amax_w == y_w).sum().float() / Ml
    else:
        mask_loss = words_acc = zero / zero   # CrossEntropyLoss over no valid target is nan, as in the reference
    lin_tok = m.token_head[0]
    if Mt > 0:   # token head: Linear + Softmax under a second log-softmax (encoder.py:323-326, 380-385)
        seq_t = seq.index_select(0, idx_t)
        y_t = tl.index_select(0, idx_t)
        lt = torch.empty((Mt, eng.Cp), dtype=F32, device=dev)
        _linear(seq_t, _d(lin_tok.weight), _d(lin_tok.bias), out=lt, N=C)
        dlt = torch.empty((Mt, eng.Cp), dtype=F32, device=dev)
        tok_rows, amax_t = ops.ce_double_softmax_rows_g32(lt, y_t, C, dlt, gs / Mt)
        token_loss = tok_rows.mean()
        token_acc = (amax_t == y_t).sum().float() / Mt
    else:
        token_loss = token_acc = zero / zero
    la = torch.empty((B, eng.Ap), dtype=F32, device=dev)
    _linear(st.pooled, _d(m.next_action.linear.weight), _d(m.next_action.linear.bias), out=la, N=A)
    next_action = batch.get("next_action")
    dla = None
    if next_action is not None:
        next_loss, action_acc, dla = ops.action_head_g32(la, _i64(next_action), A, gs, eng.Ap)
    else:
        next_loss, action_acc = 0, 0
    loss = mask_loss + next_loss + token_loss
    out = (loss, mask_loss, next_loss, token_loss, words_acc, action_acc, token_acc)
    if not backward:
        return out

    acc = bool(accumulate)
    emb = m.bert.embeddings
    g = torch.zeros((M, H), dtype=F32, device=dev)
    dec_tied = eng._decoder_tied()
    if not acc:
        eng._grad(emb.word_embeddings.weight).zero_()   # the tied decoder accumulates into it; the tables add to it later
    if Ml > 0:
        if not acc:
            eng._grad(pr.bias).zero_()                  # shares the accumulate flag of the decoder weight below
        ops.wgrad_f32(dl[:, :V], t2, eng._grad(pr.decoder.weight), eng._grad(pr.bias), accumulate=acc or dec_tied)
        g_t2 = _dgrad(dl, _d(pr.decoder.weight), K=V)
        g_t1 = torch.empty((Ml, H), dtype=F32, device=dev)
        ops.layernorm_bwd_f32(t1, g_t2, _d(pr.transform.LayerNorm.weight), pr.transform.LayerNorm.variance_epsilon,
                              eng._grad(pr.transform.LayerNorm.weight), eng._grad(pr.transform.LayerNorm.bias), dx=g_t1,
                              accumulate=acc)
        g_h = ops.dgelu_f32(g_t1, h_pre)
        ops.wgrad_f32(g_h, seq_w, eng._grad(pr.transform.dense.weight), eng._grad(pr.transform.dense.bias), accumulate=acc)
        g.index_add_(0, idx_w, _dgrad(g_h, _d(pr.transform.dense.weight)))
    elif not acc:
        eng._zero_head_grads("mlm")   # no supervised MLM row (the loss is NaN, as the reference's): zero gradients
    if Mt > 0:
        ops.wgrad_f32(dlt[:, :C], seq_t, eng._grad(lin_tok.weight), eng._grad(lin_tok.bias), accumulate=acc)
        g.index_add_(0, idx_t, _dgrad(dlt, _d(lin_tok.weight), K=C))
    elif not acc:
        eng._zero_head_grads("token")
    if dla is not None:
        ops.wgrad_f32(dla[:, :A], st.pooled, eng._grad(m.next_action.linear.weight), eng._grad(m.next_action.linear.bias),
                      accumulate=acc)
        pooler_backward(eng, st, g, _dgrad(dla, _d(m.next_action.linear.weight), K=A), acc)
    elif not acc:
        eng._zero_head_grads("action", "pooler")
    trunk_backward(eng, st, g, acc, word_grad_ready=True)
    return out
