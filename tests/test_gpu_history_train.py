"""GPU: encoder_history_states in trunk-level training (visitron_amd/training.py on csrc/attention_rect.hip) against torch autograd on
the CPU oracle, at mini_config size: outputs, every parameter gradient and the gradients of the history tensors themselves; the
per-query mask together with a history in inference; and the combinations that are refused."""
import pytest
import torch

from helpers import check_close, maxabs, model_pair
from test_gpu_rollout_train import _grads_close

pytestmark = pytest.mark.gpu
B, T = 3, 12
GRAD_TOL = 2e-2   # tests/test_gpu_rollout_train.py: what its gradient check applies to the trunk


def _pair(dev, seed=17, **cfg_kw):
    from oracle.modeling import BertImgModelwithLocationEmbeds as OTrunk
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import BertImgModelwithLocationEmbeds

    cfg = mini_config(**cfg_kw)
    ref, prod = model_pair(OTrunk, BertImgModelwithLocationEmbeds, cfg, seed=seed, device=dev)
    return cfg, ref.train(), prod.train()


def _inputs(cfg, Sh, seed=3, per_query=False):
    """ids [B, T]; one history tensor per layer [B, Sh, H]; a mask over the Sh + T keys with a padded tail and one masked history
    key -- [B, Sh+T], or per query [B, T, Sh+T] (the new positions causal among themselves); weights of the scalar loss."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g)
    hist = [torch.randn(B, Sh, cfg.hidden_size, generator=g) for _ in range(cfg.num_hidden_layers)]
    mask = torch.ones(B, Sh + T)
    mask[1, Sh + 8:] = 0
    mask[2, Sh + 5:] = 0
    mask[0, 2] = 0
    if per_query:
        m3 = mask[:, None, :].expand(B, T, Sh + T).clone()
        m3[:, :, Sh:] *= torch.tril(torch.ones(T, T))
        mask = m3
    ws, wp = torch.randn(B, T, cfg.hidden_size, generator=g), torch.randn(B, cfg.hidden_size, generator=g)
    return ids, hist, mask, ws, wp


def _history_grads_close(tag, got, want):
    for l, (gh, wh) in enumerate(zip(got, want)):
        assert gh is not None, (tag, l)
        check_close("%s d_history[%d] rel-L2" % (tag, l), gh, wh, GRAD_TOL, kind="rel_l2")


@pytest.mark.parametrize("Sh", (5, 40))
def test_training_forward_and_backward_with_history_match_oracle(dev, Sh):
    cfg, ref, prod = _pair(dev)
    ids, hist, mask, ws, wp = _inputs(cfg, Sh)
    hr = [h.clone().requires_grad_(True) for h in hist]
    want = ref(ids, attention_mask=mask, encoder_history_states=hr)
    ((want[0] * ws).sum() + (want[1] * wp).sum()).backward()
    hp = [h.to(dev).requires_grad_(True) for h in hist]
    got = prod(ids.to(dev), attention_mask=mask.to(dev), encoder_history_states=hp)
    assert got[0].requires_grad and got[0].shape == (B, T, cfg.hidden_size)
    check_close("history train Sh=%d sequence_output" % Sh, got[0], want[0], 5e-2)
    check_close("history train Sh=%d pooled_output" % Sh, got[1], want[1], 5e-2)
    ((got[0] * ws.to(dev)).sum() + (got[1] * wp.to(dev)).sum()).backward()
    _grads_close("history train Sh=%d" % Sh, prod, ref, GRAD_TOL)
    _history_grads_close("history train Sh=%d" % Sh, [h.grad for h in hp], [h.grad for h in hr])
    assert float(hp[0].grad[0, 2].abs().max()) <= 1e-3 * float(hp[0].grad[0].abs().max())   # the masked history key


def test_engine_leaves_d_history_only_for_tensors_that_require_grad(dev):
    from visitron_amd.training import _bridge_engine

    cfg, ref, prod = _pair(dev)
    ids, hist, mask, ws, wp = _inputs(cfg, 5)
    batch = dict(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    hp = [h.to(dev) for h in hist]
    hp[1].requires_grad_(True)
    eng = _bridge_engine(prod)
    seq, pooled, st = eng.trunk_forward(batch, history=hp)
    eng.trunk_backward(st, ws.to(dev), wp.to(dev))
    assert st.d_history[0] is None and st.d_history[1].shape == hp[1].shape and st.d_history[1].dtype == torch.float32
    grads = {n: eng.flat.view(eng.flat.g, "bert." + n).clone() for n, _ in prod.named_parameters()}
    # no history tensor requires grad: identical results, nothing kept
    seq2, pooled2, st2 = eng.trunk_forward(batch, history=[h.to(dev) for h in hist])
    eng.trunk_backward(st2, ws.to(dev), wp.to(dev))
    assert st2.d_history == [None] * cfg.num_hidden_layers
    assert torch.equal(seq, seq2) and torch.equal(pooled, pooled2)
    for n, g in grads.items():
        assert torch.equal(g, eng.flat.view(eng.flat.g, "bert." + n)), n
    # ... and against the oracle
    hr = [h.clone().requires_grad_(True) for h in hist]
    want = ref(ids, attention_mask=mask, encoder_history_states=hr)
    ((want[0] * ws).sum() + (want[1] * wp).sum()).backward()
    _history_grads_close("engine d_history", [st.d_history[1]], [hr[1].grad])
    # a forward without a history afterwards reaches none of it
    _, _, st3 = eng.trunk_forward(dict(input_ids=ids.to(dev), attention_mask=mask[:, 5:].to(dev)))
    assert st3.hist is None and st3.d_history is None


def test_head_mask_and_hidden_states_with_history(dev):
    cfg, ref, prod = _pair(dev, output_hidden_states=True, output_attentions=True)
    Sh = 5
    ids, hist, mask, ws, wp = _inputs(cfg, Sh, per_query=True)
    head_mask = torch.tensor([[1.0, 0.5], [0.0, 1.5]])
    g = torch.Generator().manual_seed(9)
    wh = [torch.randn(B, T, cfg.hidden_size, generator=g) * 0.3 for _ in range(cfg.num_hidden_layers + 1)]
    hr = [h.clone().requires_grad_(True) for h in hist]
    want = ref(ids, attention_mask=mask, head_mask=head_mask, encoder_history_states=hr)
    ((want[0] * ws).sum() + (want[1] * wp).sum() + sum((h * w).sum() for h, w in zip(want[2], wh))).backward()
    hp = [h.to(dev).requires_grad_(True) for h in hist]
    got = prod(ids.to(dev), attention_mask=mask.to(dev), head_mask=head_mask.to(dev), encoder_history_states=hp)
    assert len(got) == len(want) == 4
    check_close("history train head_mask sequence_output", got[0], want[0], 5e-2)
    for l, (hg, hw) in enumerate(zip(got[2], want[2])):
        assert hg.shape == hw.shape
        check_close("history train head_mask hidden[%d]" % l, hg, hw, 5e-2)
    for pg, pw in zip(got[3], want[3]):
        assert pg.shape == pw.shape == (B, cfg.num_attention_heads, T, Sh + T) and not pg.requires_grad
        assert maxabs(pg, pw) < 2e-2
    ((got[0] * ws.to(dev)).sum() + (got[1] * wp.to(dev)).sum() + sum((h * w.to(dev)).sum() for h, w in zip(got[2], wh))).backward()
    _grads_close("history train head_mask + hidden states", prod, ref, GRAD_TOL)
    _history_grads_close("history train head_mask", [h.grad for h in hp], [h.grad for h in hr])


def test_dropout_with_history_is_a_function_of_the_seed(dev):
    from visitron_amd import ops
    from visitron_amd.training import _bridge_engine

    cfg, ref, prod = _pair(dev, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    ids, hist, mask, ws, wp = _inputs(cfg, 40)
    batch = dict(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    eng = _bridge_engine(prod)

    def run(seed):
        eng.drop_seed_base, eng.fb_count = seed, 0
        hp = [h.to(dev).requires_grad_(True) for h in hist]
        out = eng.trunk_forward(batch, training=True, history=hp, want_attn=True)
        seq, pooled, st, attn = out[0], out[1], out[2], out[4]
        eng.trunk_backward(st, ws.to(dev), wp.to(dev))
        grads = [eng.flat.view(eng.flat.g, "bert." + n).clone() for n, _ in prod.named_parameters()]
        return [seq.clone(), pooled.clone()] + [a.clone() for a in attn] + grads + [d.clone() for d in st.d_history]

    a, b, c = run(1234), run(1234), run(99)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0])
    assert all(bool(torch.isfinite(x).all()) for x in a + c)
    pe = ops.attn_drop_p(0.1)
    probs = a[2]   # layer 0 after dropout: zeros where dropped, rows that sum to about 1 / (1 - p) times the kept share
    frac = float((probs[0, :, :, :] == 0).float().mean())
    assert 0.02 < frac < 0.25, frac
    assert float(probs.sum(-1).mean()) == pytest.approx(1.0, abs=0.1) and pe > 0


def test_inference_with_a_per_query_mask_and_history_matches_oracle(dev):
    cfg, ref, prod = _pair(dev, output_attentions=True)
    ref.eval()
    prod.eval()
    Sh = 11
    ids, hist, mask, _, _ = _inputs(cfg, Sh, per_query=True)
    with torch.no_grad():
        want = ref(ids, attention_mask=mask, encoder_history_states=hist)
        got = prod(ids.to(dev), attention_mask=mask.to(dev), encoder_history_states=[h.to(dev) for h in hist])
    check_close("history + per-query mask sequence_output", got[0], want[0], 5e-2)
    check_close("history + per-query mask pooled_output", got[1], want[1], 5e-2)
    for pg, pw in zip(got[2], want[2]):
        assert pg.shape == pw.shape == (B, cfg.num_attention_heads, T, Sh + T) and maxabs(pg, pw) < 2e-2


def test_refusals(dev):
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import make_batch
    from visitron_amd.training import PretrainEngine, _bridge_engine, autograd_trunk_forward

    cfg, ref, prod = _pair(dev)
    ids, hist, mask, _, _ = _inputs(cfg, 5)
    hp = [h.to(dev) for h in hist]
    batch = dict(input_ids=ids.to(dev), attention_mask=mask.to(dev))
    with pytest.raises(NotImplementedError, match="row compaction"):
        autograd_trunk_forward(prod, batch, unmasked_only=True, history=hp)
    eng = _bridge_engine(prod)
    with pytest.raises(NotImplementedError, match="chunked data-parallel"):
        eng._trunk_fwd(batch, None, None, None, True, False, comm=dict(layers_per_chunk=1), history=hp)
    with pytest.raises(NotImplementedError, match="fp32"):
        PretrainEngine(PreTrainOscar(cfg).to(dev), precision="fp32").trunk_forward(batch, history=hp)
    with pytest.raises(RuntimeError, match="one tensor per layer"):
        eng.trunk_forward(batch, history=hp[:1])
    b = make_batch(cfg, B, text_len=T, region_len=4, seed=4, with_labels=False)
    with pytest.raises(AssertionError, match="image features"):
        prod(ids.to(dev), attention_mask=mask.to(dev), img_feats=b["img_feats"].to(dev),
             img_location_embeddings=b["img_location_embeddings"].to(dev), encoder_history_states=hp)
