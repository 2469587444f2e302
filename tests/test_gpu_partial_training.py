"""GPU: PretrainEngine honours requires_grad.

  1. frozen means frozen: after three train_steps a frozen parameter holds its initial bits, its moments are zero and its
     .grad is None -- for a frozen word table, a frozen bottom (embedding block + region group + layers 0-1), a frozen layer
     between trainable ones, everything frozen but the action head, and a mixed unit (layer 2's biases);
  2. same gradients: the trainable parameters' gradients are bit-identical to the all-trainable engine's at the same seed and
     batch (the same kernels see the same operands) -- from forward_backward on the default path (the C loop), with the
     weight gradients on the side stream (a frozen layer records no event there), with the backward chunked one layer at a time through train_step's single-process hook, on the unrolled path, and through the autograd
     bridge (loss.backward() on PreTrainOscar, the trunk node under OscarEncoder);
  3. census: on the unrolled path the backward's launch counts (weight gradients, full and dx-only LayerNorm backwards -- a
     reduce launch rides behind every full one and behind no other --, attention backwards, dgrad GEMMs) are the numbers the
     contract gives for the pattern; for the all-trainable model they are the counts before requires_grad was read;
  4. gradual unfreezing: layer 0 frozen for two steps, trainable for two more -- weights and moments follow oracle/optim.py's
     rule (per-parameter step counts, as torch's state["step"]) fed the engine's own gradients, within the bound
     tests/test_gpu_train.py::test_adamw_step_matches_oracle holds ops.adamw_flat to; a state saved after step 3 and loaded into
     a fresh engine gives step 4 bit for bit;
  5. the refusals raise with their sentence.
mini_config(num_hidden_layers=3), B = 2, T = 12, R = 4, both dropouts 0.1, ops.set_deterministic(True); every case on padded rows
with a mask and on compacted rows (text lengths 12 and 7).  Alone: python -m pytest tests/test_gpu_partial_training.py -q -s"""
import pytest
import torch

pytestmark = pytest.mark.gpu

L, B, T, R = 3, 2, 12, 4
TEXT_LENS, REGION_LENS = (12, 7), (4, 3)
SEED = 4321
LAYOUTS = ["padded", "compacted"]

EMB, REGION = "bert.embeddings.", ("bert.img_embedding.", "bert.location_embeds.")
PATTERNS = {
    "word table": lambda n: n == "bert.embeddings.word_embeddings.weight",
    "bottom": lambda n: n.startswith((EMB,) + REGION + ("bert.encoder.layer.0.", "bert.encoder.layer.1.")),
    "layer 1": lambda n: n.startswith("bert.encoder.layer.1."),
    "action head only": lambda n: not n.startswith("next_action."),
    "layer 2 biases": lambda n: n.startswith("bert.encoder.layer.2.") and n.endswith(".bias"),
}
NONE_FROZEN = lambda n: False


@pytest.fixture()
def det():
    from visitron_amd import ops

    ops.set_deterministic(True)
    try:
        yield ops
    finally:
        ops.set_deterministic(False)


def _cfg():
    from visitron_amd.config import mini_config

    return mini_config(num_hidden_layers=L, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)


def _batch(dev):
    """Two sequences of 12 text + 4 region positions, the second with 7 real tokens and 3 real regions: a 0/1 mask, every
    supervised position a real one (what the compacted layout asks for), all three heads supervised."""
    from visitron_amd.synth import make_batch

    cfg = _cfg()
    b = make_batch(cfg, B, text_len=T, region_len=R, seed=17)
    mask = torch.zeros(B, T + R, dtype=torch.int64)
    for i in range(B):
        mask[i, :TEXT_LENS[i]] = 1
        mask[i, T:T + REGION_LENS[i]] = 1
    real = mask.bool()
    ids = torch.randint(5, cfg.vocab_size, (B, T), generator=torch.Generator().manual_seed(3))
    ids[:, 0] = 101
    b["input_ids"] = torch.where(real[:, :T], ids, torch.zeros_like(ids))
    labels = torch.full((B, T + R), -1, dtype=torch.int64)
    tl = torch.full((B, T + R), -1, dtype=torch.int64)
    for i, t in ((0, 3), (0, 9), (1, 2), (1, 5)):
        labels[i, t] = b["input_ids"][i, t]
    for i, t in ((0, 4), (1, 6)):
        tl[i, t] = (3 * t + i) % cfg.detector_classes
    b.update(attention_mask=mask, labels=labels, token_labels=tl)
    b["img_feats"] = b["img_feats"] * real[:, T:, None]
    b["img_location_embeddings"] = b["img_location_embeddings"] * real[:, T:, None]
    return {k: v.to(dev) for k, v in b.items()}


def _model(dev, frozen):
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict

    m = PreTrainOscar(_cfg())
    m.load_state_dict(deterministic_state_dict(m, seed=5))
    m.tie_weights()
    m = m.to(dev).train()
    for n, p in m.named_parameters():
        p.requires_grad = not frozen(n)
    return m


def _engine(dev, frozen, layout, **kw):
    """A fresh model and engine; the dropout seeds follow torch's seed, so equal seeds give equal masks."""
    from visitron_amd.training import PretrainEngine

    torch.manual_seed(SEED)
    m = _model(dev, frozen)
    kw.setdefault("lr", 1e-3)
    eng = PretrainEngine(m, schedule="constant", **kw)
    eng.compact_rows = layout == "compacted"
    return m, eng


def _checked_layout(eng, layout):
    assert (eng.last_layout is not None) == (layout == "compacted")
    if layout == "compacted":
        assert eng.last_rows == sum(TEXT_LENS) + sum(REGION_LENS)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


_reference = {}


def _all_trainable(dev, layout, path):
    """The all-trainable engine's gradients (and, on the unrolled path, its launch census) of one forward_backward: computed
    once per (layout, path) and shared."""
    key = (layout, path)
    if key not in _reference:
        m, eng = _engine(dev, NONE_FROZEN, layout)
        grads, census = _run(eng, m, dev, layout, path)
        _reference[key] = (grads, census)
    return _reference[key]


def _run(eng, m, dev, layout, path):
    """One forward_backward on `path` -> ({name: gradient clone, trainable parameters only}, backward census or None)."""
    from visitron_amd import ops

    batch = _batch(dev)
    census = None
    if path == "c loop":
        eng.forward_backward(batch)
    elif path == "side stream":
        eng.overlap_wgrad = True   # weight gradients on the side stream: a frozen layer records no event there
        eng.forward_backward(batch)
    elif path == "chunked":
        eng.lr = 0.0   # train_step with the hook steps AdamW too: nothing moves, the gradients stay in the slab
        eng.wd = 0.0
        launched = []
        eng.train_step(batch, layers_per_chunk=1, _force_comm=launched.extend)
        assert _disjoint(launched)
        frozen = [eng.flat.span[n] for n, p, _, _, _ in eng.flat.entries if not p.requires_grad]
        assert all(e_ <= a_ or s_ >= b_ for s_, e_ in launched for a_, b_ in frozen), "a frozen range went to the communicator"
        covered = sum(e_ - s_ for s_, e_ in launched)
        assert covered == sum(e_ - s_ for s_, e_ in eng.train_spans)
    else:
        # the unrolled path (what runs under ops.profile_begin): the forward alone first, then forward + backward -- the
        # difference of the two censuses is the backward's
        ops.profile_begin()
        eng.forward_backward(batch, backward=False)
        fwd = ops.profile_end()
        ops.profile_begin()
        eng.forward_backward(batch)
        both = ops.profile_end()
        census = {k: both[k]["n"] - fwd.get(k, {"n": 0})["n"] for k in both}
    torch.cuda.synchronize()
    _checked_layout(eng, layout)
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}
    return grads, census


def _assert_copies_fresh(eng):
    """Every transposed copy the dgrad GEMMs read is the transpose of its source in the mirror, and the mirror is bf16(p):
    refresh_derived_weights rebuilds only what a step moved, and must miss nothing."""
    eng.refresh_derived_weights()
    torch.cuda.synchronize()
    f = eng.flat
    assert torch.equal(f.mirror.view(torch.int16), f.p.to(torch.bfloat16).view(torch.int16))
    for l, lv in enumerate(eng._layers):
        for k, dst in lv.wt.items():
            src = lv.t["w_" + k[3:]]
            assert torch.equal(dst.view(torch.int16), src.t().contiguous().view(torch.int16)), (l, k)
    for _, prm, key in eng._head_rows():
        if key:
            src = eng._mirror(prm)
            assert torch.equal(eng.head_t[key][:, :src.shape[0]].contiguous().view(torch.int16),
                               src.t().contiguous().view(torch.int16)), key


def _disjoint(ranges):
    rs = sorted(ranges)
    return all(a[1] <= b[0] for a, b in zip(rs, rs[1:]))


# ---- 1. frozen means frozen -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_frozen_means_frozen(dev, det, pattern, layout):
    frozen = PATTERNS[pattern]
    m, eng = _engine(dev, frozen, layout)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    mirror0 = eng.flat.mirror.clone()
    batch = _batch(dev)
    for _ in range(3):
        eng.train_step(batch)
    torch.cuda.synchronize()
    _checked_layout(eng, layout)
    moved = 0
    for n, p in m.named_parameters():
        if frozen(n):
            assert torch.equal(_bits(p), _bits(before[n])), "%s: a frozen parameter moved" % n
            assert not bool(eng.flat.view(eng.flat.m, n).any()) and not bool(eng.flat.view(eng.flat.v, n).any()), n
            assert p.grad is None, n
            o, cnt, _ = eng.flat.off[n]
            assert torch.equal(eng.flat.mirror[o:o + cnt].view(torch.int16), mirror0[o:o + cnt].view(torch.int16)), n
            assert eng.param_steps[n] == 0
        else:
            assert p.grad is not None and p.grad.data_ptr() == eng.flat.view(eng.flat.g, n).data_ptr(), n
            assert eng.param_steps[n] == 3
            moved += int(not torch.equal(p.detach(), before[n]))
    n_train = sum(1 for n, _ in m.named_parameters() if not frozen(n))
    assert moved == n_train, "%d of %d trainable parameters moved" % (moved, n_train)
    _assert_copies_fresh(eng)
    # frozen after a step, before the next forward: what that step moved is still rebuilt
    for p in m.parameters():
        p.requires_grad = False
    m.next_action.linear.bias.requires_grad = True
    eng.train_step(batch)
    _assert_copies_fresh(eng)


# ---- 2. same gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("path", ["c loop", "side stream", "chunked", "unrolled"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_trainable_gradients_are_the_all_trainable_engines_bits(dev, det, pattern, path, layout):
    frozen = PATTERNS[pattern]
    want, _ = _all_trainable(dev, layout, "unrolled" if path == "unrolled" else "c loop")
    m, eng = _engine(dev, frozen, layout)
    got, _ = _run(eng, m, dev, layout, path)
    assert sorted(got) == sorted(n for n in want if not frozen(n))
    for n, g in got.items():
        assert bool(g.abs().sum() > 0), "%s: no gradient at all" % n
        assert torch.equal(_bits(g), _bits(want[n])), "%s: %d elements differ" % (n, int((_bits(g) != _bits(want[n])).sum()))
    assert all(p.grad is None for n, p in m.named_parameters() if frozen(n))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_bridge_loss_backward_gives_the_same_gradients(dev, det, pattern, layout):
    """loss.backward() on the drop-in PreTrainOscar (the engine behind the bridge is the model's own)."""
    from visitron_amd.training import _bridge_engine

    def grads(frozen):
        torch.manual_seed(SEED)
        m = _model(dev, frozen)
        eng = _bridge_engine(m)
        eng.compact_rows = layout == "compacted"
        m(**_batch(dev))[0].backward()
        torch.cuda.synchronize()
        _checked_layout(eng, layout)
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}, eng

    key = (layout, "bridge")
    if key not in _reference:
        _reference[key] = grads(NONE_FROZEN)[0]
    want, frozen = _reference[key], PATTERNS[pattern]
    got, eng = grads(frozen)
    for n in want:
        if frozen(n):
            assert got[n] is None, n
        else:
            assert torch.equal(_bits(got[n]), _bits(want[n])), n
    assert eng.units["layers"] == [any(n.startswith("bert.encoder.layer.%d." % l) and not frozen(n) for n in want)
                                   for l in range(L)]


TRUNK_PATTERNS = [p for p in PATTERNS if p != "action head only"]   # (a fully frozen trunk takes the inference path)


@pytest.mark.parametrize("compact", [False, True], ids=LAYOUTS)
@pytest.mark.parametrize("pattern", TRUNK_PATTERNS)
def test_trunk_node_under_oscar_encoder_gives_the_same_gradients(dev, det, pattern, compact):
    from visitron_amd.rollout import OscarEncoder
    from visitron_amd.training import _bridge_engine

    ids = torch.randint(5, _cfg().vocab_size, (B, T), generator=torch.Generator().manual_seed(8))
    pad = torch.zeros(B, T, dtype=torch.bool)
    for i, n in enumerate(TEXT_LENS):
        pad[i, n:] = True
        ids[i, n:] = 0
    weight = torch.randn(B, T, 128, generator=torch.Generator().manual_seed(9)).to(dev)

    def grads(frozen):
        torch.manual_seed(SEED)
        trunk = _model(dev, lambda n: False).bert
        for n, p in trunk.named_parameters():
            p.requires_grad = not frozen("bert." + n)
        torch.manual_seed(SEED + 1)
        enc = OscarEncoder(None, trunk, 128, 128, 0.0).to(dev).train()
        eng = _bridge_engine(trunk)
        eng.compact_min_rows = 0 if compact else 1 << 30
        ctx, h_t, c_t = enc(ids.to(dev), list(TEXT_LENS), pad.to(dev))
        ((ctx * weight[:, :ctx.shape[1]]).sum() + h_t.sum() + c_t.sum()).backward()
        torch.cuda.synchronize()
        assert (eng.last_layout is not None) == compact
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in trunk.named_parameters()}, eng

    key = (compact, "trunk node")
    if key not in _reference:
        _reference[key] = grads(NONE_FROZEN)[0]
    want, frozen = _reference[key], PATTERNS[pattern]
    got, eng = grads(frozen)
    seen = 0
    for n in want:
        if frozen("bert." + n) or want[n] is None:   # (the region group and the pooler get nothing from this loss)
            assert got[n] is None, n
        else:
            assert torch.equal(_bits(got[n]), _bits(want[n])), n
            seen += 1
    assert seen > 10 and eng.units["emb"] == (pattern != "bottom")


# ---- 3. census --------------------------------------------------------------------------------------------------------------
def _expected_backward_census(frozen, names):
    """The backward's launches for a frozen-name predicate, from the contract: a unit (an encoder layer, the embedding block, the
    region group, a head group) is computed when one of its members is trainable; the layer loop visits layers L-1 .. stop,
    where stop is 0 when the embedding block or the region group is trainable and the lowest trainable layer otherwise; layer
    `stop` then skips its last dgrad; a frozen layer above runs 4 dgrads, its attention backward and two dx-only LayerNorm
    backwards; a head's dgrad runs when something in the trunk wants the gradient."""
    on = lambda prefixes: any(n.startswith(prefixes) and not frozen(n) for n in names)
    layers = [on("bert.encoder.layer.%d." % l) for l in range(L)]
    emb, region = on(EMB), on(REGION)
    word = not frozen("bert.embeddings.word_embeddings.weight")
    mlm = on("mlmhead.") or word   # the tied decoder's launch feeds the word table
    token, action, pooler = on("token_head."), on("next_action."), on("bert.pooler.")
    under = emb or region          # the batch has regions
    stop = 0 if under else next((l for l in range(L) if layers[l]), L)
    visited = range(stop, L)
    trunk = under or any(layers)
    n_train = sum(layers[l] for l in visited)
    dgrad = 4 * len(visited) - (1 if (len(visited) and not under) else 0)
    dgrad += int(mlm or trunk) + int(trunk)          # through the decoder, through the transform
    dgrad += int(trunk)                              # through the token head
    dgrad += int(pooler or trunk) + int(trunk)       # through the action head, through the pooler
    return {"gemm_wgrad_tn_bf16": n_train + 2 * mlm + token + action + pooler + region,
            "layernorm_bwd_rows": 2 * n_train + mlm,   # = the reduce launches: one behind every full LayerNorm backward
            "layernorm_bwd_dx": 2 * (len(visited) - n_train) + int(trunk and not mlm),
            "attention_bwd_d64": len(visited),
            "gemm_nt_bf16": dgrad}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("pattern", ["all trainable"] + list(PATTERNS))
def test_backward_launch_census(dev, det, pattern, layout):
    frozen = PATTERNS.get(pattern, NONE_FROZEN)
    if pattern == "all trainable":
        m, eng = _engine(dev, frozen, layout)
        census = _all_trainable(dev, layout, "unrolled")[1]
    else:
        m, eng = _engine(dev, frozen, layout)
        census = _run(eng, m, dev, layout, "unrolled")[1]
    want = _expected_backward_census(frozen, [n for n, _ in m.named_parameters()])
    got = {k: census.get(k, 0) for k in want}
    print("CENSUS %-18s %-9s %s" % (pattern, layout, got))
    assert got == want
    if pattern == "all trainable":
        # the counts of the step before requires_grad was read: per layer 4 dgrads, 2 LayerNorm backwards (each with its
        # reduce), one attention backward and one grouped weight gradient; 5 head dgrads, 5 head + 1 region weight gradients,
        # the MLM transform's LayerNorm backward
        assert got == {"gemm_wgrad_tn_bf16": L + 6, "layernorm_bwd_rows": 2 * L + 1, "layernorm_bwd_dx": 0,
                       "attention_bwd_d64": L, "gemm_nt_bf16": 4 * L + 5}


# ---- 4. gradual unfreezing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gradual_unfreezing_follows_the_oracle_rule_and_resumes_bitwise(dev, det, layout):
    from oracle.optim import AdamW

    layer0 = lambda n: n.startswith("bert.encoder.layer.0.")
    m, eng = _engine(dev, layer0, layout, lr=2e-3, weight_decay=0.05)
    names = [n for n, _ in m.named_parameters()]
    # the oracle's optimizer over CPU copies, fed the engine's own gradients: isolates the update rule and its step counts
    twins = {n: torch.nn.Parameter(p.detach().cpu().clone()) for n, p in m.named_parameters()}
    no_decay = lambda n: "bias" in n or "LayerNorm.weight" in n
    opt = AdamW([dict(params=[twins[n] for n in names if not no_decay(n)], weight_decay=0.05),
                 dict(params=[twins[n] for n in names if no_decay(n)], weight_decay=0.0)], lr=2e-3, eps=1e-8)
    start = {n: t.detach().clone() for n, t in twins.items()}
    batch = _batch(dev)
    saved = None
    for step in range(4):
        if step == 2:
            for n, p in m.named_parameters():
                p.requires_grad = True
        if step == 3:
            saved = (eng.state_dict(), {k: v.clone() for k, v in m.state_dict().items()})
        eng.train_step(batch)
        torch.cuda.synchronize()
        for n, p in m.named_parameters():
            twins[n].grad = None if p.grad is None else p.grad.detach().cpu().clone()
        assert (twins["bert.encoder.layer.0.output.dense.weight"].grad is None) == (step < 2)
        opt.step()
    assert {eng.param_steps[n] for n in names if layer0(n)} == {2}
    assert {eng.param_steps[n] for n in names if not layer0(n)} == {4}
    _assert_copies_fresh(eng)
    f = eng.flat
    for n, p in m.named_parameters():
        w = twins[n].detach()
        delta = float((w - start[n]).abs().max())
        assert delta > 0
        assert float((p.detach().cpu() - w).abs().max()) < 1e-6 + 1e-4 * delta, n
        st = opt.state[twins[n]]
        assert st["step"] == eng.param_steps[n]
        for slab, key in ((f.m, "exp_avg"), (f.v, "exp_avg_sq")):
            mo = st[key]
            assert float((f.view(slab, n).cpu() - mo).abs().max()) < 1e-6 + 1e-4 * float(mo.abs().max()), n   # (from zero)

    # ---- resume: the state saved after step 3 in a fresh engine, step 4 again
    torch.manual_seed(SEED)
    m2 = _model(dev, NONE_FROZEN)
    m2.load_state_dict(saved[1])
    m2.tie_weights()
    from visitron_amd.training import PretrainEngine

    eng2 = PretrainEngine(m2, lr=2e-3, weight_decay=0.05, schedule="constant")
    eng2.compact_rows = layout == "compacted"
    eng2.load_state_dict(saved[0])
    assert eng2.param_steps == saved[0]["param_steps"] and len({t for _, _, t in eng2.adam_segments}) == 2
    eng2.train_step(batch)
    torch.cuda.synchronize()
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(_bits(p), _bits(q)), n
    assert torch.equal(_bits(eng.flat.m), _bits(eng2.flat.m)) and torch.equal(_bits(eng.flat.v), _bits(eng2.flat.v))
    assert torch.equal(eng.flat.mirror.view(torch.int16), eng2.flat.mirror.view(torch.int16))


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from visitron_amd.training import PretrainEngine

    with pytest.raises(NotImplementedError, match="shard_optimizer=True serves a model whose parameters all require grad"):
        PretrainEngine(_model(dev, PATTERNS["word table"]), shard_optimizer=True)
    m = _model(dev, NONE_FROZEN)
    eng = PretrainEngine(m, shard_optimizer=True)
    m.next_action.linear.bias.requires_grad = False
    with pytest.raises(NotImplementedError, match="shard_optimizer=True serves a model whose parameters all require grad"):
        eng.train_step(_batch(dev))


def test_fp32_engine_leaves_frozen_parameters_alone(dev):
    """The fp32 engine honours "frozen means frozen" (it may compute every gradient: it skips no launch)."""
    from visitron_amd.training import PretrainEngine

    frozen = PATTERNS["bottom"]
    torch.manual_seed(SEED)
    m = _model(dev, frozen)
    eng = PretrainEngine(m, lr=1e-3, schedule="constant", precision="fp32")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    batch = _batch(dev)
    for _ in range(2):
        eng.train_step(batch)
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if frozen(n):
            assert torch.equal(_bits(p), _bits(before[n])) and p.grad is None, n
            assert not bool(eng.flat.view(eng.flat.m, n).any()) and not bool(eng.flat.view(eng.flat.v, n).any()), n
        else:
            assert not torch.equal(p.detach(), before[n]), n
