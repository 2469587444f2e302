"""GPU: the region gather (csrc/regions.hip through visitron_amd.ops.region_gather and visitron_amd.RegionStore) against the
oracle expectation of tests/helpers_regions.py, bit for bit, and the packed operand through PretrainEngine and the module
forwards.  The store lies inside a NaN-filled buffer (the rows a view does not have are NaN too) and every output of the
kernel tests is a view inside a sentinel-filled buffer whose surroundings must stay untouched and whose inside must be fully
written.  Shapes: helpers_regions (N = 6, P = 5, B = 5, T = 9; D = 2054 the shipped width, 16, 10; R = 12, 40, 180, 0)."""
import math

import numpy as np
import pytest
import torch

import helpers_regions as hr

pytestmark = pytest.mark.gpu

PAD = 64          # elements around every view: a multiple of 16 bytes in every dtype used
SENTINEL = -7.25
_stores, _results = {}, {}


def _inside(shape, dtype, dev, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + n].view(*shape)


def _untouched(buf, n, fill):
    head, tail = buf[:PAD], buf[PAD + n:]
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == fill).all()) and bool((tail == fill).all())


def _store(dev, D, R, dtype):
    """A RegionStore of the case's features whose tensors were moved inside guard buffers: NaN around the features, 255 (a
    count no view can have) around the counts."""
    from visitron_amd import RegionStore

    key = (D, R, dtype)
    if key not in _stores:
        store = RegionStore(hr.triple_for(D, R), dev, dtype=dtype)
        fbuf, fview = _inside(store.features.shape, dtype, dev, float("nan"))
        fview.copy_(store.features)
        cbuf, cview = _inside(store.counts.shape, torch.uint8, dev, 255)
        cview.copy_(store.counts)
        store.features, store.counts = fview, cview
        _stores[key] = (store, fbuf, cbuf, fview.clone(), cview.clone())
    return _stores[key]


def _store_intact(entry):
    store, fbuf, cbuf, f0, c0 = entry
    same = torch.equal(store.features.view(torch.int16 if f0.dtype == torch.bfloat16 else torch.int32),
                       f0.view(torch.int16 if f0.dtype == torch.bfloat16 else torch.int32))
    return same and torch.equal(store.counts, c0) and _untouched(fbuf, f0.numel(), float("nan")) and _untouched(cbuf, c0.numel(), 255)


def _gather(dev, D, R, batch, dtype, packed, token=True, rows=None, counts=None):
    """ops.region_gather into sentinel-surrounded outputs -> (outputs on the host, error flag)."""
    from visitron_amd import ops

    entry = _store(dev, D, R, dtype)
    store = entry[0]
    tx = hr.text_tensors()
    if rows is None:
        rows = np.array(hr.BATCHES[batch], dtype=np.int32).T
    rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(dev)
    kpad = hr.kpad_of(D)
    S = hr.T + R
    if packed:
        shapes, dtypes, fills = [(hr.B * R, kpad)], [torch.bfloat16], [SENTINEL]
    else:
        shapes, dtypes, fills = [(hr.B, R, D), (hr.B, R, 128)], [torch.float32] * 2, [SENTINEL] * 2
    nint = 3 if token else 2
    shapes, dtypes, fills = shapes + [(hr.B, S)] * nint, dtypes + [torch.int64] * nint, fills + [-77] * nint
    bufs, outs = zip(*[_inside(s, dt, dev, f) for s, dt, f in zip(shapes, dtypes, fills)])
    outs = tuple(outs) + (() if token else (None,))
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    d = lambda t: t.to(dev)
    ops.region_gather(store.features, store.counts if counts is None else counts, store.loc_table, rows, D, d(tx["labels"]),
                      d(tx["att"]), d(tx["token_classes"]) if token else None, R, kpad=kpad if packed else None, out=outs,
                      err_flag=err)
    torch.cuda.synchronize()
    for buf, s, f in zip(bufs, shapes, fills):
        assert _untouched(buf, int(np.prod(s)), f), "written outside the view %s" % (s,)
    assert _store_intact(entry)
    got = [None if o is None else o.cpu() for o in outs]
    for g, f in zip(got, fills):
        if g is not None:
            assert not bool((g.float() == f).any()) and bool(torch.isfinite(g.float()).all()), "an element was left unwritten, or NaN"
    return got, int(err.item())


def _all(dev, D, R, batch):
    """The four gathers of one case (fp32 / bf16 store x unpacked / packed), once."""
    key = (D, R, batch)
    if key not in _results:
        res = {}
        for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            for packed in (False, True):
                got, err = _gather(dev, D, R, batch, dtype, packed)
                assert err == 0
                res[name, packed] = got
        _results[key] = res
    return _results[key]


CASES = [(D, R, batch) for D in hr.DS for R in hr.RS for batch in sorted(hr.BATCHES)]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("D,R,batch", CASES)
def test_unpacked_from_an_fp32_store_is_the_oracles(dev, D, R, batch):
    exp = hr.expectation(D, R, batch)
    feats, loc, labels, mask, tok = _all(dev, D, R, batch)["f32", False]
    assert torch.equal(feats, exp["img_feats"]) and torch.equal(loc, exp["img_location_embeddings"])
    assert torch.equal(labels, exp["labels"]) and torch.equal(mask, exp["attention_mask"]) and torch.equal(tok, exp["token_labels"])
    # without token classes, and the store's own call with no_action_grounding
    got, err = _gather(dev, D, R, batch, torch.float32, False, token=False)
    assert err == 0 and got[-1] is None and torch.equal(got[0], exp["img_feats"]) and torch.equal(got[2], exp["labels"])
    assert torch.equal(got[3], exp["attention_mask"])
    store, tx = _store(dev, D, R, torch.float32)[0], hr.text_tensors()
    for nag in (False, True):
        want = hr.expectation(D, R, batch, token_classes=not nag, no_action_grounding=nag)
        out = store.pretrain_batch(*hr.BATCHES[batch], tx["input_ids"], tx["labels"], tx["att"], tx["next_action"], R,
                                   token_classes=None if nag else tx["token_classes"], no_action_grounding=nag)
        assert list(out) == ["input_ids", "labels", "attention_mask", "img_feats", "img_location_embeddings", "next_action",
                             "token_labels"]
        for k, w in want.items():
            assert (out[k] is None and w is None) or (out[k].device == dev and torch.equal(out[k].cpu(), w)), k


@pytest.mark.parametrize("D,R,batch", CASES)
def test_packed_from_an_fp32_store_is_pack_concat_of_the_unpacked(dev, D, R, batch):
    from visitron_amd import ops

    res = _all(dev, D, R, batch)
    feats, loc = res["f32", False][:2]
    packed = res["f32", True][0]
    assert packed.shape == (hr.B * R, hr.kpad_of(D)) and packed.dtype == torch.bfloat16
    for a, b in zip(res["f32", True][1:], res["f32", False][2:]):
        assert torch.equal(a, b)
    if R == 0:
        return
    want = ops.pack_concat(feats.reshape(hr.B * R, D).to(dev), loc.reshape(hr.B * R, 128).to(dev), hr.kpad_of(D)).cpu()
    assert torch.equal(_bits(packed), _bits(want))
    assert not bool(packed[:, D + 128:].float().any())                       # the zero tail
    assert torch.equal(packed.float(), hr.packed_of(hr.expectation(D, R, batch), D).to(torch.bfloat16).float())


@pytest.mark.parametrize("D,R,batch", CASES)
def test_a_bf16_store_serves_the_rounded_features_and_the_same_packed_bits(dev, D, R, batch):
    res = _all(dev, D, R, batch)
    exp = hr.expectation(D, R, batch, rounded=True)
    assert torch.equal(res["bf16", False][0], exp["img_feats"])
    for a, b in zip(res["bf16", False][1:], res["f32", False][1:]):
        assert torch.equal(a, b)
    assert torch.equal(_bits(res["bf16", True][0]), _bits(res["f32", True][0]))
    for a, b in zip(res["bf16", True][1:], res["f32", True][1:]):
        assert torch.equal(a, b)
    store, tx = _store(dev, D, R, torch.bfloat16)[0], hr.text_tensors()
    out = store.pretrain_batch(*hr.BATCHES[batch], tx["input_ids"], tx["labels"], tx["att"], tx["next_action"], R,
                               token_classes=tx["token_classes"], packed=True)
    assert list(out) == ["input_ids", "labels", "attention_mask", "img_packed", "img_rows", "next_action", "token_labels"]
    assert out["img_rows"] == R and torch.equal(_bits(out["img_packed"].cpu()), _bits(res["f32", True][0]))


# ---- bad indices: guarded by the kernel, nothing is provoked -----------------------------------------------------------------
@pytest.mark.parametrize("bad", ["slot -1", "slot N", "view 36", "count P+1"])
@pytest.mark.parametrize("packed", [False, True])
def test_bad_indices_zero_the_item_and_raise_index_error(dev, bad, packed):
    import visitron_amd

    D, R, batch, item = 10, 12, "lengths", 3
    rows = np.array(hr.BATCHES[batch], dtype=np.int32).T.copy()
    store = _store(dev, D, R, torch.float32)[0]
    counts = None
    if bad == "count P+1":
        counts = store.counts.clone()
        counts[rows[item, 0], 4] = hr.P + 1
    else:
        rows[item] = {"slot -1": (-1, 13), "slot N": (hr.N, 13), "view 36": (3, 36)}[bad]
    good = _all(dev, D, R, batch)["f32", packed]
    got, err = _gather(dev, D, R, batch, torch.float32, packed, rows=rows, counts=counts)
    assert err == 1
    per_item = lambda t: t.reshape(hr.B, -1)
    for g, w in zip(got[:-3], good[:-3]):                     # the region tensors: the item zero, the others unchanged
        g, w = per_item(g.float()), per_item(w.float())
        assert not bool(g[item].any()) and bool(w[item].any())
        keep = [b for b in range(hr.B) if b != item]
        assert torch.equal(g[keep], w[keep])
    labels, mask, tok = got[-3:]
    assert torch.equal(labels, good[-3]) and torch.equal(tok, good[-1])
    assert not bool(mask[item, hr.T:].any()) and torch.equal(mask[:, :hr.T], good[-2][:, :hr.T])
    keep = [b for b in range(hr.B) if b != item]
    assert torch.equal(mask[keep], good[-2][keep])
    if counts is None:                                       # through the store: the flag surfaces as IndexError
        visitron_amd.check_errors()
        tx = hr.text_tensors()
        with pytest.raises(IndexError):                      # (at the call's end if the flag has landed by then)
            store.pretrain_batch(rows[:, 0], rows[:, 1], tx["input_ids"], tx["labels"], tx["att"], tx["next_action"], R,
                                 packed=packed)
            visitron_amd.check_errors()
        visitron_amd.check_errors()


# ---- the step takes the packed operand -----------------------------------------------------------------------------------------
ENG_D, ENG_R = 70, 12          # mini_config's region width


def _cfg(**kw):
    from visitron_amd.config import mini_config

    return mini_config(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, **kw)


def _model(cfg, dev):
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict

    torch.manual_seed(4321)   # the engine draws its dropout seed base from torch's seed
    m = PreTrainOscar(cfg)
    m.load_state_dict(deterministic_state_dict(m, seed=5))
    return m.to(dev).train()


def _batches(dev, plain=False):
    """The packed and the unpacked batch of one bf16 store.  plain: every item holds at least R rows and no text padding, so
    the step finds nothing to compact."""
    from visitron_amd import RegionStore

    store = RegionStore(hr.mapping_for(ENG_D, ENG_R), dev)
    tx = hr.text_tensors()
    slots, curs = ((2, 3, 4, 5, 2), (0, 7, 35, 13, 24)) if plain else hr.BATCHES["lengths"]
    att = torch.ones_like(tx["att"]) if plain else tx["att"]
    slots = [store.slot("s%d" % i, "v%02d" % i) for i in slots]
    return [store.pretrain_batch(slots, curs, tx["input_ids"], tx["labels"], att, tx["next_action"], ENG_R,
                                 token_classes=tx["token_classes"], packed=p) for p in (True, False)]


@pytest.mark.parametrize("layout,img_ln", [("compact", False), ("plain", False), ("compact", True)])
def test_train_step_on_the_packed_batch_matches_the_unpacked_one_bit_for_bit(dev, layout, img_ln):
    from visitron_amd import ops
    from visitron_amd.training import PretrainEngine

    cfg = _cfg(use_img_layernorm=True, img_layer_norm_eps=1e-12) if img_ln else _cfg()
    ops.set_deterministic(True)
    try:
        res = []
        for batch in _batches(dev, plain=layout == "plain"):
            eng = PretrainEngine(_model(cfg, dev), lr=1e-3, weight_decay=0.05, schedule="constant", warmup_steps=0)
            out = [v.detach().clone() for v in eng.train_step(batch)]
            torch.cuda.synchronize()
            assert (eng.last_layout is not None) == (layout == "compact")
            m = eng.model
            grads = [eng._grad(p).clone() for p in (m.bert.img_embedding.weight, m.bert.location_embeds.weight,
                                                    m.bert.encoder.layer[0].attention.self.query.weight,
                                                    m.bert.encoder.layer[0].output.dense.weight)]
            assert all(bool(g.any()) for g in grads)
            res.append((out, grads, eng.flat.g.clone(), eng.flat.mirror.clone()))
        (out_p, gr_p, g_p, mir_p), (out_u, gr_u, g_u, mir_u) = res
        assert len(out_p) == 7 and all(torch.equal(a, b) for a, b in zip(out_p, out_u)), (out_p, out_u)
        assert all(torch.equal(a, b) for a, b in zip(gr_p, gr_u))
        assert torch.equal(g_p, g_u) and torch.equal(_bits(mir_p), _bits(mir_u))
        assert bool(torch.isfinite(out_p[0]))
    finally:
        ops.set_deterministic(False)


def test_the_engine_checks_the_packed_operand(dev):
    from visitron_amd.training import PretrainEngine

    cfg = _cfg()
    packed, unpacked = _batches(dev)
    eng = PretrainEngine(_model(cfg, dev), lr=1e-3, schedule="constant", warmup_steps=0)
    bad = [dict(packed, img_packed=packed["img_packed"].float()),                          # not bf16
           dict(packed, img_packed=packed["img_packed"][:-1]),                             # not [B * R, kpad]
           dict(packed, img_packed=packed["img_packed"][:, :-64]),
           dict(packed, img_rows=ENG_R + 1),
           dict(packed, img_packed=packed["img_packed"].t().contiguous().t()),             # not contiguous
           dict(packed, img_packed=packed["img_packed"].cpu()),                            # not on the engine's device
           dict(packed, img_feats=unpacked["img_feats"])]                                  # both forms
    for b in bad:
        with pytest.raises(ValueError):
            eng.trunk_forward(b)
    no_rows = {k: v for k, v in packed.items() if k != "img_rows"}
    with pytest.raises(ValueError):
        eng.trunk_forward(no_rows)
    seq, pooled, _ = eng.trunk_forward(packed, training=False)
    seq_u, pooled_u, _ = eng.trunk_forward(unpacked, training=False)
    assert seq.shape == (hr.B, hr.T + ENG_R, cfg.hidden_size) and torch.equal(seq, seq_u) and torch.equal(pooled, pooled_u)


def test_the_fp32_engine_names_the_other_route(dev):
    from visitron_amd.training import PretrainEngine

    packed, _ = _batches(dev)
    eng = PretrainEngine(_model(_cfg(), dev), lr=1e-3, schedule="constant", warmup_steps=0, precision="fp32")
    with pytest.raises(NotImplementedError, match="packed=False.*float32|float32.*packed=False"):
        eng.trunk_forward(packed)
    with pytest.raises(NotImplementedError, match="packed=False"):
        eng.forward_backward(packed)


# ---- the module forwards -------------------------------------------------------------------------------------------------------
def test_module_forwards_take_the_packed_operand(dev):
    from visitron_amd.config import mini_config

    packed, unpacked = _batches(dev)
    cfg = mini_config()
    model = _model(cfg, dev).eval()
    trunk = lambda b: {k: b[k] for k in b if k in ("input_ids", "attention_mask", "img_feats", "img_location_embeddings",
                                                   "img_packed", "img_rows")}
    with torch.no_grad():
        seq_p, pooled_p = model.bert(**trunk(packed))[:2]
        seq_u, pooled_u = model.bert(**trunk(unpacked))[:2]
        out_p, out_u = model(**packed), model(**unpacked)
    assert torch.equal(seq_p, seq_u) and torch.equal(pooled_p, pooled_u)
    assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(out_p, out_u))
    with pytest.raises(ValueError):
        model(**dict(packed, img_feats=unpacked["img_feats"], img_location_embeddings=unpacked["img_location_embeddings"]))
    with pytest.raises(ValueError):
        model.bert(**dict(trunk(packed), img_feats=unpacked["img_feats"]))
    model.train()
    loss = model(**packed)[0]
    loss.backward()
    torch.cuda.synchronize()
    for p in (model.bert.img_embedding.weight, model.bert.location_embeds.weight, model.bert.encoder.layer[0].output.dense.weight):
        assert p.grad is not None and bool(p.grad.any()) and bool(torch.isfinite(p.grad).all())
