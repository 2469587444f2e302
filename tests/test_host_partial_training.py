"""CPU: what PretrainEngine derives from requires_grad -- the unit flags (encoder layers, embedding block, head groups; the tied
MLM decoder shares the word table's flag), the layer at which the backward stops, the slab ranges that are reduced and
stepped (filtered to the trainable parameters and merged), and the per-parameter update counts through state_dict() /
load_state_dict().  The engine is built over CPU tensors: nothing here launches a kernel."""
import math

import pytest
import torch

from visitron_amd import training
from visitron_amd.config import BertConfig
from visitron_amd.modeling import PreTrainOscar
from visitron_amd.training import ALIGN, PretrainEngine, backward_stop, intersect_ranges, merge_spans, step_segments, unit_flags

L = 3


def _model(untied=False):
    cfg = BertConfig(vocab_size=97, hidden_size=128, num_hidden_layers=L, num_attention_heads=2, intermediate_size=256,
                     max_position_embeddings=32, img_feature_dim=20, detector_classes=11, action_space=5)
    torch.manual_seed(0)
    m = PreTrainOscar(cfg)
    if untied:
        m.resize_embeddings({"word_embeddings": cfg.vocab_size + 3})
    return m


def _freeze(model, pred):
    for n, p in model.named_parameters():
        p.requires_grad = not pred(n)


def _engine(pred=None, untied=False, **kw):
    m = _model(untied)
    if pred is not None:
        _freeze(m, pred)
    return PretrainEngine(m, **kw)


ALL_ON = dict(layers=[True] * L, emb=True, region=True, mlm=True, token=True, action=True, pooler=True)


def test_all_trainable_is_the_whole_slab_in_one_segment():
    eng = _engine()
    assert eng.units == ALL_ON
    assert eng.train_spans == [(0, eng.flat.total)]
    assert eng.adam_segments == [(0, eng.flat.total, 0)]
    assert all(p.grad is not None for p in eng.model.parameters())
    row = eng.g_tab[0]
    assert all(getattr(row, f[0]) for f in row._fields_)


@pytest.mark.parametrize("name,pred,want", [
    ("word table only: the embedding block stays mixed, the tied decoder keeps its flag with it",
     lambda n: n == "bert.embeddings.word_embeddings.weight", ALL_ON),
    ("embedding block: the tied decoder weight is frozen with it, the rest of the MLM group is not",
     lambda n: n.startswith("bert.embeddings."), dict(ALL_ON, emb=False)),
    ("embeddings + region + layers 0-1",
     lambda n: n.startswith(("bert.embeddings.", "bert.img_embedding.", "bert.location_embeds.", "bert.encoder.layer.0.",
                             "bert.encoder.layer.1.")),
     dict(ALL_ON, emb=False, region=False, layers=[False, False, True])),
    ("layer 1 only", lambda n: n.startswith("bert.encoder.layer.1."), dict(ALL_ON, layers=[True, False, True])),
    ("everything but the action head", lambda n: not n.startswith("next_action."),
     dict(layers=[False] * L, emb=False, region=False, mlm=False, token=False, action=True, pooler=False)),
    ("a mixed unit: layer 2's biases only", lambda n: n.startswith("bert.encoder.layer.2.") and n.endswith(".bias"), ALL_ON),
    ("MLM group but for the word table: the decoder launch still feeds the word table",
     lambda n: n.startswith("mlmhead."), ALL_ON),
])
def test_unit_flags(name, pred, want):
    eng = _engine(pred)
    assert eng.units == want, name
    for n, p in eng.model.named_parameters():
        assert (p.grad is None) == pred(n), n
    for l in range(L):   # a frozen layer's row of the C loop's gradient table is null, a computed one's is whole
        row = eng.g_tab[l]
        assert [bool(getattr(row, f[0])) for f in row._fields_] == [want["layers"][l]] * 12


def test_untied_decoder_has_a_flag_of_its_own():
    eng = _engine(lambda n: n.startswith("mlmhead."), untied=True)
    assert not eng._decoder_tied()
    assert eng.units == dict(ALL_ON, mlm=False)
    eng = _engine(lambda n: n.startswith("mlmhead.") and "decoder" not in n, untied=True)
    assert eng.units == ALL_ON
    names = ["bert.embeddings.word_embeddings.weight"]
    assert unit_flags(names, [True], L, tied_decoder=False)["mlm"] is False
    assert unit_flags(names, [True], L, tied_decoder=True)["mlm"] is True
    with pytest.raises(KeyError, match="belongs to no unit"):
        unit_flags(["somewhere.else.weight"], [True], L)


def test_backward_stop():
    # something below the layers wants the gradient: every layer runs and layer 0 produces dL/d(input)
    assert backward_stop([False, False, True], True) == (0, True)
    assert backward_stop([False] * 3, True) == (0, True)
    # nothing below: the loop stops at the lowest trainable layer, whose last dgrad is not needed
    assert backward_stop([False, False, True], False) == (2, False)
    assert backward_stop([True, False, True], False) == (0, False)
    assert backward_stop([False, True, False], False) == (1, False)   # (the frozen layer 2 above runs dx-only)
    assert backward_stop([False] * 3, False) == (3, False)            # no layer at all
    # a history tensor that requires grad is a request of its own
    assert backward_stop([False, False, True], False, [False, True, False]) == (1, False)
    assert backward_stop([False, False, False], False, [False, False, False]) == (3, False)


class _St(object):
    def __init__(self, img, hist=None):
        self.img, self.hist = img, hist


def test_engine_stop_rule_counts_regions_and_callers():
    bottom = lambda n: n.startswith(("bert.embeddings.", "bert.encoder.layer.0."))
    eng = _engine(bottom)
    assert eng._backward_stop(_St(img=object())) == (0, True)      # the region group is trainable and the batch has regions
    assert eng._backward_stop(_St(img=None)) == (1, False)         # ... a text-only batch feeds nothing below layer 1
    assert eng._backward_stop(_St(img=None), d_hidden=[None] * (L + 1)) == (0, True)
    hist = dict(need=[True, False, False])
    assert eng._backward_stop(_St(img=None, hist=hist)) == (0, False)
    assert eng._trunk_wants_grad(_St(img=None))
    heads = _engine(lambda n: not n.startswith("next_action."))
    assert heads._backward_stop(_St(img=object())) == (L, False)
    assert not heads._trunk_wants_grad(_St(img=object()))
    assert heads._trunk_wants_grad(_St(img=None, hist=hist))


def test_range_helpers():
    assert merge_spans([(64, 128), (0, 64), (200, 260), (250, 300), (5, 5)]) == [(0, 128), (200, 300)]
    assert intersect_ranges([(0, 100), (150, 400)], [(50, 200), (300, 350)]) == [(50, 100), (150, 200), (300, 350)]
    assert intersect_ranges([(0, 10)], []) == []
    entries = [("a", (0, 64)), ("b", (64, 128)), ("c", (128, 192)), ("d", (192, 256))]
    assert step_segments(entries, [True] * 4, dict(a=3, b=3, c=3, d=3)) == [(0, 256, 3)]
    assert step_segments(entries, [True, False, True, True], dict(a=3, b=3, c=3, d=1)) == [(0, 64, 3), (128, 192, 3), (192, 256, 1)]
    assert step_segments(entries, [False] * 4, dict(a=0, b=0, c=0, d=0)) == []


def test_ranges_are_filtered_to_the_trainable_parameters():
    full = _engine()
    eng = _engine(lambda n: n.startswith("bert.encoder.layer.1.") or n == "bert.pooler.dense.weight")
    f = eng.flat
    frozen = [f.span[n] for n, p, _, _, _ in f.entries if not p.requires_grad]
    assert eng.train_spans == merge_spans(training.distributed.complement_ranges(f.total, merge_spans(frozen)))
    assert all(s_ % ALIGN == 0 and e_ % ALIGN == 0 for s_, e_ in eng.train_spans)
    # the layer chunk of the frozen layer is empty, its neighbours' are what they were
    assert eng._layer_chunk_ranges(1, 2) == []
    assert eng._layer_chunk_ranges(0, 1) == full._layer_chunk_ranges(0, 1)
    assert eng._layer_chunk_ranges(2, 3) == full._layer_chunk_ranges(2, 3)
    assert eng._layer_chunk_ranges(0, 3) == intersect_ranges(full._layer_chunk_ranges(0, 3), eng.train_spans)
    # the head ranges lose the pooler's weight and keep its bias
    o, cnt, _ = f.off["bert.pooler.dense.weight"]
    heads = eng._param_ranges(eng._head_params())
    assert all(e_ <= o or s_ >= o + cnt for s_, e_ in heads)
    ob = f.off["bert.pooler.dense.bias"][0]
    assert any(s_ <= ob < e_ for s_, e_ in heads)
    assert eng._trainable_ranges([(0, f.total)]) == eng.train_spans
    assert full._param_ranges(full._head_params()) != heads


def test_flags_are_read_again_and_steps_are_counted_per_parameter(monkeypatch):
    calls = []
    monkeypatch.setattr(training.ops, "adamw_flat", lambda p, g, m, v, mir, lr, step_size, *rest: calls.append(
        (p.data_ptr(), p.numel(), step_size)))
    monkeypatch.setattr(training, "invalidate_packed_weights", lambda: None)
    layer0 = lambda n: n.startswith("bert.encoder.layer.0.")
    eng = _engine(layer0, lr=1e-3, schedule="constant")
    f, base = eng.flat, eng.flat.p.data_ptr()
    eng.optimizer_step()
    eng.optimizer_step()
    lo = [f.span[n] for n, _, _, _, _ in f.entries if layer0(n)]
    for ptr, n, _ in calls:   # no launch touches a frozen range
        s_, e_ = (ptr - base) // 4, (ptr - base) // 4 + n
        assert all(e_ <= a_ or s_ >= b_ for a_, b_ in lo)
    assert {eng.param_steps[n] for n, _, _, _, _ in f.entries if layer0(n)} == {0}
    assert {eng.param_steps[n] for n, _, _, _, _ in f.entries if not layer0(n)} == {2}
    _freeze(eng.model, lambda n: False)   # unfreeze: the next step finds the flags changed
    del calls[:]
    eng.optimizer_step()
    assert eng.step_count == 3 and eng.units["layers"][0]
    assert all(p.grad is not None for p in eng.model.parameters())
    b1, b2 = eng.betas
    size = lambda t: 1e-3 * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    for ptr, n, step_size in calls:
        s_ = (ptr - base) // 4
        inside = any(a_ <= s_ < b_ for a_, b_ in lo)
        assert step_size == size(1 if inside else 3)   # its own first update, as torch's per-parameter state["step"]
    assert sum(n for _, n, _ in calls) == f.total      # every element stepped exactly once
    # frozen again: the counts stay where they are
    _freeze(eng.model, layer0)
    eng.optimizer_step()
    assert {eng.param_steps[n] for n, _, _, _, _ in f.entries if layer0(n)} == {1}
    assert eng.model.bert.encoder.layer[0].output.dense.weight.grad is None

    # ---- save / load round trip
    sd = eng.state_dict()
    assert sd["param_steps"] == eng.param_steps and sd["step_count"] == 4
    other = _engine(lr=1e-3, schedule="constant")
    other.load_state_dict(sd)
    assert other.param_steps == eng.param_steps
    assert sorted(t for _, _, t in other.adam_segments) == sorted(
        t for _, _, t in step_segments([(n, f.span[n]) for n, _, _, _, _ in f.entries], [True] * len(f.entries), eng.param_steps))
    assert {t for _, _, t in other.adam_segments} == {1, 4}
    # a state written before the counts existed: every parameter from the global step
    del sd["param_steps"]
    other.load_state_dict(sd)
    assert set(other.param_steps.values()) == {4} and other.adam_segments == [(0, f.total, 4)]


def test_a_failed_overlapped_step_takes_its_counting_back():
    eng = _engine(lambda n: n.startswith("bert.encoder.layer.0."))
    eng._adam_begin()
    eng._adam_abort()
    assert eng.step_count == 0 and set(eng.param_steps.values()) == {0}
    assert {t for _, _, t in eng.adam_segments} == {0}


def test_refusals():
    with pytest.raises(NotImplementedError, match="shard_optimizer=True serves a model whose parameters all require grad"):
        _engine(lambda n: n.startswith("bert.embeddings."), shard_optimizer=True)
    eng = _engine(shard_optimizer=True)
    eng.model.bert.pooler.dense.bias.requires_grad = False   # ... and at any later step
    with pytest.raises(NotImplementedError, match="shard_optimizer=True serves a model whose parameters all require grad"):
        eng._sync_trainable()
    eng.model.bert.pooler.dense.bias.requires_grad = True
    sd = _engine().state_dict()
    sd["param_steps"]["bert.pooler.dense.bias"] = 7
    with pytest.raises(NotImplementedError, match="took the same number of updates"):
        eng.load_state_dict(sd)


def test_all_reduce_grads_leaves_frozen_ranges_off_the_wire(monkeypatch):
    calls = []
    monkeypatch.setattr(training.distributed, "all_reduce_flat", lambda flat, per, pg=None: calls.append(("flat", flat.numel())))
    monkeypatch.setattr(training.distributed, "all_reduce_ranges",
                        lambda flat, ranges, per, pg=None, handles=None: calls.append(("ranges", list(ranges))))
    eng = _engine()
    eng.world = 2   # (no process group: the two collectives are recorded, not run)
    eng.all_reduce_grads()
    assert calls == [("flat", eng.flat.total)]   # all trainable: the whole slab in buckets, as before
    del calls[:]
    _freeze(eng.model, lambda n: n.startswith("bert.encoder.layer.1."))
    eng.all_reduce_grads()
    assert calls == [("ranges", eng.train_spans)] and len(eng.train_spans) == 3
    frozen = [eng.flat.span[n] for n, p, _, _, _ in eng.flat.entries if not p.requires_grad]
    assert all(e_ <= a_ or s_ >= b_ for s_, e_ in eng.train_spans for a_, b_ in frozen)
