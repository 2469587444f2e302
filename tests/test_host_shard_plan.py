"""CPU: the static ownership plan of the optimizer sharded over data-parallel ranks (visitron_amd.distributed.ShardPlan, built by
PretrainEngine.shard_plan): who owns which slab element, where segments are cut, where the owned moments live -- for the
four-layer mini model and for the base layer shape on two layers, at world 2, 4 and 8 and at a small and a large bucket."""
import numpy as np
import pytest
import torch

from visitron_amd.config import BertConfig, mini_config
from visitron_amd.distributed import ShardPlan, complement_ranges
from visitron_amd.modeling import PreTrainOscar
from visitron_amd.ops import round_up
from visitron_amd.training import ALIGN, PretrainEngine, _is_no_decay

WORLDS = (2, 4, 8)
BUCKETS_MB = (0.05, 64)


def _bucket_elems(mb):
    return int(mb * 1024 * 1024 // 4)   # PretrainEngine's own rule


@pytest.fixture(scope="module", params=["mini4", "base2"])
def engine(request):
    if request.param == "mini4":
        cfg = mini_config(num_hidden_layers=4)
    else:
        cfg = BertConfig(num_hidden_layers=2, vocab_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                         max_position_embeddings=64)
    m = PreTrainOscar(cfg)
    m.tie_weights()
    return PretrainEngine(m)


def _launched_ranges(eng, per_chunk):
    """The range lists forward_backward hands to comm["launch"] (and train_step's tail), from the code's own rules: the heads,
    the layer chunks last layers first with ends rounded up to ALIGN, then the complement."""
    f, L = eng.flat, eng.cfg.num_hidden_layers
    out = [eng._param_ranges(eng._head_params())]
    hi = L
    while hi > 0:
        lo = max(0, hi - per_chunk)
        out.append([(eng.layer_ranges[lo][k][0], min(round_up(eng.layer_ranges[hi - 1][k][1], ALIGN), f.total)) for k in (0, 1)])
        hi = lo
    out.append(complement_ranges(f.total, [r for rng in out for r in rng]))
    return out


@pytest.mark.parametrize("mb", BUCKETS_MB)
@pytest.mark.parametrize("world", WORLDS)
def test_every_element_has_one_owner_and_segments_respect_the_cuts(engine, world, mb):
    f = engine.flat
    fp32 = np.zeros(f.total, dtype=bool)
    for s, e in engine.fp32_spans():
        fp32[s:e] = True
    owner = np.full(f.total, -1, dtype=np.int64)
    for rank in range(world):
        plan = engine.shard_plan(world, rank, _bucket_elems(mb))
        every = plan.everything()
        assert plan.owned * world == f.total
        local = np.zeros(plan.owned, dtype=np.int64)
        for bs, be, has16, has32 in every.buckets:
            assert 0 < be - bs <= _bucket_elems(mb) and (be - bs) % (8 * world) == 0
            pieces = [plan.piece(bs, be, r) for r in range(world)]
            assert pieces[0][0] == bs and pieces[-1][1] == be
            assert all(a[1] == b[0] for a, b in zip(pieces[:-1], pieces[1:]))            # contiguous, in rank order
            assert len({pe - ps for ps, pe in pieces}) == 1 and (pieces[0][1] - pieces[0][0]) % 8 == 0
            assert has16 == bool((~fp32[bs:be]).any()) and has32 == bool(fp32[bs:be].any())
        for s, e, dec, f32, mo in every.own:
            assert e > s and s % 8 == 0 and e % 8 == 0 and mo % 8 == 0
            assert (owner[s:e] == -1).all()
            owner[s:e] = rank
            assert not (s < f.n_decay < e) and dec == (s < f.n_decay)                    # never across the decay boundary
            assert fp32[s:e].all() if f32 else not fp32[s:e].any()                       # ... nor a travel-class boundary
            local[mo:mo + e - s] += 1
        assert (local == 1).all()                                                        # bijection onto [0, owned)
        # everybody else's segments: the rest of the slab, cut by the same rules
        seen = np.zeros(f.total, dtype=np.int64)
        for s, e, f32 in every.others:
            seen[s:e] += 1
            assert not (s < f.n_decay < e) and (fp32[s:e].all() if f32 else not fp32[s:e].any())
        for s, e, _, _, _ in every.own:
            seen[s:e] += 1
        assert (seen == 1).all()
    assert (owner >= 0).all()


@pytest.mark.parametrize("mb", BUCKETS_MB)
@pytest.mark.parametrize("world", WORLDS)
def test_the_plan_does_not_depend_on_layers_per_chunk(engine, world, mb):
    plan = engine.shard_plan(world, world - 1, _bucket_elems(mb))
    per = {}
    for per_chunk in (1, 2, 3):
        own, others, buckets, covered = [], [], [], 0
        for rng in _launched_ranges(engine, per_chunk):
            la = plan.launch(rng)
            own += la.own
            others += la.others
            buckets += [b[:2] for b in la.buckets]
            covered += sum(e - s for s, e in rng)
        assert covered == engine.flat.total
        per[per_chunk] = (sorted(own), sorted(others), sorted(buckets))
    assert per[1] == per[2] == per[3]
    every = plan.everything()
    assert per[1] == (sorted(every.own), sorted(every.others), sorted(b[:2] for b in every.buckets))
    # the atoms ARE the launches at one layer per chunk, and the engine's un-overlapped launch list is that sequence
    assert sorted(r for rng in _launched_ranges(engine, 1) for r in rng) == plan.atoms
    assert engine.shard_launch_ranges() == [rng for rng in _launched_ranges(engine, 1) if rng]


@pytest.mark.parametrize("world", (3, 6, 1, 16))
def test_other_world_sizes_are_refused(engine, world):
    with pytest.raises(ValueError, match="world sizes"):
        engine.shard_plan(world, 0)
    with pytest.raises(ValueError, match="world sizes"):
        ShardPlan(128, 64, [(0, 128)], [], world, 0, 64)


def test_plan_refuses_ranges_that_are_no_union_of_atoms_and_gaps():
    plan = ShardPlan(256, 128, [(0, 64), (64, 256)], [(128, 256)], 2, 1, 64)
    assert plan.launch([(0, 256)]).own_elems == 128
    with pytest.raises(ValueError, match="union"):
        plan.launch([(0, 32)])
    with pytest.raises(ValueError, match="cover"):
        ShardPlan(256, 128, [(0, 64), (128, 256)], [], 2, 0, 64)


def test_fp32_class_holds_the_no_decay_group_and_the_embedding_tables(engine):
    f = engine.flat
    fp32 = np.zeros(f.total, dtype=bool)
    for s, e in engine.fp32_spans():
        fp32[s:e] = True
    only16 = engine.mirror_only_names()
    tables = {"bert.embeddings.%s.weight" % t for t in ("word_embeddings", "position_embeddings", "token_type_embeddings")}
    for n, _, o, cnt, grp in f.entries:
        if _is_no_decay(n) or n in tables:
            assert fp32[o:o + cnt].all() and n not in only16, n
        assert fp32[o:o + cnt].all() != (n in only16), n
    assert fp32[f.n_decay:].all()
    # what travels as bf16: the encoder's GEMM weights, and the matrices the heads / pooler / region projection take via _mirror
    H, I, L = engine.cfg.hidden_size, engine.cfg.intermediate_size, engine.cfg.num_hidden_layers
    assert sum(f.off[n][1] for n in only16 if n.startswith("bert.encoder.")) == L * (4 * H * H + 2 * H * I)
    for n in ("bert.pooler.dense.weight", "bert.img_embedding.weight", "bert.location_embeds.weight",
              "mlmhead.predictions.transform.dense.weight", "token_head.0.weight", "next_action.linear.weight"):
        assert n in only16, n


def test_flat_params_can_leave_the_moment_slabs_out():
    from visitron_amd.training import FlatParams

    f = FlatParams(PreTrainOscar(mini_config()), moments=False)
    assert f.m is None and f.v is None and f.p.numel() == f.total
    g = FlatParams(PreTrainOscar(mini_config()))
    assert g.m.numel() == g.v.numel() == g.total
