"""GPU: parity on the route the product SHIPS.  The test session sends every eval forward through the deferred-LayerNorm
loop (tests/conftest.py: VT_DEFERRED_LN_MIN_ROWS=0); a user's forward below modeling.DEFERRED_LN_MIN_ROWS_DEFAULT token rows
runs the seven-launch layer instead (bf16 embedding rows, plain GEMMs picked by a timing autotuner) -- the reference's own
batch sizes, every mini edge case, every fuzz seed and the rollout's compacted forwards among them.  Here the inference
comparisons of tests/test_gpu_reference_fixtures.py, test_gpu_golden.py, test_gpu_model.py (configs[0]) and test_gpu_fuzz.py
run once more with the shipped threshold set on every model they build (the same bodies, helpers.Route(shipped=True)):
same fixtures, same bounds, every check name marked " [shipped route]", and every call PROVES its route -- the rule is
asked for the call's row count and the output must equal, bit for bit, a run with `deferred_ln = False`.  Cases both
thresholds route alike (history states, per-layer outputs, 8 x 511 = 4 088 rows) are asserted to be such and not run twice.

Then the threshold's two sides and the compacted row count against the oracle, and every plain GEMM candidate forced
through a whole 12-layer seven-launch forward against the reference's outputs, so that the result does not depend on the
autotuner's draw on the box that runs the suite."""
import os

import numpy as np
import pytest
import torch

from helpers import SHIPPED_SUFFIX, Route, check_close, maxabs, model_pair

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 5e-2   # bf16 path, BASELINE.json north_star
SEVEN, SAME = "seven-launch layer", "same route under both thresholds"


def _routes(route):
    return [how for _, how in route.proven]


@pytest.fixture(scope="module")
def base_model(dev):
    """The 12-layer base-config PreTrainOscar on the weights ref_base_cfg0 / ref_shipped_s767 / ref_base_long / ref_text511
    were written with (integer-hash state dict, seed 0, std 0.03), built once for this module; eval forwards only."""
    from test_gpu_reference_fixtures import _product
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import PreTrainOscar

    return _product(PreTrainOscar, BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), 0, 0.03, dev)


# ---- C.1 / C.2: the fixture comparisons under the shipped threshold, each call's route proven ----------------------------
def test_mini_edge_cases_on_the_shipped_route(dev):
    from test_gpu_reference_fixtures import mini_edge_cases

    route = Route(shipped=True)
    mini_edge_cases(dev, route)
    # head masks, 3-D / float / uint8 masks, token types + positions, text_only, four 7-tuple corners, image LayerNorm: the
    # seven-launch layer; history states and the model asked for hidden states + attentions: the same route as in the session
    assert _routes(route).count(SEVEN) == 12 and _routes(route).count(SAME) == 2, route.proven


@pytest.mark.parametrize("fname,T,R,seed,tag", [("ref_shipped_s767.npz", 511, 256, 767, "shipped S=767"),
                                                 ("ref_base_long.npz", 512, 144, 77, "S=656")])
def test_shipped_pretrain_shapes_on_the_shipped_route(dev, base_model, fname, T, R, seed, tag):
    from test_gpu_reference_fixtures import shipped_shape_inference

    route = Route(shipped=True)
    shipped_shape_inference(dev, route, fname, T, R, seed, tag, model=base_model)
    assert route.proven == [(2 * (T + R), SEVEN)] * 2


def test_rollout_shape_8x511_takes_the_deferred_loop_under_both_thresholds(dev, base_model):
    from test_gpu_reference_fixtures import shipped_rollout_shape

    route = Route(shipped=True)
    shipped_rollout_shape(dev, route, model=base_model)
    assert route.proven == [(4088, SAME)] * 2


def test_rollout_encoder_on_the_shipped_route(dev):
    from test_gpu_reference_fixtures import oscar_encoder_inference

    route = Route(shipped=True)
    oscar_encoder_inference(dev, route, np.load(os.path.join(GOLD, "ref_rollout.npz")), 10, {}, "ref rollout OscarEncoder", "enc_")
    assert _routes(route) == [SEVEN] * 2


@pytest.mark.parametrize("name,kw", [("rev", dict(reverse_input=True)), ("l2", dict(num_layers=2)),
                                     ("l2bi_rev", dict(num_layers=2, bidirectional=True, reverse_input=True))])
def test_rollout_encoder_variants_on_the_shipped_route(dev, name, kw):
    from test_gpu_reference_fixtures import oscar_encoder_inference

    route = Route(shipped=True)
    oscar_encoder_inference(dev, route, np.load(os.path.join(GOLD, "ref_rollout2.npz")), 12, kw,
                            "ref rollout OscarEncoder(%s)" % name, "enc_%s_" % name)
    assert _routes(route) == [SEVEN] * 2


def test_golden_mini_fixture_on_the_shipped_route(dev):
    from test_gpu_golden import mini_fixture

    route = Route(shipped=True)
    mini_fixture(dev, route)
    assert _routes(route) == [SEVEN] * 2


def test_golden_base_cfg1_fixture_on_the_shipped_route(dev, base_model):
    from test_gpu_golden import base_cfg1_fixture

    route = Route(shipped=True)
    base_cfg1_fixture(dev, route, model=base_model)
    assert route.proven == [(456, SEVEN)] * 2


def test_base_config_cfg1_matches_oracle_on_the_shipped_route(dev):
    from test_gpu_model import base_config_cfg1

    route = Route(shipped=True)
    base_config_cfg1(dev, route)
    assert route.proven == [(456, SEVEN)] * 2


# ---- C.3: the threshold's two sides, and the compacted row count ---------------------------------------------------------
@pytest.mark.parametrize("B,deferred", [(12, False), (13, True)])
def test_the_two_sides_of_the_threshold_against_the_oracle(dev, B, deferred):
    """Base width, 3 layers, sequences of 228: B = 12 (2 736 rows) is the last batch on the seven-launch layer, B = 13
    (2 964) the first on the deferred-LayerNorm loop -- each against the oracle at 5e-2, the route proven by comparing with
    the `deferred_ln = False` run (equal below the threshold, different from it on)."""
    from oracle.modeling import BertImgModelwithLocationEmbeds as OTrunk
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT, BertImgModelwithLocationEmbeds
    from visitron_amd.synth import make_batch

    cfg = BertConfig(num_hidden_layers=3, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref, prod = model_pair(OTrunk, BertImgModelwithLocationEmbeds, cfg, seed=2, device=dev)
    enc = prod.encoder
    enc.deferred_ln_min_rows = DEFERRED_LN_MIN_ROWS_DEFAULT
    b = make_batch(cfg, B, seed=5 + B, with_labels=False)
    kw = {k: b[k] for k in ("input_ids", "token_type_ids", "attention_mask", "img_feats", "img_location_embeddings") if k in b}
    rows = b["attention_mask"].numel()
    assert rows == B * 228 and (rows >= DEFERRED_LN_MIN_ROWS_DEFAULT) is deferred
    assert enc.serves_deferred_ln(rows=rows) is deferred
    dkw = {k: v.to(dev) for k, v in kw.items()}
    with torch.no_grad():
        want = ref(**kw)
        got = prod(**dkw)
        enc.deferred_ln = False
        seven = prod(**dkw)
        enc.deferred_ln = True
    check_close("threshold B=%d x 228 sequence_output (%s)%s" % (B, "deferred loop" if deferred else SEVEN, SHIPPED_SUFFIX),
                got[0], want[0], TOL)
    check_close("threshold B=%d x 228 pooled_output (%s)%s" % (B, "deferred loop" if deferred else SEVEN, SHIPPED_SUFFIX),
                got[1], want[1], TOL)
    assert torch.equal(got[0], seven[0]) is (not deferred) and torch.equal(got[1], seven[1]) is (not deferred)


def _ragged(B, T, R, full):
    """keep [B, T + R]: the first `full` sequences whole, the others cycling through ragged text / region lengths down to one
    token (position 0 of every sequence is kept; a sequence may have no region at all)."""
    lt, lr = [T, 33, 17, 2, 1], [R, 0, 5, R, 1]
    lens_t = torch.tensor([T if i < full else lt[i % 5] for i in range(B)])
    lens_r = torch.tensor([R if i < full else lr[i % 5] for i in range(B)])
    return torch.cat([torch.arange(T)[None, :] < lens_t[:, None], torch.arange(R)[None, :] < lens_r[:, None]], 1)


@pytest.mark.parametrize("B,full,deferred", [(56, 10, False), (64, 52, True)])
def test_the_compacted_row_count_picks_the_layer_loop(dev, B, full, deferred):
    """run_trunk(keep=...) -- the rollout's eval forward on the rows that exist: SeqLayout.rows, not the padded B x S, is
    what the rule sees.  B = 56 x 52 = 2 912 padded rows of which 1 679 are kept: the seven-launch layer on compacted rows;
    B = 64 with 52 whole sequences: 2 986 kept rows, the deferred loop.  Each against the oracle's masked forward at the
    kept positions (flat 5e-2) and against the padded masked run of the same inputs on the SAME loop (absent keys against
    keys at -10000: one bf16 rounding step of the largest outputs apart -- the bound of
    test_compacted_rows_run_the_deferred_layernorm_loop, tests/test_gpu_round4.py); the route proven by the
    `deferred_ln = False` run.  Text + regions, ragged lengths down to one token."""
    from oracle.modeling import BertImgModelwithLocationEmbeds as OTrunk
    from visitron_amd.config import BertConfig
    from visitron_amd.modeling import DEFERRED_LN_MIN_ROWS_DEFAULT, BertImgModelwithLocationEmbeds
    from visitron_amd.synth import make_batch

    cfg = BertConfig(num_hidden_layers=3, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref, prod = model_pair(OTrunk, BertImgModelwithLocationEmbeds, cfg, seed=8, device=dev, weight_std=0.03)
    enc = prod.encoder
    enc.deferred_ln_min_rows = DEFERRED_LN_MIN_ROWS_DEFAULT
    T, R = 40, 12
    b = make_batch(cfg, B, text_len=T, region_len=R, seed=31 + B)
    keep = _ragged(B, T, R, full)
    kept = int(keep.sum())
    assert B * (T + R) >= DEFERRED_LN_MIN_ROWS_DEFAULT and (kept >= DEFERRED_LN_MIN_ROWS_DEFAULT) is deferred, (B * (T + R), kept)
    assert enc.serves_deferred_ln(rows=kept) is deferred and enc.serves_deferred_ln(rows=B * (T + R)) is True
    mask = keep.to(torch.int64)
    args = dict(input_ids=b["input_ids"], img_feats=b["img_feats"], img_location_embeddings=b["img_location_embeddings"])
    dargs = {k: v.to(dev) for k, v in args.items()}

    def compacted():
        outs, pooled, _, _, _ = prod.run_trunk(dargs["input_ids"], img_feats=dargs["img_feats"],
                                               img_location_embeddings=dargs["img_location_embeddings"], keep=keep.to(dev))
        lay = prod._last_layout
        assert lay.rows == kept
        return outs[-1][:lay.rows].float().cpu(), pooled.float().cpu()

    with torch.no_grad():
        want, want_pooled = ref(attention_mask=mask, **args)[:2]
        got_c, pooled_c = compacted()
        enc.deferred_ln = False
        got_7, pooled_7 = compacted()
        enc.deferred_ln = deferred            # the padded run on the loop the compacted one took
        padded = prod(attention_mask=mask.to(dev), **dargs)
        enc.deferred_ln = True
    H = cfg.hidden_size
    want_rows = want.reshape(-1, H)[keep.reshape(-1)]
    how = "deferred loop" if deferred else SEVEN
    assert (torch.equal(got_c, got_7) and torch.equal(pooled_c, pooled_7)) is (not deferred)
    print("ROUTE %d kept of %d padded rows: %s" % (kept, B * (T + R), how))
    check_close("compacted %d of %d rows sequence_output (%s)%s" % (kept, B * (T + R), how, SHIPPED_SUFFIX), got_c, want_rows, TOL)
    check_close("compacted %d of %d rows pooled_output (%s)%s" % (kept, B * (T + R), how, SHIPPED_SUFFIX), pooled_c, want_pooled, TOL)
    e_p = maxabs(padded[0].reshape(-1, H).float().cpu()[keep.reshape(-1)], got_c)
    bound_p = max(2e-2, float(want_rows.abs().max()) * 2.0 ** -7)
    print("compacted against padded (%s): %.3e, bound %.3e" % (how, e_p, bound_p))
    assert e_p <= bound_p


# ---- C.4: every plain GEMM candidate through a whole seven-launch forward ------------------------------------------------
def _unsupported(err):
    from visitron_amd import _lib

    return "(code %d)" % _lib.VT_ERR_UNSUPPORTED in str(err)


def _candidates():
    from visitron_amd import ops

    return list(ops.GEMM_CANDIDATES)


@pytest.mark.parametrize("variant", _candidates())
def test_every_gemm_candidate_through_the_seven_launch_forward(dev, base_model, variant):
    """The kernel that serves a model-level forward is the autotuner's pick on the box at hand.  Here every plain GEMM
    candidate in turn is forced on all the GEMMs of the 12-layer base model's eval forward at the shipped threshold --
    configs[0] (2 x 228 rows) and the shipped pretrain batch (2 x 767) -- and the sequence output, the pooled output and the
    three heads are held to the reference's outputs at 5e-2.  A candidate the library refuses for one of the GEMMs
    (VT_ERR_UNSUPPORTED: the split-K variant has nothing to split on the 30 522-wide decoder) is listed, and that part runs
    on the automatic choice."""
    from test_gpu_reference_fixtures import _base
    from visitron_amd import ops

    refused = []
    for fname, T, R, seed, tag in (("ref_base_cfg0.npz", 128, 100, 1234, "golden base cfg1"),
                                   ("ref_shipped_s767.npz", 511, 256, 767, "ref shipped S=767")):
        g, cfg, b, m = _base(dev, fname, 2, T, R, seed, base_model)
        S = T + R
        st = int(g["seq_stride"][0])
        route = Route(shipped=True)
        route.apply(m)
        route.suffix = "%s [GEMM %d]" % (SHIPPED_SUFFIX, variant)
        trunk = lambda: m.bert.run_trunk(b["input_ids"], attention_mask=b["attention_mask"], img_feats=b["img_feats"],
                                         img_location_embeddings=b["img_location_embeddings"])[:2]
        with torch.no_grad():
            ops.force_gemm_variant(variant)
            try:
                try:
                    outs, pooled = route.call(m, 2 * S, trunk)
                except RuntimeError as e:
                    if not _unsupported(e):
                        raise
                    refused.append("%s trunk" % tag)
                    continue
                try:
                    scores, tokp, act = m.head_outputs(outs[-1], pooled)
                    torch.cuda.synchronize()
                except RuntimeError as e:
                    if not _unsupported(e):
                        raise
                    refused.append("%s heads" % tag)
                    ops.force_gemm_variant(None)
                    scores, tokp, act = m.head_outputs(outs[-1], pooled)
            finally:
                ops.force_gemm_variant(None)
        assert route.proven == [(2 * S, SEVEN)]
        route.check("%s sequence_output slice" % tag, outs[-1].float().cpu().view(2, S, -1)[:, ::st, ::31], g["sequence_output_slice"], TOL)
        route.check("%s pooled_output" % tag, pooled, g["pooled_output"], TOL)
        route.check("%s prediction_scores slice" % tag, scores.float().cpu().view(2, S, -1)[:, ::st, ::1009],
                    g["prediction_scores_slice"], TOL)
        route.check("%s token_probs slice" % tag, tokp.float().cpu().view(2, S, -1)[:, ::st, ::97], g["token_probs_slice"], TOL)
        route.check("%s action_scores" % tag, act, g["action_scores"], TOL)
    print("GEMM %d refused by the library for: %s" % (variant, ", ".join(refused) or "nothing"))
    assert not any(r.endswith("trunk") for r in refused), refused     # every candidate serves the layer's GEMMs at these shapes


# ---- C.5: the fuzz seeds' inference half ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(24)))
def test_random_shapes_inference_on_the_shipped_route(dev, seed):
    """tests/test_gpu_fuzz.py's shapes, weights, masks and bounds (its one-argmax allowance on the accuracies included):
    trunk outputs and the eval 7-tuple against the oracle, on the seven-launch layer every one of these forwards takes for
    a user (at most 9 x 100 rows)."""
    from oracle.modeling import PreTrainOscar as OModel
    from test_gpu_fuzz import TRUNK_KEYS, _case, _close_or_both_nan
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar

    cfg = mini_config(num_hidden_layers=2 + seed % 2, use_img_layernorm=bool(seed % 2), img_layer_norm_eps=1e-12)
    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=50 + seed, device=dev, weight_std=0.03)
    route = Route(shipped=True)
    route.apply(prod)
    b, shape = _case(cfg, seed)
    bd = {k: v.to(dev) for k, v in b.items()}
    rows = b["attention_mask"].numel()
    tag = "fuzz %02d B%d T%d R%d mask%d" % ((seed,) + shape)
    trunk = {k: b[k] for k in TRUNK_KEYS if k in b}
    with torch.no_grad():
        want = ref.bert(**trunk)
        got = route.call(prod, rows, lambda: prod.bert(**{k: bd[k] for k in trunk}))
    route.check(tag + " sequence_output", got[0], want[0], 5e-2)
    route.check(tag + " pooled_output", got[1], want[1], 5e-2)
    if "img_feats" not in b:
        assert _routes(route) == [SEVEN]
        return                                      # PreTrainOscar's callers always pass regions
    with torch.no_grad():
        want7 = ref(**b)
        got7 = route.call(prod, rows, lambda: tuple(torch.as_tensor(x, dtype=torch.float32) for x in prod(**bd)))
    n_sup = {4: int((b["labels"] != -1).sum()), 5: int(b["next_action"].shape[0]), 6: int((b["token_labels"] != -1).sum())}
    tol7 = lambda i: 5e-2 if i < 4 else 1.0 / max(n_sup[i], 1) + 1e-6
    for i in range(7):
        print("PARITY %s tuple7[%d]%s got %.6f want %.6f bound %.3e" % (tag, i, SHIPPED_SUFFIX, float(got7[i]), float(want7[i]), tol7(i)))
        assert _close_or_both_nan(got7[i], want7[i], tol7(i)), (tag, i, float(got7[i]), float(want7[i]))
    assert _routes(route) == [SEVEN] * 2
