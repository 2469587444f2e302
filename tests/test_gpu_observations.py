"""GPU: the observation gather (csrc/observations.hip through visitron_amd.ops and visitron_amd.observations.FeatureStore)
against the numpy restatement of tests/helpers_observations.py, under its comparison: image and view-angle parts equal bit for
bit, device-computed angles within one fp32 ulp (equal at angle 0), lengths and mask equal.  The store lies inside a NaN-filled
buffer and every output is a view inside a sentinel-filled buffer whose surroundings must stay untouched and whose inside
must be fully written.  Shapes are the smallest at which each mechanism can go wrong."""
import math
import os

import numpy as np
import pytest
import torch

import helpers_observations as ho
import helpers_turn_based as ht

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("slots", "view_index", "heading", "elevation", "cand_point", "cand_heading", "cand_elevation", "cand_count")
PAD = 64          # floats around every view: a multiple of 4, so the views keep the 16-byte alignment of the vector path
SENTINEL = -7.25
WORST = {"ulp": 0}


def _inside(shape, dtype, dev, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + n].view(*shape)


def _untouched(buf, n, fill):
    head, tail = buf[:PAD], buf[PAD + n:]
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == fill).all()) and bool((tail == fill).all())


def _nan_store(store, dev):
    buf, view = _inside(store.shape, torch.float32, dev, float("nan"))
    view.copy_(torch.from_numpy(store))
    return buf, view


def _inputs(N, D, slots, views, counts, seed, angle=True):
    """Synthetic step: candidate views walk down from 35, angles from a generator (0 everywhere with angle=False)."""
    rng = np.random.RandomState(seed)
    B = len(slots)
    a = (lambda n: rng.uniform(-4.0, 8.0, n)) if angle else (lambda n: np.zeros(n))
    return dict(store=ho.make_store(N, D, seed), table=ho.closed_form_table(), slots=np.array(slots),
                view_index=np.array(views), heading=a(B), elevation=a(B),
                cand_point=[[(35 - 7 * j - b) % 36 for j in range(c)] for b, c in enumerate(counts)],
                cand_heading=[list(a(c)) for c in counts], cand_elevation=[list(a(c)) for c in counts],
                cand_count=np.array(counts))


def _gather(inp, dev):
    """ops.obs_gather on a NaN-surrounded store into sentinel-surrounded outputs -> the five outputs as numpy."""
    from visitron_amd import observations, ops

    N, V, D = inp["store"].shape
    B = len(inp["slots"])
    Cmax = max(0, int(np.max(inp["cand_count"]))) + 1
    sbuf, store = _nan_store(inp["store"], dev)
    host = np.zeros(ops.obs_record_bytes(B, Cmax)[0], dtype=np.uint8)
    assert observations.pack_record(host, *[inp[k] for k in FIELDS])[:2] == (B, Cmax)
    record = torch.from_numpy(host).to(dev)
    shapes = ((B, 4), (B, V, D + 4), (B, Cmax, D + 4), (B,), (B, Cmax))
    fills = (SENTINEL, SENTINEL, SENTINEL, -77, 0xEE)
    dtypes = (torch.float32, torch.float32, torch.float32, torch.int32, torch.uint8)
    bufs, outs = zip(*[_inside(s, dt, dev, f) for s, dt, f in zip(shapes, dtypes, fills)])
    outs = list(outs)
    outs[4] = outs[4].view(torch.bool)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.obs_gather(store, torch.from_numpy(inp["table"]).to(dev), record, B, Cmax, out=tuple(outs), err_flag=err)
    torch.cuda.synchronize()
    for buf, s, f, name in zip(bufs, shapes, fills, ("input_a_t", "f_t", "candidate_feat", "candidate_leng", "candidate_mask")):
        assert _untouched(buf, int(np.prod(s)), f), name + ": written outside the view"
    assert _untouched(sbuf, inp["store"].size, float("nan")) and bool(torch.equal(store.cpu(), torch.from_numpy(inp["store"])))
    got = [o.cpu().numpy() for o in outs[:4]] + [bufs[4][PAD:PAD + B * Cmax].view(B, Cmax).cpu().numpy()]
    for g, f, name in zip(got[:3], fills, ("input_a_t", "f_t", "candidate_feat")):
        assert not bool((g == f).any()) and bool(np.isfinite(g).all()), name + ": an element was left unwritten"
    assert not bool((got[3] == -77).any()) and set(np.unique(got[4])) <= {0, 1}
    return tuple(got), int(err.item())


def _check(got, inp):
    failed, worst = ho.compare(got, inp)
    WORST["ulp"] = max(WORST["ulp"], worst)
    print("OBS worst angle deviation %d ulp" % worst)
    assert failed == [], failed


# D = 8: vector path, one piece per lane and idle lanes; 260: 65 pieces, lane 0 alone on the second round; 2048: the shipped
# width, 8 rounds in one group; 6, 7: element path with 8-byte and 4-byte row starts
D_VALUES = [8, 260, 2048, 6, 7]


@pytest.mark.parametrize("D", D_VALUES)
def test_panoramic_gather_at_every_width(dev, D):
    inp = _inputs(3, D, [2, 0, 1, 0, 2], [0, 13, 35, 7, 24], [0, 1, 3, 0, 2], seed=D)
    got, err = _gather(inp, dev)
    assert err == 0
    _check(got, inp)


@pytest.mark.parametrize("D", D_VALUES)
def test_view_gather_at_every_width(dev, D):
    from visitron_amd import ops

    store_np = ho.make_store(3, D, 100 + D)
    sbuf, store = _nan_store(store_np, dev)
    slots, views = [2, 0, 1, 0, 2, 1], [0, 35, 13, 35, 7, 24]
    rows = torch.tensor(list(zip(slots, views)), dtype=torch.int32, device=dev)
    buf, out = _inside((6, D), torch.float32, dev, SENTINEL)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.obs_gather_view(store, rows, 6, out=out, err_flag=err)
    torch.cuda.synchronize()
    assert _untouched(buf, 6 * D, SENTINEL) and _untouched(sbuf, store_np.size, float("nan")) and int(err.item()) == 0
    want = store_np[slots, views]
    assert bool((out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())
    # a strided destination (rows of a wider block) keeps its neighbours
    wide = torch.full((6, D + 12), SENTINEL, device=dev)
    ops.obs_gather_view(store, rows, 6, out=wide[:, 4:4 + D])
    assert bool((wide[:, 4:4 + D].cpu().numpy().view(np.uint32) == want.view(np.uint32)).all())
    assert bool((wide[:, :4] == SENTINEL).all()) and bool((wide[:, 4 + D:] == SENTINEL).all())
    # one bad slot, one bad view: those rows are zero, the others right, the flag is raised
    bad = torch.tensor([[2, 0], [3, 1], [1, 36], [0, -1], [-1, 0], [1, 24]], dtype=torch.int32, device=dev)
    buf, out = _inside((6, D), torch.float32, dev, SENTINEL)
    ops.obs_gather_view(store, bad, 6, out=out, err_flag=err)
    got = out.cpu().numpy()
    assert int(err.item()) == 1 and _untouched(buf, 6 * D, SENTINEL) and not got[1:5].any()
    assert np.array_equal(got[0], store_np[2, 0]) and np.array_equal(got[5], store_np[1, 24])


@pytest.mark.parametrize("name,slots,views,counts", [
    ("one agent", [1], [35], [2]),
    ("two agents on one slot", [2, 0, 1, 0, 2], [5, 6, 7, 8, 9], [1, 1, 1, 1, 1]),
    ("a permutation of the slots", [2, 0, 1], [11, 12, 23], [2, 0, 1]),
    ("only END rows", [0, 1, 2], [0, 1, 2], [0, 0, 0]),
    ("ragged 0 / 1 / 3", [0, 1, 2, 1], [3, 2, 1, 0], [0, 1, 3, 0]),
])
@pytest.mark.parametrize("D", [8, 7])
def test_batches_and_candidate_counts(dev, D, name, slots, views, counts):
    inp = _inputs(3, D, slots, views, counts, seed=len(slots) + sum(counts))
    got, err = _gather(inp, dev)
    assert err == 0 and got[2].shape[1] == max(counts) + 1
    _check(got, inp)


@pytest.mark.parametrize("D", [8, 7])
def test_maximal_view_and_candidate_view(dev, D):
    inp = _inputs(3, D, [2, 2], [35, 35], [2, 1], seed=3)
    inp["cand_point"] = [[35, 0], [35]]
    got, err = _gather(inp, dev)
    assert err == 0
    _check(got, inp)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_observations.npz")))


def _store_from(inp, dev, keys=None):
    from visitron_amd import FeatureStore

    keys = keys or ho.keys_for(inp["store"].shape[0])
    return FeatureStore((keys, inp["store"]), dev, view_angle_table=inp["table"]), keys


def _np(out):
    a_t, f_t, cand, leng, mask = out
    return a_t.cpu().numpy(), f_t.cpu().numpy(), cand.cpu().numpy(), np.array(leng), mask.cpu().numpy()


def test_reference_fixture(dev, fx):
    """The fixture's inputs reproduce what the reference's Agent.get_input_feat and length2mask returned."""
    inp = {k: fx[k] for k in ("store", "table") + FIELDS}
    store, keys = _store_from(inp, dev, [str(k) for k in fx["keys"]])
    obs = ho.make_obs(ho.synthetic_inputs(), keys, garbage=True)
    out = store.get_input_feat(obs)
    assert len(out) == 4 and out[3] == [int(x) for x in fx["candidate_leng"]]
    got = _np(out + (store.last_candidate_mask,))
    _check(got, inp)
    worst = 0
    for name, g in zip(("input_a_t", "f_t", "candidate_feat"), got):
        assert g.shape == fx[name].shape
        d = ho.ulp_distance(g, fx[name])
        worst = max(worst, int(d.max()))
    assert worst <= 1                                            # against the reference's own numbers
    assert np.array_equal(got[4], fx["candidate_mask"]) and got[4].dtype == np.bool_
    direct = store.step_inputs(*[inp[k] for k in FIELDS])        # 2-D padded candidate arrays, as the fixture stores them
    for a, b in zip(_np(direct), got):
        assert np.array_equal(a, b)
    import visitron_amd

    visitron_amd.check_errors()


@pytest.mark.parametrize("what", ["slot", "slot_negative", "view_index", "cand_point", "cand_count"])
def test_a_bad_index_zeroes_its_row_and_raises_once(dev, what):
    import visitron_amd

    inp = ho.synthetic_inputs(D=8, N=3, seed=9)
    inp["slots"] = np.array([2, 0, 1, 0, 2])
    store, _ = _store_from(inp, dev)
    visitron_amd.check_errors()
    row = 3
    if what == "slot":
        inp["slots"][row] = 3
    elif what == "slot_negative":
        inp["slots"][row] = -1
    elif what == "view_index":
        inp["view_index"][row] = 36
    elif what == "cand_point":
        inp["cand_point"][row] = [12, 36, 23]
    else:
        inp["cand_count"][row] = -1
    got, err = _gather(inp, dev)                                 # NaN / sentinel surroundings: no access leaves the buffers
    assert err == 1 and not got[0][row].any() and not got[1][row].any() and not got[2][row].any()
    _check(got, inp)                                             # the restatement zeroes the same row; every other row is right
    raised = 0
    try:
        store.step_inputs(*[inp[k] for k in FIELDS])             # the flag may already land at the end of this call
    except IndexError:
        raised += 1
    try:
        visitron_amd.check_errors()
    except IndexError:
        raised += 1
    assert raised == 1
    visitron_amd.check_errors()                                  # reported once


def test_staging_ring(dev):
    """Three calls back to back with different records and no synchronisation in between each return their own result (the
    third rewrites the first pinned slot behind its event); a fourth and a fifth call after them reuse both slots again."""
    inps = [_inputs(3, 8, [b % 3 for b in range(k, k + 4)], [5 * k + b for b in range(4)], [k % 3, 1, (k + 1) % 3, 2], seed=40 + k)
            for k in range(4)]
    store, _ = _store_from(inps[0], dev)
    for k in range(1, 4):
        inps[k]["store"] = inps[0]["store"]
    outs = [store.step_inputs(*[inps[k][f] for f in FIELDS]) for k in range(3)]
    buffers = [b.data_ptr() for b in store._stage.bufs]
    assert store._stage.turn == 1 and len(set(buffers)) == 2
    outs.append(store.step_inputs(*[inps[3][f] for f in FIELDS]))
    assert store._stage.turn == 0
    views = store.view_features([0, 2, 1], [35, 0, 17])          # the view records share the ring
    assert store._stage.turn == 1 and [b.data_ptr() for b in store._stage.bufs] == buffers
    torch.cuda.synchronize()
    for k in range(4):
        _check(_np(outs[k]), inps[k])
    assert np.array_equal(views.cpu().numpy(), inps[0]["store"][[0, 2, 1], [35, 0, 17]])
    assert all(e.query() for e in store._stage.events)


def test_upload_in_chunks(dev, monkeypatch):
    from visitron_amd import FeatureStore, observations

    s = ho.make_store(7, 8, 1)
    monkeypatch.setattr(observations, "UPLOAD_CHUNK_BYTES", 3 * 36 * 8 * 4)      # 3 slots per chunk: 3 + 3 + 1
    keys = ho.keys_for(7)
    for features in ((keys, s), {k: s[i] for i, k in enumerate(keys)}, (keys, torch.from_numpy(s))):
        store = FeatureStore(features, dev)
        assert store.features.is_cuda and np.array_equal(store.features.cpu().numpy(), s) and store.nbytes == s.nbytes


# ---- composition with the decoders -------------------------------------------------------------------------------------------
def test_panoramic_decoder_fed_from_the_store(dev):
    """At the decoder sizes of tests/test_gpu_rollout.py with angle 0 everywhere (every input bit-equal), rollout.AttnDecoderLSTM
    fed from store.get_input_feat(obs) returns bitwise what it returns fed from the host-built tensors; then the loop's
    masked_fill_ + CrossEntropyLoss(ignore_index) + max(1) against rollout.action_feedback."""
    from visitron_amd import rollout

    ang, emb, hs, D = 4, 64, 512, 2048
    torch.manual_seed(4)
    dec = rollout.AttnDecoderLSTM(ang, emb, hs, 0.5, feature_size=D + ang).eval().to(dev)
    inp = _inputs(3, D, [2, 0, 1, 0, 2], [0, 13, 35, 7, 24], [2, 1, 3, 0, 2], seed=77, angle=False)
    inp["store"] = (inp["store"] % 1.0).astype(np.float32) * 0.3            # the feature scale of that test
    store, keys = _store_from(inp, dev)
    a_t, f_t, cand, leng = store.get_input_feat(ho.make_obs(inp, keys, with_feature=False))
    mask = store.last_candidate_mask
    host = ho.restate(inp)
    h_at, h_ft, h_cand = (torch.from_numpy(x).to(dev) for x in host[:3])
    assert torch.equal(a_t, h_at) and torch.equal(f_t, h_ft) and torch.equal(cand, h_cand) and leng == list(host[3])
    assert torch.equal(mask.cpu(), torch.from_numpy(host[4]))
    B, L = 5, 20
    g = torch.Generator().manual_seed(8)
    h1, c0 = (torch.randn(B, hs, generator=g) * 0.3).to(dev), (torch.randn(B, hs, generator=g) * 0.3).to(dev)
    ctx = (torch.randn(B, L, hs, generator=g) * 0.5).to(dev)
    cmask = torch.zeros(B, L, dtype=torch.bool)
    cmask[:, L - 5:] = True
    with torch.no_grad():
        want = dec(h_at, h_ft, h_cand, None, h1, c0, ctx, cmask.to(dev))
        got = dec(a_t, f_t, cand, None, h1, c0, ctx, cmask.to(dev))
    for gi, wi in zip(got, want):
        assert gi.shape == wi.shape and torch.equal(gi, wi)
    logit = got[2]
    assert logit.shape == (B, max(leng))
    target = torch.tensor([1, -100, 3, 0, 2])
    loss, nxt = rollout.action_feedback(logit, target.to(dev), mask, -100, "argmax")
    ref_logit = logit.detach().cpu().double().masked_fill_(torch.from_numpy(host[4]), -math.inf)      # agent.py:396-425
    ref_loss = torch.nn.CrossEntropyLoss(ignore_index=-100)(ref_logit, target)
    _, ref_a = ref_logit.max(1)
    bound = ht.head_reference(logit.detach().cpu(), target, torch.from_numpy(host[4])).loss_bound
    print("OBS action_feedback loss err %.3e bound %.3e" % (abs(float(loss) - float(ref_loss)), bound))
    assert abs(float(loss) - float(ref_loss)) <= bound
    assert torch.equal(nxt.cpu(), ref_a)


def test_turn_based_decoder_fed_from_view_features(dev):
    from visitron_amd import turn_based

    D, hs = 70, 128
    torch.manual_seed(6)
    dec = turn_based.AttnDecoderLSTM(8, 6, 8, hs, 0.0, feature_size=D).eval().to(dev)
    inp = _inputs(3, D, [2, 0, 1, 0, 2], [0, 13, 35, 7, 24], [0] * 5, seed=78)
    store, _ = _store_from(inp, dev)
    feat = store.view_features(inp["slots"], inp["view_index"])
    host = torch.from_numpy(inp["store"][inp["slots"], inp["view_index"]]).to(dev)
    assert feat.shape == (5, D) and torch.equal(feat, host)
    g = torch.Generator().manual_seed(9)
    h0, c0 = (torch.randn(5, hs, generator=g) * 0.3).to(dev), (torch.randn(5, hs, generator=g) * 0.3).to(dev)
    ctx = (torch.randn(5, 9, hs, generator=g) * 0.5).to(dev)
    action = torch.tensor([[1], [0], [5], [7], [2]], device=dev)
    with torch.no_grad():
        want = dec(action, host, h0, c0, ctx)
        got = dec(action, feat, h0, c0, ctx)
    for gi, wi in zip(got, want):
        assert torch.equal(gi, wi)


def test_zz_record_the_worst_angle_deviation(dev):
    """Runs last in this module: what the comparison measured, for profiles/r15/observations.txt."""
    print("OBS worst angle deviation over the module: %d ulp" % WORST["ulp"])
    assert WORST["ulp"] <= 1
