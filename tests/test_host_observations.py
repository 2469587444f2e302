"""CPU: the observation gather's semantics and host side.  The numpy restatement of tests/helpers_observations.py equals what
the reference's own Agent.get_input_feat / length2mask produced (tests/golden/ref_observations.npz), the comparison rejects
every wrong implementation of the table, and FeatureStore's host half (ids, record packing, argument checks) and the
library's argument checks work without a device."""
import ctypes
import os

import numpy as np
import pytest

import helpers_observations as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_observations.npz")
FIELDS = ("slots", "view_index", "heading", "elevation", "cand_point", "cand_heading", "cand_elevation", "cand_count")
OUTPUTS = ("input_a_t", "f_t", "candidate_feat", "candidate_leng", "candidate_mask")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIXTURE))


def fixture_inputs(fx):
    return {k: fx[k] for k in ("store", "table") + FIELDS}


def test_fixture_is_small_and_what_the_issue_describes(fx):
    assert os.path.getsize(FIXTURE) < 100 * 1024
    assert fx["store"].shape[1:] == (36, 10) and list(fx["cand_count"]) == [0, 1, 3, 3, 2]
    angles = np.concatenate([fx["heading"], fx["elevation"], fx["cand_heading"].ravel(), fx["cand_elevation"].ravel()])
    assert (angles == 0).any() and (angles < 0).any() and (angles > 2 * np.pi).any()


def test_restatement_equals_the_reference_bit_for_bit(fx):
    got = ho.restate(fixture_inputs(fx))
    for name, g in zip(OUTPUTS, got):
        w = fx[name]
        assert np.asarray(g).shape == w.shape, name
        if w.dtype == np.float32:
            assert bool((np.ascontiguousarray(g).view(np.uint32) == w.view(np.uint32)).all()), name
        else:
            assert bool((np.asarray(g) == w).all()), name
    failed, worst = ho.compare(tuple(fx[n] for n in OUTPUTS), fixture_inputs(fx))
    assert failed == [] and worst == 0
    # the synthetic inputs of the helper are the fixture's
    inp = ho.synthetic_inputs()
    assert np.array_equal(inp["store"], fx["store"]) and np.array_equal(inp["table"], fx["table"])
    assert list(fx["keys"]) == ho.keys_for(4)


def test_default_view_angle_table_is_the_closed_form():
    from visitron_amd import default_view_angle_table

    t = default_view_angle_table()
    assert t.dtype == np.float32 and t.shape == (36, 36, 4)
    w = ho.closed_form_table()
    assert bool((t.view(np.uint32) == w.view(np.uint32)).all())
    assert t[0, 0].tolist() == [0.0, 1.0, np.float32(-0.5), np.float32(np.sqrt(0.75))]
    assert "simulator" in default_view_angle_table.__doc__


@pytest.mark.parametrize("mutant", sorted(ho.MUTANTS))
def test_wrong_implementations_are_rejected(mutant):
    inp = ho.synthetic_inputs()
    assert ho.compare(ho.restate(inp), inp) == ([], 0)
    failed, _ = ho.compare(ho.restate(inp, mutant), inp)
    assert failed, ho.MUTANTS[mutant]


def test_fp32_sine_is_rejected_by_the_ulp_bound_alone():
    inp = ho.synthetic_inputs()
    failed, worst = ho.compare(ho.restate(inp, "fp32_sinf"), inp)
    assert failed and all("more than one ulp" in f for f in failed) and worst > 100


def test_one_ulp_is_accepted_and_two_are_not():
    inp = ho.synthetic_inputs()
    D = inp["store"].shape[2]
    for steps, ok in ((1, True), (2, False)):
        got = [np.array(g) for g in ho.restate(inp)]
        x = got[2][2, 0, D:D + 1]                       # sin of a candidate heading that is not 0
        for _ in range(steps):
            x[:] = np.nextafter(x, np.float32(2))
        failed, worst = ho.compare(tuple(got), inp)
        assert (failed == []) == ok and worst == steps
    got = [np.array(g) for g in ho.restate(inp)]
    got[2][1, 0, D] = np.float32(1e-45)                 # sin(0) must be 0 exactly
    assert ho.compare(tuple(got), inp)[0] == ["candidate_feat angle part (where it must be equal)"]


# ---- FeatureStore's host half ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_store():
    from visitron_amd import FeatureStore

    inp = ho.synthetic_inputs()
    keys = ho.keys_for(inp["store"].shape[0])
    return FeatureStore({k: inp["store"][i] for i, k in enumerate(keys)}, "cpu"), inp, keys


def test_store_construction_and_ids(cpu_store):
    from visitron_amd import FeatureStore, observations

    store, inp, keys = cpu_store
    assert (store.N, store.V, store.D, store.nbytes) == (4, 36, 10, 4 * 36 * 10 * 4)
    assert np.array_equal(store.features.numpy(), inp["store"])
    assert [store.slot(k) for k in keys] == [0, 1, 2, 3]
    with pytest.raises(KeyError):
        store.slot("scan0_nowhere")
    pair = FeatureStore((keys, inp["store"]), "cpu", view_angle_table=ho.closed_form_table())
    assert np.array_equal(pair.features.numpy(), inp["store"]) and pair.slot(keys[3]) == 3
    assert np.array_equal(store.view_angle_table.numpy(), observations.default_view_angle_table())
    with pytest.raises(ValueError):
        FeatureStore((keys[:3], inp["store"]), "cpu")
    with pytest.raises(ValueError):
        FeatureStore({"a_b": inp["store"][0], "a_c": inp["store"][1][:, :9]}, "cpu")
    with pytest.raises(ValueError):
        FeatureStore((keys, inp["store"]), "cpu", view_angle_table=np.zeros((36, 4), np.float32))
    with pytest.raises(TypeError):
        FeatureStore((keys, inp["store"]), "cpu", view_angle_table=np.zeros((36, 36, 4), np.float64))


def test_record_packing_round_trips_field_for_field():
    from visitron_amd import observations, ops

    inp = ho.synthetic_inputs()
    args = [inp[k] for k in FIELDS]
    nbytes, off = ops.obs_record_bytes(5, 4)
    assert off % 8 == 0 and off >= 12 * 5 + 4 * 5 * 4 and nbytes == off + 8 * (2 * 5 + 2 * 5 * 4)
    buf = np.full(nbytes + 8, 0xAB, dtype=np.uint8)
    assert observations.pack_record(buf[:nbytes], *args) == (5, 4, nbytes)
    assert bool((buf[nbytes:] == 0xAB).all())
    back = observations.unpack_record(buf, 5, 4)
    for name, b, a in zip(FIELDS, back, args):
        if name.startswith("cand_") and name != "cand_count":
            for r in range(5):
                n = int(inp["cand_count"][r])
                assert list(b[r, :n]) == list(a[r]) and not b[r, n:].any(), name
        else:
            assert list(b) == list(a), name
    assert back[2].dtype == np.float64 and back[0].dtype == np.int32 and back[5].dtype == np.float64
    # an odd B * (3 + Cmax): the doubles still start 8-byte aligned
    assert ops.obs_record_bytes(1, 2)[1] == 24 and ops.obs_record_bytes(3, 2)[1] == 64
    # 2-D candidate arrays are accepted as they are
    C = 3
    pts = np.zeros((5, C), dtype=np.int64)
    for r in range(5):
        pts[r, :len(inp["cand_point"][r])] = inp["cand_point"][r]
    buf2 = np.zeros(nbytes, dtype=np.uint8)
    observations.pack_record(buf2, inp["slots"], inp["view_index"], inp["heading"], inp["elevation"], pts,
                             np.zeros((5, C)), np.zeros((5, C)), inp["cand_count"])
    assert np.array_equal(observations.unpack_record(buf2, 5, 4)[4][:, :C], pts)


class _NoFeature(dict):
    def __getitem__(self, k):
        assert k != "feature", "the store must not read ob['feature']"
        return dict.__getitem__(self, k)


def test_get_input_feat_never_reads_feature(cpu_store):
    store, inp, keys = cpu_store
    plain = store.obs_fields(ho.make_obs(inp, keys, with_feature=False))
    garbage = store.obs_fields(ho.make_obs(inp, keys, garbage=True))
    guarded = [_NoFeature(ob, candidate=[_NoFeature(c) for c in ob["candidate"]]) for ob in ho.make_obs(inp, keys, garbage=True)]
    ragged = ("cand_point", "cand_heading", "cand_elevation")

    def plain_lists(fields):
        return [[list(r) for r in g] if name in ragged else list(g) for name, g in zip(FIELDS, fields)]

    assert plain_lists(garbage) == plain_lists(plain) == plain_lists(store.obs_fields(guarded))
    assert plain_lists(plain) == plain_lists([inp[name] for name in FIELDS])
    with pytest.raises(KeyError):
        store.obs_fields([dict(guarded[0], viewpoint="vp99")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a store that is not on a HIP device serves no gather
        store.get_input_feat(guarded)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        store.view_features([0, 1], [3, 4])


def test_shape_and_dtype_mistakes_raise_on_the_host(cpu_store):
    store, inp, _ = cpu_store
    good = {k: inp[k] for k in FIELDS}

    def call(**kw):
        return store.step_inputs(*[dict(good, **kw)[k] for k in FIELDS])

    with pytest.raises(ValueError):
        call(view_index=inp["view_index"][:4])
    with pytest.raises(ValueError):
        call(heading=np.zeros((5, 1)))
    with pytest.raises(TypeError):
        call(slots=inp["slots"].astype(np.float32))
    with pytest.raises(TypeError):
        call(heading=np.array(["a"] * 5))
    with pytest.raises(ValueError):
        call(cand_point=inp["cand_point"][:4])
    with pytest.raises(ValueError):
        call(cand_heading=[[], [0.0], [1.0, 2.0], [1.0, 2.0, 3.0], [1.0, 2.0]])       # agent 2 has 3 candidates
    with pytest.raises(TypeError):
        call(cand_point=[[], [35.0], [4, 17, 30], [12, 0, 23], [9, 2]])
    with pytest.raises(ValueError):
        call(cand_point=np.zeros((5, 2), dtype=np.int64))                             # narrower than max(cand_count)
    with pytest.raises(ValueError):
        call(cand_count=np.zeros((5, 1), dtype=np.int64))
    with pytest.raises(ValueError):
        call(slots=np.array([0, 1, 2, 3, 1 << 40]))
    with pytest.raises(ValueError):
        store.step_inputs([], [], [], [], [], [], [], [])
    with pytest.raises(ValueError):
        store.view_features([0, 1], [0])
    with pytest.raises(TypeError):
        store.view_features([0.5, 1.0], [0, 1])


def test_public_names():
    import visitron_amd
    from visitron_amd import observations, rollout, turn_based

    assert visitron_amd.FeatureStore is observations.FeatureStore
    assert visitron_amd.default_view_angle_table is observations.default_view_angle_table
    assert callable(rollout.action_feedback) and "agent.py:396-425" in rollout.action_feedback.__doc__
    import torch

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rollout.action_feedback(torch.zeros(2, 6), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 6, dtype=torch.bool))
    assert turn_based.action_feedback is not None


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_exports_both_symbols_and_checks_arguments_before_any_launch():
    from visitron_amd import _lib

    lib = _lib.load()
    assert lib.vt_abi_version() >= 20
    for name in ("vt_obs_gather_f32", "vt_obs_gather_view_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    mem = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(mem) + 63) & ~63          # a 64-byte aligned host address: never dereferenced
    p = lambda off=0: ctypes.c_void_p(base + off)

    def gather(**kw):
        a = dict(store=p(), N=3, V=36, D=8, table=p(64), record=p(128), B=2, Cmax=2, a_t=p(256), f_t=p(512), cand=p(1024),
                 leng=p(2048), mask=p(2100), err=None)
        a.update(kw)
        return lib.vt_obs_gather_f32(a["store"], a["N"], a["V"], a["D"], a["table"], a["record"], a["B"], a["Cmax"], a["a_t"],
                                     a["f_t"], a["cand"], a["leng"], a["mask"], a["err"], None)

    assert gather(store=None) == _lib.VT_ERR_NULL
    assert gather(record=None) == _lib.VT_ERR_NULL
    assert gather(table=None) == _lib.VT_ERR_NULL
    assert gather(mask=None) == _lib.VT_ERR_NULL
    assert gather(D=0) == _lib.VT_ERR_BAD_SHAPE
    assert gather(D=-4) == _lib.VT_ERR_BAD_SHAPE
    assert gather(B=0) == _lib.VT_ERR_BAD_SHAPE
    assert gather(Cmax=0) == _lib.VT_ERR_BAD_SHAPE
    assert gather(N=0) == _lib.VT_ERR_BAD_SHAPE
    assert gather(V=0) == _lib.VT_ERR_BAD_SHAPE
    assert gather(store=p(4)) == _lib.VT_ERR_BAD_ALIGN
    assert gather(record=p(132)) == _lib.VT_ERR_BAD_ALIGN
    assert gather(f_t=p(514)) == _lib.VT_ERR_BAD_ALIGN

    def view(**kw):
        a = dict(store=p(), N=3, V=36, D=8, rows=p(64), B=2, out=p(256), ld=8, err=None)
        a.update(kw)
        return lib.vt_obs_gather_view_f32(a["store"], a["N"], a["V"], a["D"], a["rows"], a["B"], a["out"], a["ld"], a["err"], None)

    assert view(store=None) == _lib.VT_ERR_NULL
    assert view(rows=None) == _lib.VT_ERR_NULL
    assert view(out=None) == _lib.VT_ERR_NULL
    assert view(D=0) == _lib.VT_ERR_BAD_SHAPE
    assert view(B=0) == _lib.VT_ERR_BAD_SHAPE
    assert view(ld=7) == _lib.VT_ERR_BAD_SHAPE
    assert view(store=p(8)) == _lib.VT_ERR_BAD_ALIGN
    assert view(out=p(258)) == _lib.VT_ERR_BAD_ALIGN
