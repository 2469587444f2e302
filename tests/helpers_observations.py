"""What the observation gather (visitron_amd/observations.py, csrc/observations.hip) is held to, in numpy.

`restate(inp)` states the semantics of tasks/viewpoint_select/agent.py:186-228 fed by data_loader.py:516-642 over a feature
store: f_t[b, v] = [store[slot_b, v] | table[view_index_b, v]], candidate_feat[b, j] = [store[slot_b, cand_point[b][j]] |
sin, cos of the candidate's heading and elevation] below cand_count[b] and zero from the END row on, candidate_leng =
cand_count + 1, candidate_mask = j > leng - 1, input_a_t = sin, cos of the agent's heading and elevation.  An agent with a bad
index (slot, view, a candidate view below its count, a negative count) has every float output zero.

`compare(got, inp)` is the comparison of both test files:
  * the image part and the view-angle part are a copy and a table lookup: EQUAL, bit for bit (compared as uint32 words, so a
    NaN or a -0.0 in the wrong place shows);
  * the candidate and action angles are computed on the device in float64 and rounded once.  A float64 sin / cos within a few
    float64 ulps of the exact value rounds to the correctly rounded fp32 value or, where the exact value lies within those few
    float64 ulps of a rounding boundary, to its neighbour: at most ONE fp32 unit in the last place from
    float32(math.sin(x)) / float32(math.cos(x)).  Where the angle is 0 the exact values 0 and 1 must come out EQUAL;
  * lengths and mask are integers: EQUAL.
`MUTANTS` lists subtly wrong implementations, each with a note where it hides; the comparison must reject every one."""
import math

import numpy as np

V = 36


def closed_form_table():
    """[36, 36, 4]: [base][view] = sin h, cos h, sin e, cos e, h = (view % 12 - base % 12) 30 deg, e = (view // 12 - 1) 30 deg."""
    t = np.empty((V, V, 4), dtype=np.float32)
    for base in range(V):
        for view in range(V):
            h = (view % 12 - base % 12) * math.radians(30)
            e = (view // 12 - 1) * math.radians(30)
            t[base, view] = [math.sin(h), math.cos(h), math.sin(e), math.cos(e)]
    return t


def make_store(N, D, seed, v=V):
    """Non-negative features (a post-ReLU pool) with all-distinct values, so a row taken from the wrong place never matches."""
    rng = np.random.RandomState(seed)
    s = rng.rand(N, v, D).astype(np.float32) + np.arange(N * v, dtype=np.float32).reshape(N, v, 1)
    return s


def keys_for(N):
    return ["scan%d_vp%02d" % (i % 2, i) for i in range(N)]


# 2 pi + 0.001: fp32 rounding of the argument alone moves sin by hundreds of fp32 ulps (sin x ~ 1e-3, ulp 1.2e-10, argument
# error up to 2.4e-7): the place where an fp32 sinf shows
ABOVE_2PI = 6.2841853071795865


def synthetic_inputs(D=10, N=4, seed=5):
    """B = 5, candidate counts 0, 1, 3, 3, 2; angles include 0, negative values and values above 2 pi; two agents share a
    slot; no candidate view equals its column; heading differs from elevation everywhere but at 0."""
    return dict(
        store=make_store(N, D, seed), table=closed_form_table(),
        slots=np.array([2, 0, 3, 0, 1]), view_index=np.array([0, 13, 35, 7, 24]),
        heading=np.array([0.0, -1.3, ABOVE_2PI, 2.5, 7.9]),
        elevation=np.array([0.0, -math.radians(30), math.radians(30), 0.0, -0.1]),
        cand_point=[[], [35], [4, 17, 30], [12, 0, 23], [9, 2]],
        cand_heading=[[], [0.0], [-2.75, ABOVE_2PI, 0.4], [9.1, -0.001, 3.0], [1.0, 6.9]],
        cand_elevation=[[], [0.0], [0.5, -0.5, 0.0], [-0.2, 0.3, 12.7], [-1.0, 0.25]],
        cand_count=np.array([0, 1, 3, 3, 2]))


def make_obs(inp, keys, with_feature=True, garbage=False):
    """The reference's observation dicts for these inputs.  `feature` entries are built as data_loader.py:566,595,620 build
    them (with_feature), or filled with garbage of the right shape, or left out."""
    store, table = inp["store"], inp["table"]
    D = store.shape[2]
    obs = []
    for b in range(len(inp["slots"])):
        slot = int(inp["slots"][b])
        scan, vp = keys[slot].split("_")
        cands = []
        for j in range(int(inp["cand_count"][b])):
            h, e = float(inp["cand_heading"][b][j]), float(inp["cand_elevation"][b][j])
            c = {"pointId": int(inp["cand_point"][b][j]), "heading": h, "elevation": e, "scanId": scan,
                 "viewpointId": "next%d" % j, "idx": j + 1}
            if garbage:
                c["feature"] = np.full(D + 4, np.nan, dtype=np.float32)
            elif with_feature:
                ang = np.array([math.sin(h), math.cos(h), math.sin(e), math.cos(e)], dtype=np.float32)
                c["feature"] = np.concatenate((store[slot, c["pointId"]], ang), -1)
            cands.append(c)
        ob = {"scan": scan, "viewpoint": vp, "viewIndex": int(inp["view_index"][b]), "heading": float(inp["heading"][b]),
              "elevation": float(inp["elevation"][b]), "candidate": cands}
        if garbage:
            ob["feature"] = np.full((V, D + 4), np.nan, dtype=np.float32)
        elif with_feature:
            ob["feature"] = np.concatenate((store[slot], table[ob["viewIndex"]]), -1)
        obs.append(ob)
    return obs


def _angle(h, e, fn=(math.sin, math.cos)):
    return [fn[0](h), fn[1](h), fn[0](e), fn[1](e)]


def _sinf(x):
    return float(np.sin(np.float32(x)))


def _cosf(x):
    return float(np.cos(np.float32(x)))


# name -> where it hides
MUTANTS = {
    "end_row_not_zeroed": "only in row cand_count[b] of candidate_feat; every counted row and the mask are right",
    "padding_unwritten": "only in rows past the END row of the shorter agents (left at what the buffer held)",
    "mask_off_by_one": "one entry per row, at j = cand_count[b]: the END action becomes unselectable",
    "sin_cos_swapped": "in the 4-float tail of candidate rows only; invisible at angles where sin = cos",
    "heading_elevation_swapped": "in the tail of candidate rows and input_a_t; invisible where heading = elevation (both 0)",
    "table_transposed": "in the tail of f_t only: table[view][base]; the elevation half is right on the diagonal band",
    "candidate_at_column": "image part of candidate rows: view j instead of cand_point[b][j]; right wherever they coincide",
    "slot_of_previous_row": "every image part of agent b comes from agent b - 1's slot; right where neighbours share a slot",
    "tail_at_d_minus_4": "the angle tail lands on the last 4 image columns, the true tail keeps what the buffer held",
    "fp32_sinf": "the angles evaluated in fp32: within one ulp at most arguments, hundreds of ulps just above 2 pi",
}


def restate(inp, mutant=None, fill=-7.25):
    """-> (input_a_t [B, 4], f_t [B, 36, D+4], candidate_feat [B, Cmax, D+4], candidate_leng int [B], candidate_mask bool
    [B, Cmax]).  `fill` is what an unwritten element holds (mutants that skip writes)."""
    assert mutant is None or mutant in MUTANTS
    store, table = inp["store"], inp["table"]
    N, v_, D = store.shape
    slots, views, counts = (np.asarray(inp[k]) for k in ("slots", "view_index", "cand_count"))
    B = len(slots)
    Cmax = max(0, int(counts.max())) + 1
    a_t = np.zeros((B, 4), dtype=np.float32)
    f_t = np.zeros((B, v_, D + 4), dtype=np.float32)
    cand = np.zeros((B, Cmax, D + 4), dtype=np.float32)
    if mutant in ("padding_unwritten", "tail_at_d_minus_4"):
        cand[:] = fill
    if mutant == "tail_at_d_minus_4":
        f_t[:] = fill
    leng = np.clip(counts, 0, Cmax - 1) + 1
    fn = (_sinf, _cosf) if mutant == "fp32_sinf" else (math.sin, math.cos)
    if mutant == "sin_cos_swapped":
        fn = (math.cos, math.sin)
    tail = slice(D - 4, D) if mutant == "tail_at_d_minus_4" else slice(D, D + 4)
    for b in range(B):
        n = int(counts[b])
        bad = not (0 <= slots[b] < N and 0 <= views[b] < v_ and 0 <= n < Cmax)
        bad = bad or any(not 0 <= int(p) < v_ for p in inp["cand_point"][b][:max(n, 0)])
        if bad:
            cand[b] = 0.0
            f_t[b] = 0.0
            continue
        slot = int(slots[b - 1]) if (mutant == "slot_of_previous_row" and b > 0) else int(slots[b])
        h, e = float(inp["heading"][b]), float(inp["elevation"][b])
        a_t[b] = _angle(e, h, fn) if mutant == "heading_elevation_swapped" else _angle(h, e, fn)
        f_t[b, :, :D] = store[slot]
        f_t[b, :, tail] = table[:, views[b]] if mutant == "table_transposed" else table[views[b]]
        for j in range(n):
            p = j if mutant == "candidate_at_column" else int(inp["cand_point"][b][j])
            ch, ce = float(inp["cand_heading"][b][j]), float(inp["cand_elevation"][b][j])
            cand[b, j, :D] = store[slot, p]
            cand[b, j, tail] = _angle(ce, ch, fn) if mutant == "heading_elevation_swapped" else _angle(ch, ce, fn)
        if mutant == "end_row_not_zeroed":
            cand[b, n] = cand[b, n - 1] if n > 0 else f_t[b, 0]
        if mutant != "padding_unwritten":
            cand[b, n + (mutant == "end_row_not_zeroed"):] = 0.0
        else:
            cand[b, n] = 0.0
    j = np.arange(Cmax)[None, :]
    mask = (j >= leng[:, None] - 1) if mutant == "mask_off_by_one" else (j > leng[:, None] - 1)
    return a_t, f_t, cand, leng, mask


def ulp_distance(a, b):
    """Distance in fp32 units in the last place between two finite float32 arrays (ordered-integer difference)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def compare(got, inp):
    """got = the five outputs as numpy arrays -> (list of what failed, worst angle deviation in fp32 ulps)."""
    a_t, f_t, cand, leng, mask = got
    w_at, w_ft, w_cand, w_leng, w_mask = restate(inp)
    D = inp["store"].shape[2]
    failed = []
    if not _bits_equal(f_t[..., :D], w_ft[..., :D]):
        failed.append("f_t image part")
    if not _bits_equal(f_t[..., D:], w_ft[..., D:]):
        failed.append("f_t view-angle part")
    if not _bits_equal(cand[..., :D], w_cand[..., :D]):
        failed.append("candidate_feat image part")
    if list(np.asarray(leng).reshape(-1)) != list(w_leng):
        failed.append("candidate_leng")
    if np.asarray(mask).shape != w_mask.shape or not bool((np.asarray(mask).astype(bool) == w_mask).all()):
        failed.append("candidate_mask")
    worst = 0
    counts = np.asarray(inp["cand_count"])
    live = np.arange(w_cand.shape[1])[None, :] < counts[:, None]          # rows whose tail is a computed angle
    live &= np.abs(w_cand[..., D:]).sum(-1) > 0                           # (a bad agent's rows are zero: exact)
    exact_zero_angle = np.zeros(w_cand.shape[:2] + (4,), dtype=bool)
    for b in range(len(counts)):
        for j in range(max(int(counts[b]), 0)):
            exact_zero_angle[b, j] = [inp["cand_heading"][b][j] == 0] * 2 + [inp["cand_elevation"][b][j] == 0] * 2
    for name, g, w, computed in (
            ("candidate_feat angle part", cand[..., D:], w_cand[..., D:], live[..., None] & ~exact_zero_angle),
            ("input_a_t", a_t, w_at, None)):
        g = np.ascontiguousarray(g, dtype=np.float32)
        if g.shape != w.shape or not bool(np.isfinite(g).all()):
            failed.append(name)
            continue
        if computed is None:   # input_a_t: computed everywhere but on bad agents (zero) and at angle 0
            zero = np.stack([np.asarray(inp["heading"]) == 0] * 2 + [np.asarray(inp["elevation"]) == 0] * 2, -1)
            computed = (np.abs(w).sum(-1, keepdims=True) > 0) & ~zero
        computed = np.broadcast_to(computed, w.shape)
        d = ulp_distance(g, w)
        if bool((g.view(np.uint32) != w.view(np.uint32))[~computed].any()):
            failed.append(name + " (where it must be equal)")
        if computed.any():
            worst = max(worst, int(d[computed].max()))
            if int(d[computed].max()) > 1:
                failed.append(name + " (more than one ulp)")
    return failed, worst
