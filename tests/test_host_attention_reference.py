"""No GPU: the fp64 attention reference, the CPU rounding models and the derived bounds of tests/helpers_attention.py.

What this file proves on a machine without a GPU is that tests/test_gpu_attention_conformance.py would fail on a subtly wrong
kernel: the minimal bf16 implementation passes every bound at every case family, and each entry of a table of wrong
implementations is rejected on at least one case of the table it is aimed at."""
import math

import pytest
import torch

import helpers_attention as ha

F64 = torch.float64


def _rand(shape, g, std):
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16).to(F64)


def _cpu_keep(B, nh, S, lens, p_eff, g, rounded=True):
    """A stand-in for the kernels' hash on the CPU: per (batch, head) one flat random sequence indexed by q * pitch + key,
    pitch = the sequence's length rounded up to 4 (the kernels' rule) or the length itself (the mutant's)."""
    keep = torch.ones(B, nh, S, S)
    for b in range(B):
        n = int(lens[b])
        pitch = (n + 3) & ~3 if rounded else n
        for h in range(nh):
            gg = torch.Generator().manual_seed(int(g) * 7919 + b * nh + h)
            flat = (torch.rand(n * ((n + 3) & ~3) + 4, generator=gg) >= p_eff).float()
            idx = torch.arange(n)[:, None] * pitch + torch.arange(n)[None, :]
            keep[b, h, :n, :n] = flat[idx]
    return keep


def make_case(name, B, S, nh, std=1.5, lens=None, bias=None, drop=None, head_scale=None, seed=0, q=None, k=None):
    """drop: (requested p, effective p) or None."""
    g = torch.Generator().manual_seed(seed)
    c = dict(name=name, B=B, S=S, nh=nh, lens=lens, head_scale=head_scale)
    c["q"] = _rand((B, nh, S, 64), g, std) if q is None else q
    c["k"] = _rand((B, nh, S, 64), g, std) if k is None else k
    c["v"] = _rand((B, nh, S, 64), g, std)
    c["dctx"] = _rand((B, nh, S, 64), g, 0.7)
    ll = [S] * B if lens is None else lens
    if lens is not None:
        rows = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None])[:, None, :, None].to(F64)
        for key in ("q", "k", "v", "dctx"):
            c[key] = c[key] * rows
    c["bias"] = (ha.length_bias(ll, S) if bias is None else ha.canonical_bias(bias))
    c["keep"], c["keep_mut"], c["p_eff"], c["p_req"] = None, None, 0.0, 0.0
    if drop is not None:
        c["p_req"], c["p_eff"] = drop
        c["keep"] = _cpu_keep(B, nh, S, ll, c["p_eff"], seed + 1)
        c["keep_mut"] = _cpu_keep(B, nh, S, ll, c["p_eff"], seed + 1, rounded=False)
    return c


def _terms(c):
    if "terms" not in c:
        c["terms"] = ha.ForwardTerms(c["q"], c["k"], c["v"], c["bias"], c["keep"], c["p_eff"], c["head_scale"])
    return c["terms"]


def _bterms(c):
    if "bterms" not in c:
        ctx_given = ha.forward_model(c["q"], c["k"], c["v"], c["bias"], c["keep"], c["p_eff"], None, lens=c["lens"])[0]
        t = _terms(c)
        valid_b = t.has_key.all(-1).all(-1)
        c["ctx_given"] = ctx_given
        c["bterms"] = ha.BackwardTerms(c["q"], c["k"], c["v"], c["bias"], c["dctx"], ctx_given, c["keep"], c["p_eff"], valid_b)
    return c["bterms"]


def _signed(c):
    """The signed statistic runs on random data with N >= 1e5 at std 0.5 and 1.5.  std 4 stays out, for a reason found on the
    rounding model, not on a kernel: its rows are nearly one-hot, every output lies a hair inside a bf16 grid point (V's own
    value divided by l = 1 + eps), and rounding to nearest is then not zero-mean (the model itself reaches 0.47 of the limit)."""
    return (c["B"] * c["nh"] * c["S"] * 64 >= 100000 and c["name"] == "numerics" and c["lens"] is None
            and float(c["v"].std()) < 2.0)


def fwd_ratios(c, mutant=None, signed=False):
    ctx, lse, probs = ha.forward_model(c["q"], c["k"], c["v"], c["bias"], c["keep"], c["p_eff"], c["head_scale"], mutant=mutant,
                                       lens=c["lens"], p_requested=c["p_req"], keep_mutant=c["keep_mut"])
    if c["head_scale"] is not None:
        probs = probs * c["head_scale"].to(F64).view(1, -1, 1, 1)
    ctx = torch.nan_to_num(ctx, nan=0.0) * _terms(c).has_key.unsqueeze(-1) + 0.0   # (rows without a finite key: not compared)
    # (a mutant is a wrong FORWARD kernel: the probabilities come from a kernel of their own and must not be what catches it)
    return ha.forward_ratios(_terms(c), ctx, lse, probs if c["keep"] is None and mutant is None else None, lens=c["lens"],
                             signed=signed)


def bwd_ratios(c, mutant=None, signed=False):
    t = _bterms(c)
    got = ha.attention_bwd_ref64(c["q"], c["k"], c["v"], c["bias"], c["dctx"], c["ctx_given"], c["keep"], c["p_eff"],
                                 round_model=True, mutant=mutant, lens=c["lens"])
    got = tuple(torch.nan_to_num(x, nan=0.0) for x in got)
    return ha.backward_ratios(t, got, lens=c["lens"], signed=signed)


# ---- the case families of the GPU file (section 3 of its docstring), at host size ----------------------------------------
def mask_forms(S):
    """{form: [6, S] additive fp64 bias} of the six mask patterns."""
    raw = ha.mask_patterns(S)
    return {form: torch.stack([ha.form_bias(raw[i], form) for i in range(6)]).double() for form in ha.FORMS}


def _cases():
    cs = {}
    g = torch.Generator().manual_seed(5)
    cs["lengths S=256"] = make_case("lengths S=256", 10, 256, 1, lens=[1, 2, 31, 32, 33, 64, 65, 193, 255, 256], seed=1)
    cs["lengths S=320"] = make_case("lengths S=320", 6, 320, 1, lens=[320, 257, 256, 1, 33, 289], seed=2)
    cs["lengths S=1025"] = make_case("lengths S=1025", 3, 1025, 1, lens=[1025, 513, 1], seed=3)
    cs["lengths S=256 p=0.1/16"] = make_case("lengths S=256 p=0.1/16", 6, 256, 1, lens=[1, 2, 33, 65, 230, 255],
                                              drop=(0.1, 6554.0 / 65536.0), seed=4)
    cs["lengths S=320 p=0.2/8"] = make_case("lengths S=320 p=0.2/8", 4, 320, 1, lens=[320, 257, 1, 290],
                                             drop=(0.2, 51.0 / 256.0), seed=5)
    for S in (33, 100, 300):
        for form, bias in mask_forms(S).items():
            cs["masks S=%d %s" % (S, form)] = make_case("masks", 6, S, 1, bias=bias, seed=10 + S)
    S = 100
    causal = torch.where(torch.arange(S)[:, None] >= torch.arange(S)[None, :], 0.0, -math.inf).double()
    band = torch.where((torch.arange(S)[:, None] - torch.arange(S)[None, :]).abs() <= 5, 0.0, -10000.0).double()
    cs["per-query causal+band S=100"] = make_case("per-query", 2, S, 2, bias=torch.stack([causal, band]), seed=20)
    cs["masks S=230 p=0.1/16"] = make_case("masks drop", 6, 230, 1, bias=mask_forms(230)["-10000"],
                                           drop=(0.1, 6554.0 / 65536.0), seed=21)
    for std in (0.5, 1.5, 4.0):
        cs["numerics S=228 std %.1f" % std] = make_case("numerics", 4, 228, 4, std=std, seed=30)
    cs["numerics S=656 std 0.5"] = make_case("numerics", 1, 656, 2, std=0.5, seed=31)
    cs["numerics S=228 std 0.5 p=0.1/8"] = make_case("numerics", 4, 228, 4, std=0.5, drop=(0.1, 26.0 / 256.0), seed=32)
    cs["numerics S=228 std 0.5 p=0.1/16"] = make_case("numerics", 4, 228, 4, std=0.5, drop=(0.1, 6554.0 / 65536.0), seed=32)
    cs["numerics S=230 std 0.5 p=0.1/16"] = make_case("numerics", 2, 230, 2, std=0.5, drop=(0.1, 6554.0 / 65536.0), seed=33)
    for what in ha.SCORE_SHAPES:
        q, k = _rand((1, 2, 300, 64), g, 0.5), _rand((1, 2, 300, 64), g, 0.5)
        q[..., 0], k[..., 0] = 8.0, ha.score_ramp(what, 300).to(torch.bfloat16).to(F64)   # score += 8 * ramp / 8
        cs["numerics S=300 " + what] = make_case("numerics", 1, 300, 2, std=1.0, q=q, k=k, seed=40)
    cs["head scale -1.5 / 0"] = make_case("head scale", 2, 100, 3, head_scale=torch.tensor([1.0, 0.0, -1.5]), seed=50)
    return cs


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_closed_form_backward_matches_float64_autograd():
    for name in ("masks S=33 -10000", "lengths S=256 p=0.1/16", "per-query causal+band S=100"):
        c = cases()[name]
        x = [c[n].clone().requires_grad_(True) for n in ("q", "k", "v")]
        ctx = ha.attention_ref64(x[0], x[1], x[2], c["bias"], c["keep"], c["p_eff"])[0]
        ctx.backward(c["dctx"])
        got = ha.attention_bwd_ref64(c["q"], c["k"], c["v"], c["bias"], c["dctx"], None, c["keep"], c["p_eff"])
        got2 = ha.attention_bwd_ref64(c["q"], c["k"], c["v"], c["bias"], c["dctx"], ctx.detach(), c["keep"], c["p_eff"])
        for g, g2, w in zip(got, got2, x):
            assert float((g - w.grad).norm()) <= 1e-12 * float(w.grad.norm()), name
            assert float((g2 - w.grad).norm()) <= 1e-12 * float(w.grad.norm()), name


@pytest.mark.parametrize("mask3", [False, True])
def test_reference_matches_the_oracle_module(mask3):
    """attention_ref64 against oracle.modeling.CaptionBertSelfAttention (eval, float64, identity projections)."""
    from oracle.config import make_config
    from oracle.modeling import CaptionBertSelfAttention

    B, S, nh = 2, 19, 2
    H = nh * 64
    cfg = make_config(hidden_size=H, num_attention_heads=nh, output_attentions=True)
    mod = CaptionBertSelfAttention(cfg).double().eval()
    for lin in (mod.query, mod.key, mod.value):
        with torch.no_grad():
            lin.weight.copy_(torch.eye(H, dtype=F64))
            lin.bias.zero_()
    g = torch.Generator().manual_seed(9)
    x = _rand((B, S, H), g, 1.0)
    if mask3:
        bias = torch.where(torch.rand(B, S, S, generator=g) > 0.3, 0.0, -10000.0).double()
        add = bias[:, None, :, :]
    else:
        bias = torch.where(torch.rand(B, S, generator=g) > 0.3, 0.0, -10000.0).double()
        add = bias[:, None, None, :]
    hm = torch.tensor([0.5, -2.0], dtype=F64)
    with torch.no_grad():
        want_ctx, want_p = mod(x, add, head_mask=hm.view(1, nh, 1, 1))
    t = x.view(B, S, nh, 64).permute(0, 2, 1, 3)
    ctx, lse, probs = ha.attention_ref64(t, t, t, bias, head_scale=hm)
    assert float((ctx.permute(0, 2, 1, 3).reshape(B, S, H) - want_ctx).abs().max()) < 1e-12
    assert float((probs * hm.view(1, nh, 1, 1) - want_p).abs().max()) < 1e-12
    s = ha.scores64(t, t, bias)
    assert float((torch.exp(s - lse.unsqueeze(-1)) - probs).abs().max()) < 1e-12


# ---- the rounding model passes every bound at every family ------------------------------------------------------------------
def test_rounding_model_passes_every_bound():
    worst = {}
    for name, c in cases().items():
        signed = _signed(c)
        r = fwd_ratios(c, signed=signed)
        assert ha.passes(r), (name, r)
        rb = bwd_ratios(c, signed=signed) if c["head_scale"] is None else {}
        assert ha.passes(rb), (name, rb)
        for key, val in list(r.items()) + list(rb.items()):
            worst[key] = max(worst.get(key, 0.0), abs(val))
    print()
    for key in sorted(worst):
        print("rounding model, worst %-28s %.3f" % (key, worst[key]))
    assert 0.05 < worst["ctx err/bound"] <= 1.0      # the bound is neither missed nor idle


# ---- the mutant table -------------------------------------------------------------------------------------------------------
_LEN = ["lengths S=256", "lengths S=320", "lengths S=1025", "masks S=33 -10000", "masks S=300 -10000"]
_NUM = ["numerics S=228 std 0.5", "numerics S=228 std 1.5", "numerics S=656 std 0.5"]
_DROP = ["lengths S=256 p=0.1/16", "lengths S=320 p=0.2/8", "numerics S=228 std 0.5 p=0.1/16", "masks S=230 p=0.1/16"]
MUTANT_TABLE = [
    ("last_key_dropped", "f", _LEN + _NUM),
    ("first_key_of_second_chunk_dropped", "f", ["lengths S=320", "lengths S=1025", "masks S=300 -10000"]),
    ("partial_tile_duplicates_last_row", "f", _LEN),
    ("rescale_skipped_once", "f", ["numerics S=300 rising", "numerics S=300 max in last tile"] + _NUM),
    ("p_truncated", "f", _NUM),
    ("normaliser_from_rounded_p", "f", _NUM + _LEN),
    ("normaliser_after_dropout", "f", _DROP),
    # 0.1 against attn_drop_p(0.1) = 0.100006 in 16-bit mode is a relative 7e-6, below bf16 resolution and any statistic at
    # these N: only the 8-bit mode's 0.1016 (1.7e-3) is detectable, through the signed statistic
    ("dropout_scale_from_requested_p", "f", ["numerics S=228 std 0.5 p=0.1/8"]),
    ("dropout_pitch_unrounded", "f", ["numerics S=230 std 0.5 p=0.1/16", "masks S=230 p=0.1/16", "lengths S=256 p=0.1/16"]),
    ("lse_off_by_ln2_2^-10", "f", _NUM),
    ("head_reads_next_heads_v", "f", _NUM),
    ("delta_without_dropout_scale", "b", _DROP),
    ("last_query_ignored", "b", _LEN + _NUM),
    ("dq_second_key_block_not_added", "b", ["lengths S=320", "lengths S=1025", "masks S=300 -10000", "numerics S=656 std 0.5"]),
]


def test_every_mutant_is_rejected():
    assert sorted(m for m, _, _ in MUTANT_TABLE) == sorted(ha.FWD_MUTANTS + ha.BWD_MUTANTS)
    rows, survivors = [], []
    for mutant, kind, names in MUTANT_TABLE:
        killed = None
        for name in names:
            c = cases()[name]
            signed = _signed(c)
            r = fwd_ratios(c, mutant, signed) if kind == "f" else bwd_ratios(c, mutant, signed)
            bad = {key: val for key, val in r.items() if not abs(val) <= 1.0}
            if bad:
                key = max(bad, key=lambda q: abs(bad[q]) if bad[q] == bad[q] else math.inf)
                killed = (name, key, bad[key])
                break
        rows.append((mutant, killed))
        if killed is None:
            survivors.append(mutant)
    print("\n%-36s %-36s %-22s %s" % ("mutant", "killed by case", "check", "ratio to the bound"))
    for mutant, killed in rows:
        print("%-36s %-36s %-22s %s" % ((mutant,) + (("SURVIVED", "", "") if killed is None else
                                                      (killed[0], killed[1], "%.3g" % killed[2]))))
    assert not survivors, survivors


# ---- the exact constructions ------------------------------------------------------------------------------------------------
def test_bit_column_answers_are_unique_for_every_length():
    """Q = 0, V = bit columns: every (2 count - n) / n, n = 1 .. 320 and the long lengths of the sweep, rounds to ONE bf16 value
    whatever fp32 does to it, and the counts tell any two neighbouring lengths apart."""
    seen = {}
    for n in list(range(1, 321)) + [511, 512, 513, 767, 768, 769, 1024, 1025]:
        row, unique = ha.bit_columns_expected(n)
        assert unique, n
        seen[n] = row
    # fp64 check of the construction itself: softmax of zero scores is exactly 1 / n
    c = ha.attention_ref64(torch.zeros(1, 1, 37, 64, dtype=F64), torch.zeros(1, 1, 37, 64, dtype=F64),
                           ha.bit_columns(37).view(1, 1, 37, 64), torch.zeros(1, 37, dtype=F64))[0]
    assert torch.equal(ha.bf16r(c[0, 0, 5]), seen[37])
    changed = sum(1 for n in range(2, 321) if not torch.equal(seen[n], seen[n - 1]))
    assert changed == 319


@pytest.mark.parametrize("S", [228, 767, 1025])
def test_permutation_construction_is_exact_enough(S):
    qkv, pi = ha.permutation_case(S, 1, seed=S)
    q, k, v = ha.split_qkv(qkv, 1, S, 1)
    probs = ha.attention_ref64(q, k, v, torch.zeros(1, S, dtype=F64))[2][0, 0]
    hit = probs[torch.arange(S), pi[0]]
    off = probs.clone()
    off[torch.arange(S), pi[0]] = 0
    assert float(off.max()) < 2.0 ** -60 and float((1 - hit).abs().max()) < 2.0 ** -50


def test_the_two_ds_rounding_forms_are_two_draws_of_one_error():
    """helpers_attention.DS_FORMS: dS rounded with or without the dropout scale.  Each form judged against the OTHER's yardstick
    stays within the L2 margin at every dropout case -- the same roundings, another draw -- while the max-norm margin is
    not safe across forms (printed: 0.64 at these sizes; over the 512 (batch, head) pairs of the GPU file's 256-sequence sweep
    one form against the other reaches 1.07 on the CPU and 1.02 on hardware, on single elements): hence the GPU file tells each
    kernel's form."""
    worst = {}
    for name, c in cases().items():
        if c["keep"] is None:
            continue
        t = _bterms(c)
        assert t.models["deferred"] is not t.models["folded"]
        for form, other in (("folded", "deferred"), ("deferred", "folded")):
            r = ha.backward_ratios(t, tuple(torch.nan_to_num(x, nan=0.0) for x in t.models[form]), lens=c["lens"], ds_form=other)
            for key, val in r.items():
                worst[key] = max(worst.get(key, 0.0), val)
                assert "max" in key or val <= 1.0, (name, form, key, val)
            own = ha.backward_ratios(t, tuple(torch.nan_to_num(x, nan=0.0) for x in t.models[form]), lens=c["lens"], ds_form=form)
            assert max(own.values()) <= 0.5 + 1e-9, (name, form, own)
    print()
    for key in sorted(worst):
        print("one form against the other's yardstick, worst %-22s %.3f" % (key, worst[key]))
