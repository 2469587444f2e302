"""The rectangular attention kernels (csrc/attention_rect.hip: Sq queries over Sk = Sh + Sq keys) against the fp64 reference and the
derived bounds of tests/helpers_attention.py / tests/helpers_attention_rect.py, through visitron_amd.ops only.  Alone:
    python -m pytest tests/test_gpu_attention_rect.py -q -s

Every operand is a view inside a NaN-filled buffer and every output a view inside a sentinel-filled one; nothing outside the
windows may change, and the dq columns of the history rows must come back as exact zeros.  The measured ratios of the run
are written to profiles/r13/attention_rect_conformance.txt: a record, not thresholds."""
import math
import os

import pytest
import torch

import helpers_attention as ha
import helpers_attention_rect as hr

pytestmark = pytest.mark.gpu
BF16, F64 = torch.bfloat16, torch.float64
SENTINEL = 57.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RECORD = []


def _window(dev, rows, cols, fill, dtype=BF16):
    """(buffer, view [rows, cols]): the view starts 2 rows and 8 columns inside a buffer 4 rows and 16 columns larger."""
    buf = torch.full((rows + 4, cols + 16), fill, dtype=dtype, device=dev)
    return buf, buf[2:2 + rows, 8:8 + cols]


def _flat_window(dev, n, fill, dtype):
    buf = torch.full((n + 8,), fill, dtype=dtype, device=dev)
    return buf, buf[4:4 + n]


def _outside_untouched(buf, view_rows, view_cols, fill, what):
    b = buf.clone()
    b[2:2 + view_rows, 8:8 + view_cols] = fill
    assert bool((b == fill).all()), "%s: written outside its window" % what


def _operand(dev, x):
    buf, view = _window(dev, x.shape[0], x.shape[1], float("nan"))
    view.copy_(x.to(dev, BF16))
    return view


def _record(label, ratios):
    _RECORD.append((label, dict(ratios)))
    ha.assert_ratios(label, ratios)


def run_case(dev, case, drop=None, backward=True, twice=False, tag=""):
    """One case through the forward (ctx, lse, keep words) and the backward; returns (ctx view, dqkv view or None) on the device."""
    from visitron_amd import ops

    B, nh, Sq, Sk, H = case.B, case.nh, case.Sq, case.Sk, case.H
    label = "rect %s%s" % (case.label(), tag)
    qd, dd = _operand(dev, case.qkv), _operand(dev, case.dctx)
    md = None
    if case.mask is not None:
        mbuf, md = _flat_window(dev, case.mask.numel(), float("nan"), torch.float32)
        md.copy_(case.mask.reshape(-1).to(dev))
        md = md.view(case.mask.shape)
    hs = None if case.head_scale is None else case.head_scale.to(dev, torch.float32)
    lbuf, lse = _flat_window(dev, B * nh * Sq, SENTINEL, torch.float32)
    cbuf, cview = _window(dev, B * Sq, H, SENTINEL)
    dr, words, wbuf = ops.NO_DROP, None, None
    nw = ops.keep_words_rect(B, nh, Sq, Sk)
    if drop is not None:
        dr = drop
        wbuf, words = _flat_window(dev, nw, 0x5A5A5A5A, torch.int32)
    ops.attention_rect_fwd(qd, B, Sq, Sk, nh, mask=md, mask_additive=case.mask_additive, head_scale=hs, out=cview, lse=lse, drop=dr,
                           keep_bits=words)
    torch.cuda.synchronize()
    _outside_untouched(cbuf, B * Sq, H, SENTINEL, label + " ctx")
    assert bool((lbuf[:4] == SENTINEL).all()) and bool((lbuf[4 + B * nh * Sq:] == SENTINEL).all()), label + ": lse window"
    if drop is not None:
        assert bool((wbuf[:4] == 0x5A5A5A5A).all()) and bool((wbuf[4 + nw:] == 0x5A5A5A5A).all()), label + ": keep-word window"
        keep = ops.unpack_keep_bits_rect(words, B, nh, Sq, Sk).cpu()
        # the hash's own decisions: element (q, key) of (b, h) is q * Sk' + key, the first Sq rows of the square site of Sk rows
        want = torch.stack([torch.stack([ops.attn_dropout_mask(Sk, dr, b * nh + h, device=dev)[:Sq].bool().cpu() for h in range(nh)])
                            for b in range(B)])
        assert torch.equal(keep, want), label + ": keep words differ from the site's hash"
        case.keep, case.p_eff = keep, ops.attn_drop_p(dr[0])
    _record(label + " fwd", hr.judge_forward(case, cview.float().cpu(), lse.view(B, nh, Sq)))
    if twice:
        cbuf2, cview2 = _window(dev, B * Sq, H, SENTINEL)
        ops.attention_rect_fwd(qd, B, Sq, Sk, nh, mask=md, mask_additive=case.mask_additive, head_scale=hs, out=cview2, drop=dr)
        assert torch.equal(cview2, cview), label + ": two forward launches differ"
    if not backward:
        return cview, None
    assert case.head_scale is None
    outs = []
    for kb in ([words, None] if drop is not None else [None]):
        gbuf, gview = _window(dev, B * Sk, 3 * H, SENTINEL)
        ops.attention_rect_bwd(qd, dd, cview, lse.view(B, nh, Sq), B, Sq, Sk, nh, mask=md, mask_additive=case.mask_additive, out=gview,
                               drop=dr, keep_bits=kb)
        torch.cuda.synchronize()
        _outside_untouched(gbuf, B * Sk, 3 * H, SENTINEL, label + " dqkv")
        how = "" if drop is None else (" keep words" if kb is not None else " hash")
        _record(label + " bwd" + how, hr.judge_backward(case, cview.float().cpu(), gview.float().cpu()))
        outs.append(gview)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), label + ": keep words and hash give different gradients"
    if twice:
        gbuf2, gview2 = _window(dev, B * Sk, 3 * H, SENTINEL)
        ops.attention_rect_bwd(qd, dd, cview, lse.view(B, nh, Sq), B, Sq, Sk, nh, mask=md, mask_additive=case.mask_additive, out=gview2,
                               drop=dr, keep_bits=words)
        assert torch.equal(gview2, outs[0]), label + ": two backward launches differ"
    return cview, outs[0]


@pytest.mark.parametrize("shape", hr.SHAPES)
def test_forward_and_backward_hold_the_derived_bounds(dev, shape):
    B, nh, Sh, Sq = shape
    run_case(dev, hr.Case(B, nh, Sh, Sq, "none"), twice=True)
    run_case(dev, hr.Case(B, nh, Sh, Sq, "causal"))


@pytest.mark.parametrize("form", [f for f in hr.BIAS_FORMS if f not in ("none", "causal")])
def test_bias_forms(dev, form):
    for shape in ((2, 2, 37, 5), (2, 2, 250, 17), (1, 2, 300, 33)):
        run_case(dev, hr.Case(*shape, form=form))


@pytest.mark.parametrize("p", (0.1, 0.5))
def test_dropout_with_the_keep_words_read_back(dev, p):
    from visitron_amd import ops

    for i, shape in enumerate(((2, 2, 37, 5), (2, 2, 250, 17), (1, 2, 300, 33), (1, 2, 539, 228))):
        case = hr.Case(*shape, form="causal" if i % 2 else "0/1")
        run_case(dev, case, drop=(p, 1234 + i, ops.site_attn(i)), twice=(i == 1), tag=" p=%g" % p)
        kept, n = float(case.keep.float().mean()), case.keep.numel()
        pe = ops.attn_drop_p(p)
        sigma = math.sqrt(pe * (1 - pe) / n)
        print("kept fraction %.5f, expected %.5f +- %.5f (n = %d)" % (kept, 1 - pe, sigma, n))
        assert abs(kept - (1 - pe)) <= 6 * sigma, (shape, kept, pe)


def test_eight_bit_dropout_fields(dev):
    from visitron_amd import ops

    old = ops.attn_dropout_bits()
    ops.set_attn_dropout_bits(8)
    try:
        run_case(dev, hr.Case(2, 2, 250, 17, "0/1"), drop=(0.1, 77, ops.site_attn(1)), tag=" 8-bit")
    finally:
        ops.set_attn_dropout_bits(old)


def test_head_scale(dev):
    hs = torch.tensor([0.5, -1.25, 0.0])
    run_case(dev, hr.Case(2, 3, 37, 5, "0/1", head_scale=hs), backward=False)


def test_bit_columns_census_names_the_keys_that_were_summed(dev):
    """Uniform scores (q = 0) over v = helpers_attention.bit_columns: every context element is (2 count - n) / n rounded once to bf16,
    so a dropped, duplicated or out-of-range key -- a history key among them -- changes a count."""
    from visitron_amd import ops

    for B, nh, Sh, Sq in ((2, 2, 37, 5), (1, 2, 255, 2), (1, 1, 768, 256), (1, 2, 300, 33)):
        Sk, H = Sh + Sq, nh * 64
        want, unique = ha.bit_columns_expected(Sk)
        qkv = torch.zeros(B, Sk, 3, nh, 64)
        qkv[:, :, 1] = torch.randn(B, Sk, nh, 64).to(BF16).float()
        qkv[:, :, 2] = ha.bit_columns(Sk).float()[None, :, None, :]
        out = ops.attention_rect_fwd(_operand(dev, qkv.reshape(B * Sk, 3 * H)), B, Sq, Sk, nh)
        got = out.float().cpu().to(F64).view(B, Sq, nh, 64)
        if unique:
            assert torch.equal(got, want.expand_as(got)), (Sh, Sq)
        else:
            assert float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max()), (Sh, Sq)
        # one masked history key leaves the census of the others
        mask = torch.ones(B, Sk)
        mask[:, Sh // 2] = 0
        bias = torch.where(mask == 1, 0.0, -math.inf)
        out = ops.attention_rect_fwd(_operand(dev, qkv.reshape(B * Sk, 3 * H)), B, Sq, Sk, nh, mask=bias.to(dev), mask_additive=True)
        cols = ha.bit_columns(Sk)
        x = (cols.sum(0) - cols[Sh // 2]) / (Sk - 1)
        got = out.float().cpu().to(F64).view(B, Sq, nh, 64)
        assert float((got - x).abs().max()) <= 2.0 ** -8 * float(x.abs().max()) + 2.0 ** -20, (Sh, Sq)


def test_one_hot_probabilities_return_integer_values_exactly(dev):
    """helpers_attention.permutation_case over the extended rows: query i's score with key pi(Sh + i) is 512 and every other one is
    lower by a margin that makes its probability < 2^-60, so ctx[i] == v[pi(Sh + i)] bit for bit, wherever that key sits."""
    from visitron_amd import ops

    for Sh, Sq in ((37, 5), (250, 17), (539, 228)):
        Sk, nh = Sh + Sq, 2
        qkv, pi = ha.permutation_case(Sk, nh, seed=Sk)
        v = torch.randint(-8, 9, (Sk, nh, 64)).float()
        qkv = qkv.view(Sk, 3, nh, 64).clone()
        qkv[:, 2] = v
        out = ops.attention_rect_fwd(_operand(dev, qkv.reshape(Sk, 3 * nh * 64)), 1, Sq, Sk, nh).float().cpu().view(Sq, nh, 64)
        for h in range(nh):
            assert torch.equal(out[:, h], v[pi[h, Sh:], h]), (Sh, Sq, h)


def test_limits_are_refused_by_the_host_check(dev):
    from visitron_amd import ops

    H = 64
    ctx = torch.full((1025, H), SENTINEL, dtype=BF16, device=dev)
    qkv = torch.zeros((1025, 3 * H), dtype=BF16, device=dev)
    lse = torch.zeros(1025, dtype=torch.float32, device=dev)
    for Sq, Sk in ((1, 1025), (5, 4), (0, 4)):
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.attention_rect_fwd(qkv, 1, Sq, Sk, 1, out=ctx)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.attention_rect_bwd(qkv, ctx, ctx, lse, 1, Sq, Sk, 1, out=torch.empty_like(qkv))
    torch.cuda.synchronize()
    assert bool((ctx == SENTINEL).all())
    ops.attention_rect_fwd(qkv, 1, 1024, 1024, 1, out=ctx[:1024])     # the largest legal problem
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ctx.float()).all()) and bool((ctx[1024] == SENTINEL).all())


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    """After the module's tests: the run's measured ratios -> profiles/r13/attention_rect_conformance.txt (a tree that cannot be
    written to keeps the record it has)."""
    yield
    if not _RECORD:
        return
    keys = sorted({k for _, r in _RECORD for k in r})
    lines = ["# measured / bound of every check of tests/test_gpu_attention_rect.py (all must be <= 1)\n"]
    for label, r in _RECORD:
        lines.append("%-58s %s\n" % (label, "  ".join("%s %.3f" % (k, r[k]) for k in keys if k in r)))
    lines.append("# worst: %s\n" % "  ".join("%s %.3f" % (k, max(r.get(k, 0.0) for _, r in _RECORD)) for k in keys))
    try:
        out_dir = os.path.join(ROOT, "profiles", "r13")
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "attention_rect_conformance.txt"), "w") as fh:
            fh.writelines(lines)
    except OSError:
        pass
