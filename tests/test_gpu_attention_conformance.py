"""The fused attention kernels (csrc/attention_fwd.hip; csrc/attention_bwd.hip and its kernel files attention_bwd_*.hip)
against the fp64 reference and the derived bounds of tests/helpers_attention.py, through visitron_amd.ops only.  This file is the acceptance gate of any new attention
kernel; alone:  python -m pytest tests/test_gpu_attention_conformance.py -q -s

Every case runs the forward (with lse), the probabilities where the layout allows them (padded, no dropout) and the backward
under EACH of set_attn_bwd_waves 4, 8, 10, 16, 17; where the dispatcher routes a setting to another kernel (more than one key
block, a per-query bias, dropout without keep words, B > 1 024) the case still runs: that is the shipped routing.

  a. every length: compacted layouts whose sequences walk every length across the 32-key tile, the 32-query wave slice, the
     64-key wave block and the 256-key chunk, with and without dropout;
  b. padded layouts with one mask pattern per sequence, in every form a caller can pass a mask;
  c. numerics: input scales, scores that rise / fall from tile to tile, a shared +200;
  d. exact answers;
  e. layout and hygiene: leading dimensions, head counts, B > 1 024, run-to-run reproducibility.

A per-query bias [B, S, S] through the BACKWARD is served (the 4- and 8-wave kernels carry it; the training engine uses it for
the reference's 3-D masks), so it is held to the fp64 reference here like every other form."""
import math

import pytest
import torch

import helpers_attention as ha

pytestmark = pytest.mark.gpu
BF16, F64 = torch.bfloat16, torch.float64
WAVES = (4, 8, 10, 16, 17)
# which of helpers_attention.DS_FORMS each backward kernel is (it matters under dropout only): the 4-wave kernel rounds dS with
# the dropout scale folded in, the 8-wave kernel (settings 8, 10, and wherever 16 / 17 are routed to it) and both 16-wave kernels
# round it before that scale
DS_FORM = {4: "folded", 8: "deferred", 10: "deferred", 16: "deferred", 17: "deferred"}
SENTINEL = 57.0


def _randn(shape, g, std):
    return (torch.randn(shape, generator=g) * std).to(BF16).float()


def _from_heads(x, B, S, nh):
    """[B*S, nh*64] on any device -> [B, nh, S, 64] float64 on the CPU."""
    return ha.heads(x.float(), B, S, nh)


def _length_groups(lens, B, S):
    """[(sequence indices, padded length, lengths)]: the fp64 reference of a compacted batch is built per group of sequences of
    similar length (the same multiple of 32) at that group's own padded length -- exact, since rows past a sequence's length are
    zero and its keys there carry a bias of -inf, and 2.5 x cheaper for a sweep over every length.  Padded batches: one group."""
    if lens is None:
        return [(None, S, None)]
    key = (torch.as_tensor(lens) + 31) // 32
    groups = []
    for kk in key.unique().tolist():
        idx = torch.nonzero(key == kk).flatten()
        lg = [int(lens[i]) for i in idx.tolist()]
        groups.append((idx, max(lg), lg))
    return groups


def _crop(x, g, square=3):
    """x of a group: the sequences g[0], the first g[1] positions of dimension 2 (square = 1: of dimension 1; 4: of 2 and 3)."""
    idx, Sg, _ = g
    if x is None or idx is None:
        return x
    x = x[idx]
    if square == 1:
        return x[:, :Sg].contiguous()
    return (x[:, :, :Sg, :Sg] if square == 4 else x[:, :, :Sg]).contiguous()


def _merge(out, ratios):
    for key, val in ratios.items():
        if key not in out or abs(val) > abs(out[key]) or val != val:
            out[key] = val


def run_case(dev, name, qkv, B, S, nh, lens=None, mask=None, mask_additive=False, bias64=None, dctx=None, drop=None, bits=16,
             head_scale=None, signed=False, want_probs=True, backward=True, waves=WAVES, skip_b=None, wide=False, twice=False):
    """One case through forward, probabilities and every backward kernel.  qkv [B*S, 3 nh 64] fp32 in the PADDED geometry
    (bf16-exact; rows past a sequence's length are not passed to the kernels), lens: a compacted batch (ops.SeqLayout);
    mask / mask_additive: what the kernels get, bias64: the same as the fp64 additive bias.  wide: ld_qkv = 3H + 8 and the
    outputs as column slices of wider buffers.  Returns the forward context [B, nh, S, 64] (fp64)."""
    from visitron_amd import ops

    H = nh * 64
    assert not (signed and lens is not None), "the signed statistic is not merged over length groups"
    seq, index = None, torch.arange(B * S)
    if lens is not None:
        keepm = torch.arange(S)[None, :] < torch.as_tensor(lens)[:, None]
        seq = ops.SeqLayout(keepm.to(dev))
        index = seq.index.cpu()
        assert seq.rows == int(sum(lens))
        qkv = qkv * keepm.reshape(-1, 1).float()
    rows = index.numel()
    if dctx is None:
        dctx = _randn((B * S, H), torch.Generator().manual_seed(B * 7 + S), 0.7)
    if lens is not None:
        dctx = dctx * keepm.reshape(-1, 1).float()
    bias = ha.length_bias(lens if lens is not None else [S] * B, S) if bias64 is None else ha.canonical_bias(bias64)
    q, k, v = ha.split_qkv(qkv, B, S, nh)
    d64 = ha.heads(dctx, B, S, nh)

    def dev_rows(x, width):   # the kernels' input: real rows only, optionally with a padded leading dimension
        x = x[index]
        if not wide:
            return x.to(dev, BF16).contiguous()
        buf = torch.full((rows, width + 8), SENTINEL, dtype=BF16, device=dev)
        buf[:, :width] = x.to(dev, BF16)
        return buf[:, :width]

    def out_buf(width):       # rows + 4 (sentinel rows), as a column slice of a wider buffer when `wide`
        buf = torch.full((rows + 4, width + (16 if wide else 0)), SENTINEL, dtype=BF16, device=dev)
        return buf, (buf[:, 8:8 + width] if wide else buf)

    def padded(x):            # kernel output rows -> padded geometry
        full = torch.zeros((B * S, x.shape[1]), dtype=torch.float32)
        full[index] = x[:rows].float().cpu()
        return full

    def untouched(buf, view, what):
        assert bool((buf[rows:] == SENTINEL).all()), "%s: rows past the batch's rows were written (%s)" % (name, what)
        if wide:
            assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + view.shape[1]:] == SENTINEL).all()), \
                "%s: padding columns were written (%s)" % (name, what)

    qd, dd = dev_rows(qkv, 3 * H), dev_rows(dctx, H)
    md = None if mask is None else mask.to(dev, torch.float32).contiguous()
    hs = None if head_scale is None else head_scale.to(dev, torch.float32)
    old_bits = ops.attn_dropout_bits()
    ops.set_attn_dropout_bits(bits)
    try:
        keep, p_eff, words, dr = None, 0.0, None, ops.NO_DROP
        if drop is not None:
            dr, p_eff = drop, ops.attn_drop_p(drop[0])
            words = torch.zeros(ops.keep_words(B, nh, S), dtype=torch.int32, device=dev)
            keep = torch.zeros(B, nh, S, S)
            for b in range(B):
                n = int(lens[b]) if lens is not None else S
                for h in range(nh):
                    keep[b, h, :n, :n] = ops.attn_dropout_mask(n, dr, b * nh + h, device=dev).float().cpu()
        lse = torch.zeros((B, nh, S), dtype=torch.float32, device=dev)
        cbuf, cview = out_buf(H)
        kw = dict(mask=md, mask_additive=mask_additive) if seq is None else dict(seq=seq)
        ops.attention_fwd(qd, B, S, nh, head_scale=hs, out=cview, lse=lse, drop=dr, keep_bits=words, **kw)
        torch.cuda.synchronize()
        untouched(cbuf, cview, "forward")
        if drop is not None:   # the keep words are the hash's decisions, for every sequence
            got_keep = ops.unpack_keep_bits(words, B, nh, S).cpu()
            valid = keep.new_zeros(B, 1, S, S, dtype=torch.bool)
            for b in range(B):
                n = int(lens[b]) if lens is not None else S
                valid[b, :, :n, :n] = True
            assert torch.equal(got_keep & valid, keep.bool() & valid), "%s: keep words differ from attn_dropout_mask" % name
        ctx64 = _from_heads(padded(cview), B, S, nh)
        probs = None
        if want_probs and seq is None and drop is None:
            probs = ops.attention_probs(qd, lse, B, S, nh, head_scale=hs, **kw).cpu()
        groups, lse_c, ratios, fterms = _length_groups(lens, B, S), lse.cpu(), {}, []
        for g in groups:
            t = ha.ForwardTerms(_crop(q, g), _crop(k, g), _crop(v, g), _crop(bias, g, 1), _crop(keep, g, 4), p_eff, head_scale)
            fterms.append(t)
            _merge(ratios, ha.forward_ratios(t, _crop(ctx64, g), _crop(lse_c, g), probs, lens=g[2], signed=signed))
        ha.assert_ratios(name + " fwd", ratios)
        if twice:
            cbuf2, cview2 = out_buf(H)
            ops.attention_fwd(qd, B, S, nh, head_scale=hs, out=cview2, drop=dr, **kw)
            assert torch.equal(cview2[:rows], cview[:rows]), "%s: two forward launches differ" % name
        if not backward:
            return ctx64
        assert head_scale is None
        bts = []
        for g, t in zip(groups, fterms):
            valid_b = t.has_key.all(-1).all(-1)
            if skip_b is not None:
                assert len(groups) == 1 and torch.equal(~valid_b, skip_b), "%s: only the named sequences may be left out" % name
            else:
                assert bool(valid_b.all()), name
            bts.append(ha.BackwardTerms(_crop(q, g), _crop(k, g), _crop(v, g), _crop(bias, g, 1), _crop(d64, g), _crop(ctx64, g),
                                        _crop(keep, g, 4), p_eff, valid_b))
        del fterms

        def bwd_ratios(gview):
            gp, out = padded(gview), {}
            got = tuple(_from_heads(gp[:, i * H:(i + 1) * H], B, S, nh) for i in range(3))
            for g, bt in zip(groups, bts):
                _merge(out, ha.backward_ratios(bt, tuple(_crop(x, g) for x in got), lens=g[2], signed=signed, ds_form=DS_FORM[w]))
            return out

        ctx_d = cview[:rows]
        for w in waves:
            for kb in ([words, None] if drop is not None else [None]):
                label = "%s bwd waves %d%s" % (name, w, "" if drop is None else (" keep words" if kb is not None else " hash"))
                gbuf, gview = out_buf(3 * H)
                ops.set_attn_bwd_waves(w)
                try:
                    ops.attention_bwd(qd, dd, ctx_d, lse, B, S, nh, out=gview, drop=dr, keep_bits=kb, **kw)
                    torch.cuda.synchronize()
                    if twice:
                        gbuf2, gview2 = out_buf(3 * H)
                        ops.attention_bwd(qd, dd, ctx_d, lse, B, S, nh, out=gview2, drop=dr, keep_bits=kb, **kw)
                        torch.cuda.synchronize()
                finally:
                    ops.set_attn_bwd_waves(0)
                untouched(gbuf, gview, label)
                ha.assert_ratios(label, bwd_ratios(gview))
                if twice and S <= 256:
                    assert torch.equal(gview2[:rows], gview[:rows]), "%s: two launches differ (S <= 256 promises bitwise)" % label
                elif twice:
                    ha.assert_ratios(label + " second launch", bwd_ratios(gview2))
        return ctx64
    finally:
        ops.set_attn_dropout_bits(old_bits)


# ---- a. every length ---------------------------------------------------------------------------------------------------------
def _sweep_lens(which):
    g = torch.Generator().manual_seed(77)
    if which == 256:
        return 256, [int(x) + 1 for x in torch.randperm(256, generator=g)]
    if which == 320:
        lens = list(range(193, 321)) + [1, 31, 32, 33, 64, 255, 256, 257]
        return 320, [lens[int(i)] for i in torch.randperm(len(lens), generator=g)]
    return 1025, [1025, 1024, 769, 768, 767, 513, 512, 511, 257, 1]


SWEEP_DROPS = [None, (0.1, 16), (0.2, 8)]


@pytest.mark.parametrize("drop", SWEEP_DROPS, ids=["no dropout", "p=0.1 16-bit", "p=0.2 8-bit"])
@pytest.mark.parametrize("which", [256, 320, 1025])
def test_every_length(dev, which, drop):
    from visitron_amd import ops

    S, lens = _sweep_lens(which)
    B, nh = len(lens), 2
    qkv = _randn((B * S, 3 * nh * 64), torch.Generator().manual_seed(which), 1.0)
    name = "sweep S=%d%s" % (S, "" if drop is None else " p=%.1f/%d" % drop)
    run_case(dev, name, qkv, B, S, nh, lens=lens, drop=None if drop is None else (drop[0], 4242 + which, ops.site_attn(1)),
             bits=16 if drop is None else drop[1])


# ---- b. padded layout with masks ------------------------------------------------------------------------------------------------
MASK_S = [1, 2, 31, 32, 33, 64, 100, 228, 255, 256, 257, 300, 511, 512, 513, 656, 767, 1024]
FORMS, mask_patterns, form_bias = ha.FORMS, ha.mask_patterns, ha.form_bias


def _mask_qkv(S):
    return _randn((6 * S, 3 * 2 * 64), torch.Generator().manual_seed(2000 + S), 1.0)


@pytest.mark.parametrize("S", MASK_S)
def test_masks_raw(dev, S):
    raw = mask_patterns(S)
    run_case(dev, "masks raw S=%d" % S, _mask_qkv(S), 6, S, 2, mask=raw, bias64=(1.0 - raw.double()) * -10000.0)


def _additive_case(dev, name, S, forms, **kw):
    raw = mask_patterns(S)
    bias = torch.stack([form_bias(raw[i], forms[i]) for i in range(6)])
    # rows with no finite key are outside the contract (NaN in the reference too): exactly the "nothing kept" sequence, and only
    # in the two infinite forms
    skip_b = torch.tensor([i == 2 and forms[i] in ("-inf", "finfo.min") for i in range(6)])
    run_case(dev, name, _mask_qkv(S), 6, S, 2, mask=bias, mask_additive=True, bias64=bias.double(), skip_b=skip_b, **kw)


@pytest.mark.parametrize("S", MASK_S)
def test_masks_additive_forms_paired(dev, S):
    """Pattern i of the batch takes form (i + rank of S) mod 4: over the 18 lengths every (pattern, form) pair runs at several
    lengths, in a third of the launches of the full cross product (which test_masks_additive_forms_crossed runs at two lengths)."""
    r = MASK_S.index(S)
    forms = [FORMS[(i + r) % 4] for i in range(6)]
    _additive_case(dev, "masks additive paired S=%d" % S, S, forms)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", [100, 300])
def test_masks_additive_forms_crossed(dev, S, form):
    _additive_case(dev, "masks additive %s S=%d" % (form, S), S, [form] * 6)


@pytest.mark.parametrize("S", MASK_S)
def test_masks_per_query(dev, S):
    """[B, S, S] bias: a causal mask (-inf above the diagonal), a band (-10 000 outside |q - k| <= 5), and four of the per-key
    patterns broadcast over the queries."""
    raw = mask_patterns(S)
    qi, ki = torch.arange(S)[:, None], torch.arange(S)[None, :]
    b3 = torch.zeros(6, S, S)
    b3[0] = torch.where(qi >= ki, 0.0, -math.inf)
    b3[1] = torch.where((qi - ki).abs() <= 5, 0.0, -10000.0)
    for i, form in ((2, "-10000"), (3, "-inf"), (4, "finfo.min"), (5, "fractional")):
        b3[i] = form_bias(raw[i], form)[None, :].expand(S, S)
    run_case(dev, "masks per-query S=%d" % S, _mask_qkv(S), 6, S, 2, mask=b3, mask_additive=True, bias64=b3.double())


@pytest.mark.parametrize("S", [228, 300])
def test_masks_with_dropout(dev, S):
    from visitron_amd import ops

    raw = mask_patterns(S)
    run_case(dev, "masks raw p=0.1/16 S=%d" % S, _mask_qkv(S), 6, S, 2, mask=raw, bias64=(1.0 - raw.double()) * -10000.0,
             drop=(0.1, 99 + S, ops.site_attn(2)), bits=16)


# ---- c. numerics ------------------------------------------------------------------------------------------------------------------
def _signed_ok(std):
    """The signed statistic runs at std 0.5 and 1.5.  At std 4 the rows are nearly one-hot, every output lies a hair inside a
    bf16 grid point (V's own value divided by l = 1 + eps) and rounding to nearest is not zero-mean: the CPU rounding model
    itself reaches 0.47 of the limit there (tests/test_host_attention_reference.py)."""
    return std < 2.0


@pytest.mark.parametrize("std", [0.5, 1.5, 4.0])
@pytest.mark.parametrize("S", [228, 656])
def test_input_scales(dev, S, std):
    B, nh = (4, 4) if S == 228 else (2, 2)                      # N = B nh S 64 >= 1e5 for the signed statistic
    qkv = _randn((B * S, 3 * nh * 64), torch.Generator().manual_seed(S * 10 + int(std * 2)), std)
    run_case(dev, "numerics S=%d std %.1f" % (S, std), qkv, B, S, nh, signed=_signed_ok(std))


@pytest.mark.parametrize("p,bits", [(0.1, 16), (0.1, 8)])
def test_input_scale_of_the_model_with_dropout(dev, p, bits):
    """The dropout scale is 1 / (1 - attn_drop_p(p)), not 1 / (1 - p): in 8-bit mode (0.1016) the difference is a relative
    1.7e-3 on every output, visible to the signed statistic only."""
    from visitron_amd import ops

    B, S, nh = 4, 228, 4
    qkv = _randn((B * S, 3 * nh * 64), torch.Generator().manual_seed(321), 0.5)
    run_case(dev, "numerics S=228 std 0.5 p=%.1f/%d" % (p, bits), qkv, B, S, nh, drop=(p, 555, ops.site_attn(0)), bits=bits,
             signed=True)


@pytest.mark.parametrize("what", ha.SCORE_SHAPES)
def test_score_shapes(dev, what):
    """helpers_attention.score_ramp: the rescale branch of the online softmax at every tile, once, late; a shared +200."""
    B, S, nh = 2, 300, 2
    x = _randn((B, S, 3, nh, 64), torch.Generator().manual_seed(len(what)), 0.5)
    x[:, :, 0, :, 0] = 8.0                                       # score += 8 * ramp / 8
    x[:, :, 1, :, 0] = ha.score_ramp(what, S).to(BF16).float()[None, :, None]
    run_case(dev, "numerics S=300 " + what, x.reshape(B * S, -1), B, S, nh)


# ---- d. exact answers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [256, 320, 1025])
def test_exact_counts_at_every_length(dev, which):
    """Q = 0 and V[k] = the bits of k as +-1 columns: every context element is (2 count - n) / n rounded once to bf16, for every
    length of sweep (a): any dropped, duplicated or out-of-range key changes a count."""
    from visitron_amd import ops

    S, lens = _sweep_lens(which)
    B, nh = len(lens), 2
    keepm = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    seq = ops.SeqLayout(keepm.to(dev))
    x = torch.zeros(B, S, 3, nh, 64)
    x[:, :, 2] = ha.bit_columns(S).float()[None, :, None, :]
    g = torch.Generator().manual_seed(3)
    x[:, :, 1] = _randn((B, S, nh, 64), g, 1.0)                  # K is arbitrary: Q = 0
    qd = x.reshape(B * S, -1)[seq.index.cpu()].to(dev, BF16)
    ctx = ops.attention_fwd(qd, B, S, nh, seq=seq).float().cpu()
    off = 0
    for n in lens:
        want, unique = ha.bit_columns_expected(n)
        assert unique, n
        got = ctx[off:off + n].view(n, nh, 64)
        assert torch.equal(got, want.float().view(1, 1, 64).expand(n, nh, 64)), "length %d" % n
        off += n
    # Q = 0, no mask: dV[k] = mean_q dO[q] for every k, within one rounding; dQ = 0 exactly is NOT claimed (dS = P (dP - delta)
    # cancels only to rounding)
    dctx = _randn((B * S, nh * 64), g, 1.0)[seq.index.cpu()]
    lse = torch.zeros((B, nh, S), dtype=torch.float32, device=dev)
    cd = ops.attention_fwd(qd, B, S, nh, seq=seq, lse=lse)
    for w in WAVES:
        ops.set_attn_bwd_waves(w)
        try:
            dv = ops.attention_bwd(qd, dctx.to(dev, BF16), cd, lse, B, S, nh, seq=seq)[:, 2 * nh * 64:].float().cpu()
        finally:
            ops.set_attn_bwd_waves(0)
        off = 0
        for n in lens:
            want = dctx[off:off + n].double().mean(0, keepdim=True)
            a = dctx[off:off + n].double().abs().mean(0, keepdim=True)
            # one bf16 rounding of the result, the fp32 sum of n terms each carrying P = 1 / n (exact in bf16 only for n a power
            # of two: u on every term otherwise)
            bound = ha.U * want.abs() + (ha.U + 2.0 ** -18) * a
            assert bool(((dv[off:off + n].double() - want).abs() <= bound).all()), "dV, length %d, waves %d" % (n, w)
            off += n


@pytest.mark.parametrize("S", [228, 767, 1025])
def test_exact_permutation(dev, S):
    """K[k] = random +-8 codes and Q[q] = K[pi(q)]: ctx[q] == V[pi(q)] bit for bit (any row, key or swizzle permutation shows)."""
    from visitron_amd import ops

    nh = 2
    qkv, pi = ha.permutation_case(S, nh, seed=S)
    ctx = ops.attention_fwd(qkv.to(dev, BF16), 1, S, nh).float().cpu().view(S, nh, 64)
    v = qkv.view(S, 3, nh, 64)[:, 2]
    for h in range(nh):
        assert torch.equal(ctx[:, h], v[pi[h], h]), "head %d" % h


def test_zero_gradient_in_zero_gradient_out_and_head_scale(dev):
    from visitron_amd import ops

    B, S, nh = 2, 300, 3
    g = torch.Generator().manual_seed(8)
    qkv = _randn((B * S, 3 * nh * 64), g, 1.0)
    qd = qkv.to(dev, BF16)
    lse = torch.zeros((B, nh, S), dtype=torch.float32, device=dev)
    ctx = ops.attention_fwd(qd, B, S, nh, lse=lse)
    for S2 in (S, 200):                                           # one key block, and two with the fp32 dQ slab
        for w in WAVES:
            ops.set_attn_bwd_waves(w)
            try:
                lse2 = torch.zeros((B, nh, S2), dtype=torch.float32, device=dev)
                q2 = qd[:B * S2]
                c2 = ops.attention_fwd(q2, B, S2, nh, lse=lse2)
                dq = ops.attention_bwd(q2, torch.zeros_like(c2), c2, lse2, B, S2, nh)
            finally:
                ops.set_attn_bwd_waves(0)
            assert float(dq.float().abs().max()) == 0.0, (S2, w)
    hs = torch.tensor([1.0, 0.0, -1.5])
    got = run_case(dev, "head scale 1 / 0 / -1.5", qkv, B, S, nh, head_scale=hs, backward=False)
    assert float(got[:, 1].abs().max()) == 0.0                   # head scale 0: exactly 0
    base = ha.heads(ctx.float(), B, S, nh)
    assert torch.equal(got[:, 0], base[:, 0])


def test_per_query_bias_backward_is_served_and_seq_refused(dev):
    """The backward takes a per-query bias [B, S, S] (the training engine's 3-D masks; test_masks_per_query holds it to fp64);
    what the dispatcher refuses is that bias together with compacted rows."""
    from visitron_amd import ops

    B, S, nh = 1, 40, 1
    qd = _randn((B * S, 192), torch.Generator().manual_seed(4), 1.0).to(dev, BF16)
    lse = torch.zeros((B, nh, S), dtype=torch.float32, device=dev)
    ctx = ops.attention_fwd(qd, B, S, nh, lse=lse)
    with pytest.raises((RuntimeError, AssertionError)):
        seq = ops.SeqLayout(torch.ones(B, S, dtype=torch.bool, device=dev))
        ops.attention_bwd(qd, ctx, ctx, lse, B, S, nh, mask=torch.zeros(B, S, S, device=dev), mask_additive=True, seq=seq)


# ---- e. layout and hygiene --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,nh", [(100, 1), (228, 12), (300, 16)])
def test_wide_buffers_head_counts_and_reproducibility(dev, S, nh):
    """ld_qkv = 3H + 8, out / dqkv as column slices of wider buffers (padding columns keep a sentinel); nh 1, 12, 16; two
    launches bitwise equal for every kernel at S <= 256 (the header's promise) and within the bound at S > 256."""
    B = 2
    raw = torch.ones(B, S)
    raw[1, S // 2:] = 0
    qkv = _randn((B * S, 3 * nh * 64), torch.Generator().manual_seed(S + nh), 1.0)
    run_case(dev, "wide buffers S=%d nh=%d" % (S, nh), qkv, B, S, nh, mask=raw, bias64=(1.0 - raw.double()) * -10000.0,
             wide=True, twice=True)


def test_wide_buffers_compacted_with_dropout(dev):
    from visitron_amd import ops

    B, S, nh = 5, 256, 2
    qkv = _randn((B * S, 3 * nh * 64), torch.Generator().manual_seed(19), 1.0)
    run_case(dev, "wide buffers compacted p=0.1/16", qkv, B, S, nh, lens=[256, 1, 77, 130, 33], drop=(0.1, 7, ops.site_attn(3)),
             wide=True, twice=True)


def test_more_than_1024_sequences(dev):
    """B = 1 030 at S = 9: the persistent kernel stands down; against fp64, not against another kernel."""
    B, S, nh = 1030, 9, 2
    qkv = _randn((B * S, 3 * nh * 64), torch.Generator().manual_seed(1030), 1.0)
    raw = torch.ones(B, S)
    raw[::3, 5:] = 0
    run_case(dev, "B=1030 S=9", qkv, B, S, nh, mask=raw, bias64=(1.0 - raw.double()) * -10000.0)
