"""The rollout caller's kernels (csrc/rollout.hip: lstm_step_kernel, lstm_step_bwd_kernel, softdot_kernel, softdot_bwd_kernel<1|2>,
softdot_bwd_dots / softdot_bwd_apply<1|2>, skinny_linear_kernel<GRID>; csrc/lstm_persistent.hip: lstm_persistent_kernel) against the
float64 references and the derived per-element bounds of tests/helpers_rollout.py.
Alone:  python -m pytest tests/test_gpu_rollout_conformance.py -m gpu -q -s

Every strided input is a view of a NaN-filled buffer (a load outside a row's columns would poison the result) that must hold the
same bits afterwards; every strided output is a view of a sentinel-filled buffer whose surroundings must still hold the sentinel.
measured / bound of every check goes through helpers.check_close against 1 (the worst case of a group per name; the cases that
fail are listed in the assertion); exact contracts carry the bound 0 inside the judge (any difference is an infinite ratio) or
are torch.equal / isnan assertions.  Sequences are never asked to survive a chaotic recurrence: a sequence call must equal, bit
for bit, the chain of single-step calls issued here on the same buffers, and each step of that chain is held to the one-step
bound from the kernel's own previous state."""
import collections

import pytest
import torch

import helpers_rollout as hr
from helpers import check_close

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENT = hr.SENTINEL


class Tally(object):
    """worst ratio per check name of a test; failures keep the case's name"""

    def __init__(self, group):
        self.group, self.top, self.where = group, collections.OrderedDict(), {}

    def add(self, case_name, rs):
        for k, v in rs.items():
            v = hr.INF if v != v else v
            if v >= self.top.get(k, -1.0):
                self.top[k], self.where[k] = v, case_name

    def exact(self, case_name, what, ok):
        self.add(case_name, {what: 0.0 if ok else hr.INF})

    def finish(self):
        failed = []
        for k, v in self.top.items():
            print("ROLLOUT-GPU %s | %s | %.3f | %s" % (self.group, k, v, self.where[k]))
            try:
                check_close("rollout conformance %s: %s: error / bound" % (self.group, k), v, 0.0, 1.0)
            except AssertionError as e:
                failed.append("%s (worst case: %s)" % (e, self.where[k]))
        assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).clone()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _view(buf, dev, like):
    """the device twin of a CPU strided view `like` of the flat CPU buffer `buf`"""
    d = buf.to(dev)
    return d, torch.as_strided(d, like.shape, like.stride(), like.storage_offset())


# =====================================================================================================================================
# soft-dot attention
# =====================================================================================================================================
def _sd_groups():
    g = collections.OrderedDict()
    for c in hr.cases("softdot"):
        g.setdefault("%s%s" % (c.path, " long" if c.L >= 40 else ""), []).append(c)
    return g


SD_GROUPS = _sd_groups()
SELECTIONS = (("weighted only", True, False, True), ("probabilities", True, True, True), ("logits", True, True, False),
              ("logits alone", False, True, False))


@pytest.mark.parametrize("group", list(SD_GROUPS))
def test_softdot_attention_forward(dev, group):
    from visitron_amd import ops

    tally = Tally("softdot_kernel %s" % group)
    for case in SD_GROUPS[group]:
        I = hr.softdot_inputs(case)
        outs, _ = hr.case_terms(case)
        buf, ctx = _view(I.buf, dev, I.ctx)
        before = _bits(buf)
        t = I.t.to(dev)
        mask = None if I.mask is None else I.mask.to(dev)
        for sel, ww, wa, prob in SELECTIONS:
            weighted, attn = ops.softdot_attention(t, ctx, mask, ww, wa, prob)
            got = {}
            if ww:
                got["weighted"] = weighted
            if wa:
                got["p" if prob else "logit"] = attn
            tally.add("%s, %s" % (case.name, sel), hr.judge(outs, got))
        tally.exact(case.name, "the context buffer is untouched", torch.equal(before, _bits(buf)))
    tally.finish()


@pytest.mark.parametrize("group", list(SD_GROUPS))
def test_softdot_attention_backward_in_both_forms(dev, group):
    from visitron_amd import ops

    tally = Tally("softdot_bwd %s" % group)
    keep = ops.SOFTDOT_SPLIT_KEYS
    try:
        for case in SD_GROUPS[group]:
            I = hr.softdot_inputs(case)
            buf, ctx = _view(I.buf, dev, I.ctx)
            before = _bits(buf)
            t = I.t.to(dev)
            mask = None if I.mask is None else I.mask.to(dev)
            for sub in case.bwd:
                prob, gsel = sub
                outs, _ = hr.case_terms(case, sub)
                dw = I.dw.to(dev) if gsel in ("dw", "both") else None
                da = I.da.to(dev) if gsel in ("da", "both") else None
                res = {}
                for form, split in (("one workgroup", 1 << 30), ("two launches", 1)):
                    ops.SOFTDOT_SPLIT_KEYS = split
                    for want_ctx in (True, False):
                        d_t, d_c = ops.softdot_attention_bwd(t, ctx, mask, dw, da, prob, want_ctx)
                        got = {"d_target": d_t}
                        if want_ctx:
                            got["d_context"] = d_c
                            res[form] = got
                        else:
                            assert d_c is None
                        tally.add("%s, %s, %s, %s" % (case.name, "prob" if prob else "logit", gsel, form),
                                  hr.judge(outs, got, prefix="%s " % form))
                for k in ("d_target", "d_context"):      # the two forms against each other: within twice the bound
                    a, b, O = res["one workgroup"][k].cpu().double(), res["two launches"][k].cpu().double(), outs[k]
                    fin = torch.isfinite(O.y)
                    tally.exact(case.name, "both forms %s NaN in the same places" % k, torch.equal(torch.isnan(a), torch.isnan(b)))
                    err = (a - b)[fin].abs()
                    err = torch.where(torch.isnan(err), torch.full_like(err, hr.INF), err)
                    r = torch.where(err == 0, torch.zeros_like(err), err / (2 * O.bound[fin]))
                    tally.add(case.name, {"both forms %s difference / twice the bound" % k: float(r.max()) if r.numel() else 0.0})
            tally.exact(case.name, "the context buffer is untouched", torch.equal(before, _bits(buf)))
    finally:
        ops.SOFTDOT_SPLIT_KEYS = keep
    tally.finish()


# =====================================================================================================================================
# skinny linear
# =====================================================================================================================================
@pytest.mark.parametrize("form", hr.SK_FORMS)
def test_skinny_linear(dev, form):
    from visitron_amd import ops

    tally = Tally("skinny_linear_kernel<%s>" % ("GRID" if form == "grid" else "by address, %s" % form))
    for case in hr.cases("skinny"):
        if case.form != form:
            continue
        I = hr.skinny_inputs(case)
        outs, _ = hr.case_terms(case)
        b0, x0 = _view(I.buf0, dev, I.x0)
        b1, x1 = _view(I.buf1, dev, I.x1) if I.x1 is not None else (None, None)
        wb = I.wbuf.to(dev)
        w = wb[:, :case.Kpad]
        out = ops.skinny_linear(x0, w, None if I.bias is None else I.bias.to(dev), x1, ops.ACT_TANH if case.tanh else ops.ACT_NONE)
        tally.add(case.name, hr.judge(outs, {"out": out}))
        ok = _same(b0.cpu(), I.buf0) and (b1 is None or _same(b1.cpu(), I.buf1)) and _same(wb.cpu(), I.wbuf)
        tally.exact(case.name, "the input buffers are untouched", ok)
    tally.finish()


# =====================================================================================================================================
# LSTM step, forward
# =====================================================================================================================================
def _lstm_step_device(I, dev, train):
    """one step through ops.lstm_step (train = False) or vt_lstm_step_train_f32 (train = True): xproj and seq_out strided views"""
    from visitron_amd import _lib, ops

    B, hs = I["h"].shape
    xbuf = torch.full((B, 4 * hs + 5), float("nan"), device=dev)
    x = xbuf[:, 3:3 + 4 * hs]
    x.copy_(I["x"])
    sbuf = torch.full((B, 2 * hs + 3), SENT, device=dev)
    seq = sbuf[:, 1:1 + hs]
    h, c, w = I["h"].to(dev), I["c"].to(dev).clone(), I["w"].to(dev)
    h_out = torch.full((B, hs), SENT, device=dev)
    lens = None if I["lens"] is None else I["lens"].to(dev)
    r = dict(xbuf=xbuf, sbuf=sbuf, seq=seq, h_out=h_out, c=c)
    if not train:
        ops.lstm_step(x, h, h_out, c, w, I["t"], lens, seq)
        return r
    r["sv_g"] = torch.full((B, 4 * hs), SENT, device=dev)
    r["sv_c"] = torch.full((B, hs), SENT, device=dev)
    r["sv_h"] = torch.full((B, hs), SENT, dtype=BF16, device=dev)
    p = ops._ptr
    rc = _lib.load().vt_lstm_step_train_f32(p(x), x.stride(0), p(h), p(h_out), p(c), p(w), p(lens), p(seq), seq.stride(0), B, hs,
                                            int(I["t"]), p(r["sv_g"]), p(r["sv_c"]), p(r["sv_h"]), ops._stream())
    _lib.check(rc, "vt_lstm_step_train_f32")
    return r


def test_lstm_step_forward(dev):
    tally = Tally("lstm_step_kernel")
    for case in hr.cases("lstm"):
        I = hr.lstm_inputs(case)
        outs, V = hr.case_terms(case)
        B, hs = case.B, case.hs
        act = V["act"]
        a = _lstm_step_device(I, dev, False)
        b = _lstm_step_device(I, dev, True)
        tally.add(case.name, hr.judge(outs, {"h_out": a["h_out"], "c_out": a["c"], "seq_out": a["seq"]}))
        # exact contracts (inactive rows carry the bound 0 inside the judge as well: state passed through, output position zero)
        ina = ~act
        tally.exact(case.name, "an inactive row passes h and c through bit for bit",
                    _same(a["h_out"].cpu()[ina], I["h"][ina]) and _same(a["c"].cpu()[ina], I["c"][ina]))
        tally.exact(case.name, "an inactive row's output position is exactly zero", bool((a["seq"].cpu()[ina] == 0).all()))
        same = all(_same(a[k], b[k]) for k in ("h_out", "c", "sbuf", "xbuf"))
        tally.exact(case.name, "the train form's h, c and seq_out are the plain form's bit for bit", same)
        tally.exact(case.name, "xproj is untouched", _same(a["xbuf"][:, 3:3 + 4 * hs].cpu(), I["x"]) and bool(torch.isnan(a["xbuf"][:, :3]).all())
                    and bool(torch.isnan(a["xbuf"][:, 3 + 4 * hs:]).all()))
        sb = a["sbuf"].cpu()
        tally.exact(case.name, "seq_out's neighbours hold the sentinel", bool((sb[:, :1] == SENT).all()) and bool((sb[:, 1 + hs:] == SENT).all()))
        svg = b["sv_g"].cpu()
        tally.add(case.name, hr.judge({"sv_g": _rows(outs["sv_g"], act)}, {"sv_g": svg[act]}))
        tally.exact(case.name, "sv_c equals the input c", _same(b["sv_c"].cpu()[act], I["c"][act]))
        tally.exact(case.name, "sv_h equals torch's .to(bfloat16) of h_prev", _same(b["sv_h"].cpu()[act], I["h"].to(BF16)[act]))
        untouched = bool((svg[ina] == SENT).all()) and bool((b["sv_c"].cpu()[ina] == SENT).all()) and bool((b["sv_h"].cpu()[ina].float() == SENT).all())
        tally.exact(case.name, "saves of inactive rows are untouched", untouched)
    tally.finish()


def _rows(O, sel):
    """an Out restricted to the batch rows `sel`"""
    R = hr.Out(O.y[sel], O.E[sel])
    R.bound = O.bound[sel]
    return R


# =====================================================================================================================================
# sequences: bit for bit the chain of single steps; every step of the chain inside the one-step bound
# =====================================================================================================================================
SEQ_T = 6
SEQ_LENS = (6, 1, 4, 6, 2, 3, 5, 1, 6, 2, 3, 4, 5, 6, 1, 2, 3)


def _seq_inputs(B, hs, S, seed):
    g = hr._gen("sequence %d %d %d" % (B, hs, seed))
    return dict(x=torch.randn(B, S, 4 * hs, generator=g), h=torch.randn(B, hs, generator=g) * 0.5, c=torch.randn(B, hs, generator=g),
                w=hr.lstm_weights(hs), lens=torch.tensor(SEQ_LENS[:B], dtype=torch.int32))


def _chain(ops, x, h0, c0, w, lens, T, reverse, seq):
    """T single-step launches on the sequence's own buffers -> (h, c, [(t, h_prev, c_prev) per step])"""
    B, hs = h0.shape
    hb = [h0.clone(), torch.empty_like(h0)]
    c = c0.clone()
    steps = []
    for i in range(T):
        t = T - 1 - i if reverse else i
        steps.append((t, hb[i & 1].clone(), c.clone()))
        ops.lstm_step(x[:, t], hb[i & 1], hb[(i + 1) & 1], c, w, t, lens, None if seq is None else seq[:, t])
    return hb[T & 1], c, steps


def _hold_steps(tally, name, steps, x, w, lens, T, reverse, seq, h_fin, c_fin):
    """each step of a chain against float64 from the kernel's own previous h and c"""
    for n, (t, hp, cp) in enumerate(steps):
        act = None if lens is None else (t < lens.cpu().to(torch.int64))
        outs, _ = hr.lstm_terms(x[:, t].cpu().double(), hp.cpu().double(), cp.cpu().double(), w.cpu().double(), act)
        nxt = steps[n + 1] if n + 1 < len(steps) else (None, h_fin, c_fin)
        tally.add("%s, step at position %d" % (name, t), hr.judge(outs, {"h_out": nxt[1], "c_out": nxt[2], "seq_out": seq[:, t]}, prefix="chain "))


@pytest.mark.parametrize("reverse", (False, True))
def test_lstm_sequences_equal_their_step_chains(dev, reverse):
    from visitron_amd import ops

    tally = Tally("lstm sequences %s" % ("reverse" if reverse else "forward"))
    B, hs, S, T = 17, 128, SEQ_T + 1, SEQ_T
    I = _seq_inputs(B, hs, S, 0)
    x, w, lens = I["x"].to(dev), I["w"].to(dev), I["lens"].to(dev)
    keep = ops.LSTM_PERSISTENT
    ops.LSTM_PERSISTENT = False
    try:
        for ragged in (True, False):
            ln = lens if ragged else None
            name = "lstm_sequence%s" % (" ragged" if ragged else "")
            h0, c0 = I["h"].to(dev), I["c"].to(dev)
            sbuf_c = torch.full((B, T + 1, 2 * hs), SENT, device=dev)
            h_c, c_c, steps = _chain(ops, x, h0, c0, w, ln, T, reverse, sbuf_c[:, :T, hs:])
            sbuf = torch.full((B, T + 1, 2 * hs), SENT, device=dev)
            h2 = (h0.clone(), torch.full_like(h0, SENT))
            c = c0.clone()
            ops.lstm_sequence(x, h2, c, w, T, ln, sbuf[:, :T, hs:], reverse=reverse)
            tally.exact(name, "the sequence call equals its chain of steps bit for bit", _same(h2[0], h_c) and _same(c, c_c) and _same(sbuf, sbuf_c))
            tally.exact(name, "seq_out's neighbours hold the sentinel", bool((sbuf[:, :, :hs] == SENT).all()) and bool((sbuf[:, T:] == SENT).all()))
            _hold_steps(tally, name, steps, x, w, ln, T, reverse, sbuf_c[:, :T, hs:], h_c, c_c)
            if ragged:
                pad = torch.arange(T, device=dev)[None, :] >= lens[:, None]
                tally.exact(name, "zero padding past each length", bool((sbuf[:, :T, hs:][pad] == 0).all()))
                # the compacted layout: bitwise the padded one
                start = torch.cumsum(lens, 0, dtype=torch.int32) - lens
                rows = torch.full((int(lens.sum()) + 1, 4 * hs), float("nan"), device=dev)
                for b in range(B):
                    n = int(I["lens"][b])
                    rows[int(start[b]):int(start[b]) + n] = x[b, :n]
                sbuf_r = torch.full((B, T + 1, 2 * hs), SENT, device=dev)
                h2r, cr = (h0.clone(), torch.empty_like(h0)), c0.clone()
                ops.lstm_sequence_rows(rows[:-1], start.contiguous(), h2r, cr, w, T, lens, sbuf_r[:, :T, hs:], reverse=reverse)
                tally.exact("lstm_sequence_rows", "the compacted layout equals the padded one bit for bit",
                            _same(h2r[0], h_c) and _same(cr, c_c) and _same(sbuf_r, sbuf_c))
            # the training form: zero initial state, saves like the padded sequence
            z = torch.zeros_like(h0)
            sq_c = torch.full((B, T, hs), SENT, device=dev)
            h_z, c_z, steps_z = _chain(ops, x, z, z, w, ln, T, reverse, sq_c)
            seq_t, h_t, c_t, (sv_g, sv_c, sv_h) = ops.lstm_sequence_train(x, w, T, ln, reverse)
            tally.exact(name, "lstm_sequence_train equals its chain of steps bit for bit", _same(seq_t, sq_c) and _same(h_t, h_z) and _same(c_t, c_z))
            _hold_steps(tally, name + " (train)", steps_z, x, w, ln, T, reverse, sq_c, h_z, c_z)
            for t, hp, cp in steps_z:
                act = torch.ones(B, dtype=torch.bool) if ln is None else (t < I["lens"].to(torch.int64))
                outs, _ = hr.lstm_terms(x[:, t].cpu().double(), hp.cpu().double(), cp.cpu().double(), I["w"].double(), act)
                tally.add("%s (train), saves at position %d" % (name, t), hr.judge({"sv_g": _rows(outs["sv_g"], act)}, {"sv_g": sv_g[:, t].cpu()[act]},
                                                                                    prefix="chain "))
                tally.exact(name, "the sequence's sv_c and sv_h are the step's previous state",
                            _same(sv_c[:, t].cpu()[act], cp.cpu()[act]) and _same(sv_h[:, t].cpu()[act], hp.cpu().to(BF16)[act]))
    finally:
        ops.LSTM_PERSISTENT = keep
    tally.finish()


# =====================================================================================================================================
# LSTM step, backward
# =====================================================================================================================================
def _bwd_device(I, dev):
    """vt_lstm_step_bwd_f32 with every input explicit; the gate gradients land in sentinel-filled buffers with 8 spare columns"""
    from visitron_amd import _lib, ops

    B, hs = I["svc"].shape
    p = ops._ptr
    D = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in I.items()}
    dc = D["dc"].clone()
    g16 = torch.full((B, 4 * hs + 8), SENT, dtype=BF16, device=dev)
    g32 = torch.full((B, 4 * hs + 8), SENT, device=dev)
    ld = lambda t_: 0 if t_ is None else t_.stride(0)
    rc = _lib.load().vt_lstm_step_bwd_f32(p(D["dgn"]), ld(D["dgn"]), p(D["wt"]), p(D["dh_final"]), p(D["d_out"]), ld(D["d_out"]), p(dc),
                                          p(D["svg"]), ld(D["svg"]), p(D["svc"]), ld(D["svc"]), p(g16), g16.stride(0), p(g32), g32.stride(0),
                                          p(D["lens"]), B, hs, int(I["t"]), int(I["t_next"]), ops._stream())
    _lib.check(rc, "vt_lstm_step_bwd_f32")
    return g32, g16, dc


def test_lstm_step_backward(dev):
    tally = Tally("lstm_step_bwd_kernel")
    for case in hr.cases("lstm_bwd"):
        I = hr.lstm_bwd_inputs(case)
        outs, V = hr.case_terms(case)
        hs = case.hs
        g32, g16, dc = _bwd_device(I, dev)
        tally.add(case.name, hr.judge(outs, {"dg32": g32[:, :4 * hs], "dg16": g16[:, :4 * hs], "dc": dc}))
        ina = ~V["act"][:, 0]
        zero = bool((g32[:, :4 * hs].cpu()[ina] == 0).all()) and bool((g16[:, :4 * hs].cpu()[ina].float() == 0).all())
        tally.exact(case.name, "an inactive row writes exact-zero gate gradients and keeps dc", zero and _same(dc.cpu()[ina], I["dc"][ina]))
        tally.exact(case.name, "the gate gradients' neighbours hold the sentinel",
                    bool((g32[:, 4 * hs:] == SENT).all()) and bool((g16[:, 4 * hs:].float() == SENT).all()))
    tally.finish()


@pytest.mark.parametrize("reverse", (False, True))
def test_lstm_sequence_backward_equals_its_step_chain(dev, reverse):
    from visitron_amd import _lib, ops

    tally = Tally("lstm_sequence_bwd %s" % ("reverse" if reverse else "forward"))
    B, hs, S, T = 17, 128, SEQ_T + 1, SEQ_T
    I = _seq_inputs(B, hs, S, 1)
    g = hr._gen("sequence backward")
    x, w, lens = I["x"].to(dev), I["w"].to(dev), I["lens"].to(dev)
    wt = w.t().contiguous()
    d_seq = torch.randn(B, T, hs, generator=g).to(dev)
    dh_fin, dc_fin = torch.randn(B, hs, generator=g).to(dev), torch.randn(B, hs, generator=g).to(dev)
    p = ops._ptr
    for ragged in (True, False):
        ln = lens if ragged else None
        name = "lstm_sequence_bwd%s" % (" ragged" if ragged else "")
        _, _, _, saved = ops.lstm_sequence_train(x, w, T, ln, reverse)
        sv_g, sv_c, _ = saved
        dg = ops.lstm_sequence_bwd(d_seq, dh_fin, dc_fin, saved, wt, T, ln, reverse)
        chain = torch.zeros_like(dg)
        dc = dc_fin.clone()
        for i in range(T - 1, -1, -1):
            t = T - 1 - i if reverse else i
            tn = -1 if i == T - 1 else (t - 1 if reverse else t + 1)
            nxt = None if tn < 0 else dg[:, tn]
            g32 = torch.full((B, 4 * hs), SENT, device=dev)
            dc_in = dc.clone()
            rc = _lib.load().vt_lstm_step_bwd_f32(p(nxt), S * 4 * hs, p(wt), p(dh_fin), p(d_seq[:, t]), d_seq.stride(0), p(dc), p(sv_g[:, t]),
                                                  S * 4 * hs, p(sv_c[:, t]), S * hs, p(chain[:, t]), S * 4 * hs, p(g32), 4 * hs, p(ln), B, hs, t,
                                                  tn, ops._stream())
            _lib.check(rc, "vt_lstm_step_bwd_f32")
            J = dict(dgn=nxt, wt=wt, dh_final=dh_fin, d_out=d_seq[:, t], dc=dc_in, svg=sv_g[:, t], svc=sv_c[:, t], lens=ln, t=t, t_next=tn)
            J = hr.to64({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in J.items()})
            if ln is not None:        # rows the forward never ran hold uninitialised saves: they are inactive, their inputs do not count
                ina = ~(t < J["lens"].to(torch.int64))
                J["svg"], J["svc"] = J["svg"].clone(), J["svc"].clone()
                J["svg"][ina], J["svc"][ina] = 0.5, 0.0
            outs, _ = hr.lstm_bwd_terms(J)
            tally.add("%s, step at position %d" % (name, t), hr.judge(outs, {"dg32": g32, "dg16": chain[:, t], "dc": dc}, prefix="chain "))
        tally.exact(name, "the sequence call equals its chain of steps bit for bit", _same(dg, chain))
        tally.exact(name, "positions from T on stay zero", bool((dg[:, T:].float() == 0).all()))
    tally.finish()


# =====================================================================================================================================
# the persistent recurrence
# =====================================================================================================================================
@pytest.mark.parametrize("B,hs", [(21, 128), (5, 256)])
def test_lstm_persistent_recurrence(dev, B, hs):
    from visitron_amd import ops

    T = 5
    tally = Tally("lstm_persistent_kernel<%d, %d>" % (hs // 128, (B + 15) // 16))
    g = hr._gen("persistent %d %d" % (B, hs))
    xc = torch.randn(B, T + 1, 4 * hs, generator=g)
    h0c, c0c = torch.randn(B, hs, generator=g) * 0.5, torch.randn(B, hs, generator=g)
    wc = hr.lstm_weights(hs)
    lens_c = torch.tensor([(5, 1, 3, 5, 2, 4)[b % 6] for b in range(B)], dtype=torch.int32)
    x, h0, c0, w, lens = xc.to(dev), h0c.to(dev), c0c.to(dev), wc.to(dev), lens_c.to(dev)
    keep = ops.LSTM_PERSISTENT
    ops.LSTM_PERSISTENT = True
    try:
        def run(xv, ln, Tn, reverse):
            sbuf = torch.full((B, Tn + 1, 2 * hs), SENT, device=dev)
            h2, c = (h0.clone(), torch.empty_like(h0)), c0.clone()
            ops.lstm_sequence(xv, h2, c, w, Tn, ln, sbuf[:, :Tn, hs:], reverse=reverse)
            ok = bool((sbuf[:, :, :hs] == SENT).all()) and bool((sbuf[:, Tn:] == SENT).all())
            return h2[0], c, sbuf[:, :Tn, hs:], ok

        for reverse in (False, True):
            name = "persistent %s" % ("reverse" if reverse else "forward")
            ops.profile_begin()
            full = run(x, lens, T, reverse)
            prof = ops.profile_end()
            assert "lstm_persistent" in prof and "lstm_step" not in prof, \
                "the persistent kernel did not serve the call (a time-out and fall-back to the step launches is a finding): %s" % sorted(prof)
            tally.exact(name, "seq_out's neighbours hold the sentinel", full[3])
            pad = torch.arange(T, device=dev)[None, :] >= lens[:, None]
            tally.exact(name, "zero padding past each length", bool((full[2][pad] == 0).all()))
            # the prefixes T' = 1 .. T from the same initial state expose the state after every step
            prev = (h0, c0)
            for k in range(1, T + 1):
                if reverse:       # the first k steps of the full run: positions T-1 .. T-k
                    ln_k = (lens - (T - k)).clamp(0, k).to(torch.int32).contiguous()
                    h_k, c_k, s_k, ok = run(x[:, T - k:], ln_k, k, True)
                    t, common, mine = T - k, full[2][:, T - k:], s_k
                else:
                    h_k, c_k, s_k, ok = run(x, lens, k, False)
                    t, common, mine = k - 1, full[2][:, :k], s_k
                tally.exact(name, "a prefix agrees with the full run bit for bit on their common positions", ok and _same(common.contiguous(), mine.contiguous()))
                act = t < lens_c.to(torch.int64)
                outs, _ = hr.lstm_terms(xc[:, t].double(), prev[0].cpu().double(), prev[1].cpu().double(), wc.double(), act)
                tally.add("%s, step at position %d" % (name, t), hr.judge(outs, {"h_out": h_k, "c_out": c_k, "seq_out": full[2][:, t]}, prefix="step "))
                prev = (h_k, c_k)
            tally.exact(name, "the last prefix is the full run", _same(prev[0], full[0]) and _same(prev[1], full[1]))
            # the compacted layout: the same bits
            start = (torch.cumsum(lens, 0, dtype=torch.int32) - lens).contiguous()
            rows = torch.full((int(lens.sum()) + 1, 4 * hs), float("nan"), device=dev)
            for b in range(B):
                n = int(lens_c[b])
                rows[int(start[b]):int(start[b]) + n] = x[b, :n]
            sbuf = torch.full((B, T + 1, 2 * hs), SENT, device=dev)
            h2, c = (h0.clone(), torch.empty_like(h0)), c0.clone()
            ops.profile_begin()
            ops.lstm_sequence_rows(rows[:-1], start, h2, c, w, T, lens, sbuf[:, :T, hs:], reverse=reverse)
            prof = ops.profile_end()
            assert "lstm_persistent" in prof and "lstm_step" not in prof, sorted(prof)
            tally.exact(name, "the compacted layout equals the padded one bit for bit",
                        _same(h2[0], full[0]) and _same(c, full[1]) and _same(sbuf[:, :T, hs:].contiguous(), full[2].contiguous())
                        and bool((sbuf[:, :, :hs] == SENT).all()) and bool((sbuf[:, T:] == SENT).all()))
    finally:
        ops.LSTM_PERSISTENT = keep
    tally.finish()
