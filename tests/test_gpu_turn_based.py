"""GPU: the turn-based decoder step (csrc/turn_based.hip, visitron_amd/turn_based.py).

Part 1 holds the fused cell to the float64 restatement and per-element bounds of tests/helpers_turn_based.py; part 2 holds the
modules to the reference's recorded outputs and gradients (tests/golden/ref_turn_based.npz, written by
tests/golden/make_golden_turn_based.py) and the action head to its restatement.  Every ratio is printed before it is asserted
(run with -s; profiles/r14/turn_based.txt keeps the lines of one run)."""
import math
import os

import numpy as np
import pytest
import torch

import helpers_turn_based as ht
from helpers import check_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
NAN = float("nan")


def _record(name, rs):
    print("RATIOS %-44s %s" % (name, "  ".join("%s=%.3f" % (k, v) for k, v in sorted(rs.items()))))


# ---- operands as views inside NaN-filled buffers, outputs inside sentinel-filled ones ------------------------------------------
def _rows_view(t, dev, fill=NAN, lead=1, pad=3):
    """[R, C] -> a view at row 1, column `lead` of a filled [R + 2, C + pad] buffer: rows 4-byte aligned only, odd stride."""
    R, C = t.shape
    buf = torch.full((R + 2, C + pad), fill, dtype=t.dtype, device=dev)
    v = buf[1:R + 1, lead:lead + C]
    v.copy_(t)
    return v


def _flat_view(t, dev, fill=NAN, guard=64):
    """A contiguous copy `guard` elements into a filled 1-D buffer (16-byte aligned for guard % 8 == 0)."""
    buf = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device=dev)
    v = buf[guard:guard + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _packed_w_ih(w_ih, dev):
    """bf16 [G, Kpad] view (zero past K, Kpad = K rounded up to 32) inside a NaN buffer with a row stride of Kpad + 8."""
    G, K = w_ih.shape
    Kpad = (K + 31) // 32 * 32
    buf = torch.full((G + 2, Kpad + 8), NAN, dtype=BF16, device=dev)
    v = buf[1:G + 1, 8:8 + Kpad]
    v.zero_()
    v[:, :K] = w_ih.to(BF16)
    return v


class _Out(object):
    """[B, W] output inside a sentinel buffer with one guard row before and after."""

    def __init__(self, B, W, dev, dtype=torch.float32):
        self.buf = torch.full(((B + 2) * W,), ht.SENTINEL, dtype=dtype, device=dev)
        self.view = self.buf[W:(B + 1) * W].view(B, W)
        self.B, self.W = B, W

    def guard(self):
        g = self.buf.view(self.B + 2, self.W)
        return torch.stack((g[0], g[-1])).float().cpu()


def _run_cell(o, dev, save, h_out_is_h_prev=False):
    from visitron_amd import ops

    if o.ids is not None:
        idbuf = torch.full((o.B + 2,), 10 ** 9, dtype=torch.int64, device=dev)
        idbuf[1:o.B + 1] = o.ids.to(dev)
        first = (idbuf[1:o.B + 1], _rows_view(o.table, dev))
    else:
        first = _rows_view(o.x_emb, dev)
    feature = _rows_view(o.feature, dev, lead=2)
    h_prev, c_prev = _flat_view(o.h_prev, dev), _flat_view(o.c_prev, dev)
    w_ih = _packed_w_ih(o.w_ih, dev)
    w_hh = _flat_view(o.w_hh.to(BF16), dev)
    bias = _flat_view((o.b_ih + o.b_hh), dev)
    h_out, c_out = _Out(o.B, o.hs, dev), _Out(o.B, o.hs, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if h_out_is_h_prev:
        return ops.turn_lstm_cell(first, feature, h_prev, c_prev, w_ih, w_hh, bias, h_out=h_prev, c_out=c_out.view, err_flag=err)
    sv = (_Out(o.B, 4 * o.hs, dev), _Out(o.B, o.hs, dev), _Out(o.B, o.hs, dev, dtype=BF16)) if save else None
    _, _, saved = ops.turn_lstm_cell(first, feature, h_prev, c_prev, w_ih, w_hh, bias, h_out=h_out.view, c_out=c_out.view,
                                     save=tuple(b.view for b in sv) if save else False, err_flag=err)
    torch.cuda.synchronize()
    got = dict(h=h_out.view.cpu(), c=c_out.view.cpu(), gates=None if saved is None else saved[0].cpu(),
               c_prev_after=c_prev.cpu(), h_guard=h_out.guard(), c_guard=c_out.guard(), err=int(err.item()), saved=saved,
               h_prev_after=h_prev.cpu())
    if save:   # the saves' surroundings count as guard rows of the results
        got["h_guard"] = torch.cat((got["h_guard"].reshape(-1), sv[1].guard().reshape(-1), sv[2].guard().reshape(-1)))
        got["c_guard"] = torch.cat((got["c_guard"].reshape(-1), sv[0].guard().reshape(-1)))
    return got


CELL_CASES = [(B, hs, E, F) for hs in (128, 512) for (E, F) in ((8, 70), (64, 2054), (64, 2052), (3, 5)) for B in (1, 16, 17, 21)]


@pytest.mark.parametrize("B,hs,E,F", CELL_CASES)
def test_cell_against_float64(dev, B, hs, E, F):
    """Both entry forms (ids + table without saves, ready block with saves) within every bound; caller's buffers untouched."""
    o = ht.cell_operands(B, hs, E, F, seed=B + hs + E + F)
    ref = ht.cell_reference(o)
    got = _run_cell(o, dev, save=False)
    rs = ht.cell_ratios(o, ref, got)
    _record("cell ids   B=%d hs=%d E=%d F=%d" % (B, hs, E, F), rs)
    assert got["err"] == 0 and torch.equal(got["h_prev_after"], o.h_prev)
    ob = ht.cell_operands(B, hs, E, F, seed=B + hs + E + F, block=True)
    gotb = _run_cell(ob, dev, save=True)
    rsb = ht.cell_ratios(ob, ref, gotb)
    _record("cell block B=%d hs=%d E=%d F=%d" % (B, hs, E, F), rsb)
    assert ht.passes(rs), rs
    assert ht.passes(rsb), rsb
    sv_g, sv_c, sv_h = gotb["saved"]
    assert torch.equal(sv_c.cpu(), o.c_prev) and torch.equal(sv_h.cpu(), ref.h_prev16)
    assert torch.equal(gotb["h"], got["h"]) and torch.equal(gotb["c"], got["c"])      # the two forms: the same arithmetic


def test_cell_signed_bias(dev):
    """Non-negative activations and weights: a truncating bf16 convert would push every gate the same way."""
    o = ht.cell_operands(21, 512, 64, 2054, seed=7, kind="positive", block=True)
    rs = ht.cell_ratios(o, ht.cell_reference(o), _run_cell(o, dev, save=True), signed=True)
    _record("cell positive B=21 hs=512 E=64 F=2054", rs)
    assert ht.passes(rs), rs


@pytest.mark.parametrize("B,hs,E,F", [(17, 128, 3, 5), (5, 512, 64, 2054)])
def test_cell_exact_construction(dev, B, hs, E, F):
    """Small integers, every pre-activation zero: i = f = o = 1/2, g = 0, so c' = c / 2 bit for bit and h' = tanh(c / 2) / 2."""
    o = ht.cell_operands(B, hs, E, F, seed=3, kind="exact")
    got = _run_cell(o, dev, save=True)
    assert torch.equal(got["c"], o.c_prev * 0.5)
    g = got["gates"]
    assert torch.equal(g[:, :2 * hs], torch.full((B, 2 * hs), 0.5)) and torch.equal(g[:, 3 * hs:], torch.full((B, hs), 0.5))
    assert bool((g[:, 2 * hs:3 * hs] == 0).all())
    rs = ht.cell_ratios(o, ht.cell_reference(o), got)
    assert ht.passes(rs), rs


def test_cell_out_of_range_id_raises_and_neighbours_are_unchanged(dev):
    from visitron_amd import modeling

    o = ht.cell_operands(17, 128, 8, 70, seed=11)
    good = _run_cell(o, dev, save=False)
    bad_rows = (3, 16)
    o.ids = o.ids.clone()
    o.ids[3], o.ids[16] = o.A, -1
    got = _run_cell(o, dev, save=False)
    assert got["err"] == 1
    keep = [r for r in range(o.B) if r not in bad_rows]
    assert torch.equal(got["h"][keep], good["h"][keep]) and torch.equal(got["c"][keep], good["c"][keep])
    rs = ht.cell_ratios(o, ht.cell_reference(o), got)      # the bad rows: the embedding counts as zero
    assert ht.passes(rs), rs
    modeling.check_errors()                                  # nothing pending from the op-level calls
    err = torch.ones(1, dtype=torch.int32, device=dev)
    modeling._post_index_flag(err)
    with pytest.raises(IndexError):
        modeling.check_errors()


def test_module_out_of_range_action_raises_index_error(dev):
    from visitron_amd import modeling
    from visitron_amd.turn_based import AttnDecoderLSTM

    dec = AttnDecoderLSTM(8, 6, 8, 128, 0.0, feature_size=70).to(dev).eval()
    B = 3
    args = (torch.rand(B, 70, device=dev), torch.zeros(B, 128, device=dev), torch.zeros(B, 128, device=dev),
            torch.rand(B, 4, 128, device=dev))
    with torch.no_grad():
        dec(torch.tensor([[1], [2], [3]], device=dev), *args)
        modeling.check_errors()
        with pytest.raises(IndexError):
            dec(torch.tensor([[1], [8], [3]], device=dev), *args)
            modeling.check_errors()


def test_cell_refuses_h_out_aliasing_h_prev(dev):
    o = ht.cell_operands(4, 128, 8, 70, seed=1)
    with pytest.raises(RuntimeError, match="unsupported"):
        _run_cell(o, dev, save=False, h_out_is_h_prev=True)


# ---- part 2: the modules against the reference's fixture -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ref_turn_based.npz")))


def _decoder(fx, dev, dropout=0.0):
    from visitron_amd.turn_based import AttnDecoderLSTM

    sd = {k[3:]: torch.from_numpy(v.astype(np.float32)) for k, v in fx.items() if k.startswith("sd.")}
    A_in, E = sd["embedding.weight"].shape
    A_out, hs = sd["decoder2action.weight"].shape
    dec = AttnDecoderLSTM(A_in, A_out, E, hs, dropout, feature_size=sd["lstm.weight_ih"].shape[1] - E)
    dec.load_state_dict(sd)
    return dec.to(dev)


def _t(fx, k, dev):
    return torch.from_numpy(fx[k]).to(dev)


def test_softdot_attention_matches_the_reference(dev, fx):
    att = _decoder(fx, dev).attention_layer.eval()
    h, ctx, mask = _t(fx, "h0", dev), _t(fx, "ctx", dev), _t(fx, "mask", dev)
    with torch.no_grad():
        for tag, m in (("nomask", None), ("mask", mask)):
            h_tilde, attn = att(h, ctx, m)
            check_close("turn_based softdot %s h_tilde" % tag, h_tilde, fx["attn.%s.h_tilde" % tag], 5e-2)
            check_close("turn_based softdot %s attn" % tag, attn, fx["attn.%s.attn" % tag], 2e-2)
            if m is not None:
                assert bool((attn[m.bool()] == 0).all())
            assert abs(float(attn.sum(1).mean()) - 1.0) < 1e-5


def test_decoder_two_steps_match_the_reference(dev, fx):
    dec = _decoder(fx, dev).eval()
    ctx, mask = _t(fx, "ctx", dev), _t(fx, "mask", dev)
    h, c = _t(fx, "h0", dev), _t(fx, "c0", dev)
    h_in, c_in = h.clone(), c.clone()
    with torch.no_grad():
        for i in range(2):
            h1, c1, alpha, logit = dec(_t(fx, "action%d" % i, dev), _t(fx, "feature%d" % i, dev), h, c, ctx, mask)
            if i == 0:
                assert torch.equal(h, h_in) and torch.equal(c, c_in)        # the caller's state is never written
            check_close("turn_based step %d h_1" % i, h1, fx["step.%d.h_1" % i], 5e-2)
            check_close("turn_based step %d c_1" % i, c1, fx["step.%d.c_1" % i], 5e-2)
            check_close("turn_based step %d alpha" % i, alpha, fx["step.%d.alpha" % i], 2e-2)
            want = fx["step.%d.logit" % i]
            check_close("turn_based step %d logit" % i, logit, want, 2e-2 * max(1.0, float(np.abs(want).max())))
            assert bool((alpha[mask.bool()] == 0).all()) and logit.shape == want.shape
            h, c = h1, c1
        # one row is served as one row
        h1, c1, alpha, logit = dec(_t(fx, "action0", dev)[:1], _t(fx, "feature0", dev)[:1], h_in[:1], c_in[:1], ctx[:1], mask[:1])
        check_close("turn_based step 0 one row h_1", h1, fx["step.0.h_1"][:1], 5e-2)
        check_close("turn_based step 0 one row logit", logit, fx["step.0.logit"][:1],
                    2e-2 * max(1.0, float(np.abs(fx["step.0.logit"]).max())))


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-6 * (b.numel() ** 0.5)))


def test_training_gradients_match_the_reference(dev, fx):
    """Two teacher-forced steps under train() at dropout 0 through action_feedback, as agent.py:307-331 builds the loss."""
    from visitron_amd.turn_based import action_feedback

    dec = _decoder(fx, dev).train()
    ctx = _t(fx, "ctx", dev).requires_grad_()
    h0, c0 = _t(fx, "h0", dev).requires_grad_(), _t(fx, "c0", dev).requires_grad_()
    mask = _t(fx, "mask", dev)
    a_t = _t(fx, "action0", dev)
    h, c, loss = h0, c0, 0.0
    for i in range(2):
        h, c, alpha, logit = dec(a_t.view(-1, 1), _t(fx, "feature%d" % i, dev), h, c, ctx, mask)
        before = logit.detach().clone()
        target = _t(fx, "train.target%d" % i, dev)
        step_loss, nxt = action_feedback(logit, target, _t(fx, "train.blocked%d" % i, dev), ignore_index=-100, feedback="teacher")
        assert torch.equal(logit.detach(), before) and torch.equal(nxt, target)
        check_close("turn_based train loss step %d" % i, float(step_loss), float(fx["train.loss%d" % i]), 2e-2)
        loss = loss + step_loss
        a_t = torch.where(target == -100, torch.zeros_like(target), target)
    loss.backward()
    grads = {k: p.grad for k, p in dec.named_parameters()}
    grads.update(ctx=ctx.grad, h0=h0.grad, c0=c0.grad)
    for k, g in sorted(grads.items()):
        want = torch.from_numpy(fx["grad." + k].astype(np.float32)) * float(fx["gscale." + k])
        assert g is not None, k
        check_close("turn_based train grad %s rel-L2" % k, _rel(g, want), 0.0, 2e-2)


def test_training_at_the_shipped_sizes_with_dropout_and_adam(dev):
    """agent.py's loop at --aemb 64, --lstm_img_feature_dim 2054 (cell input 2118 = 2 mod 4), hidden 512, B = 8, L = 40: ten
    steps of visitron_amd.optim.Adam (weight_decay 0) on encoder and decoder, dropout 0.5, through action_feedback."""
    from oracle.modeling import PreTrainOscar as OModel
    from helpers import model_pair
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.optim import Adam
    from visitron_amd.turn_based import AttnDecoderLSTM, OscarEncoder, action_feedback

    cfg = mini_config(num_hidden_layers=2, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    _, prod = model_pair(OModel, PreTrainOscar, cfg, seed=43, device=dev)
    torch.manual_seed(12)
    enc = OscarEncoder(None, prod.bert, 512, 512, 0.5).to(dev).train()
    dec = AttnDecoderLSTM(8, 6, 64, 512, 0.5, feature_size=2054).to(dev).train()
    B, L = 8, 40
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(1, cfg.vocab_size, (B, L), generator=g).to(dev)
    lens = [40, 40, 33, 33, 21, 20, 9, 2]
    pad = torch.zeros(B, L, dtype=torch.uint8)
    for i, n in enumerate(lens):
        pad[i, n:] = 1
    pad = pad.to(dev)
    feats = [(torch.randn(B, 2054, generator=g).abs() * 0.5).to(dev) for _ in range(2)]
    targets = [torch.randint(0, 6, (B,), generator=g).to(dev) for _ in range(2)]
    targets[1][5] = -100
    blocked = torch.zeros(B, 6, dtype=torch.bool)
    blocked[2, 1] = True
    targets[0][2], targets[1][2] = 3, 4
    blocked = blocked.to(dev)
    start = torch.full((B,), 7, dtype=torch.int64, device=dev)

    def loss_of():
        ctx, h_t, c_t = enc(ids, lens, pad.bool())
        a_t, loss = start, 0.0
        for i in range(2):
            h_t, c_t, alpha, logit = dec(a_t.view(-1, 1), feats[i], h_t, c_t, ctx, pad[:, :ctx.shape[1]])
            step_loss, a_t = action_feedback(logit, targets[i], blocked, feedback="teacher")
            a_t = torch.where(a_t == -100, torch.zeros_like(a_t), a_t)
            loss = loss + step_loss
        return loss, logit

    with torch.no_grad():
        l1, l2 = loss_of()[1], loss_of()[1]
    assert not torch.equal(l1, l2)                       # two forward calls at dropout 0.5 differ
    opt_e, opt_d = Adam(enc.parameters(), lr=1e-3, weight_decay=0), Adam(dec.parameters(), lr=1e-3, weight_decay=0)
    losses = []
    for _ in range(10):
        opt_e.zero_grad()
        opt_d.zero_grad()
        loss, _ = loss_of()
        loss.backward()
        opt_e.step()
        opt_d.step()
        losses.append(float(loss))
    print("losses", losses)
    assert all(math.isfinite(l) for l in losses) and min(losses[-3:]) < losses[0], losses
    for n, p in dec.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


# ---- the action head ---------------------------------------------------------------------------------------------------------------
def test_action_head_sampling_matches_the_inverse_cdf(dev):
    """64 rows x 8 seeds: every row whose u is farther than 1e-5 from a CDF step takes the fp64 inverse CDF's action."""
    from visitron_amd.turn_based import action_feedback

    logit, target, blocked = ht.head_case(*ht.SAMPLE_CASE)
    B = logit.shape[0]
    lg, tg, bl = logit.to(dev), target.to(dev), blocked.to(dev)
    checked = 0
    for seed in ht.SAMPLE_SEEDS:
        _, a_t = action_feedback(lg, tg, bl, feedback="sample", seed=seed)
        want, safe = ht.head_sample(logit, blocked, seed)
        a = a_t.cpu()
        assert torch.equal(a[safe], want[safe])
        assert not bool(blocked[torch.arange(B), a].any())
        checked += int(safe.sum())
    assert checked >= 0.99 * B * len(ht.SAMPLE_SEEDS)
    _, again = action_feedback(lg, tg, bl, feedback="sample", seed=ht.SAMPLE_SEEDS[0])
    _, first = action_feedback(lg, tg, bl, feedback="sample", seed=ht.SAMPLE_SEEDS[0])
    assert torch.equal(again, first)                       # the same seed: the same actions


def _head_inputs(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    logit = torch.randn(B, A, generator=g) * 2.0
    if A > 1:
        logit[1 % B, :] = logit[1 % B, 0]                                  # a row of ties
        logit[2 % B, A - 1] = logit[2 % B].max()                           # the maximum twice
    blocked = torch.rand(B, A, generator=g) < 0.3                          # ragged
    blocked[torch.arange(B), torch.randint(0, A, (B,), generator=g)] = False   # at least one entry open per row
    target = torch.randint(0, A, (B,), generator=g)
    target[::4] = -100
    if A > 1:
        blocked[3 % B, target[3 % B].clamp(min=0)] = False
    return logit, target, blocked


@pytest.mark.parametrize("A", [1, 6, 15, 64])
@pytest.mark.parametrize("use_blocked", [False, True])
def test_action_head_against_float64(dev, A, use_blocked):
    from visitron_amd.turn_based import action_feedback

    B = 37
    logit, target, blocked = _head_inputs(B, A, 100 + A)
    if not use_blocked:
        blocked = None
    else:
        open_t = ~blocked[torch.arange(B), target.clamp(min=0)] | (target == -100)
        target = torch.where(open_t, target, torch.full_like(target, -100))     # blocked targets: their own test below
    ref = ht.head_reference(logit, target, blocked)
    lg = _rows_view(logit, dev).requires_grad_()
    before = lg.detach().clone()
    bl = None if blocked is None else blocked.to(dev)
    for mode in ("teacher", "argmax", "sample"):
        lg.grad = None
        loss, a_t = action_feedback(lg, target.to(dev), bl, feedback=mode, seed=12345)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and a_t.dtype == torch.int64 and a_t.shape == (B,)
        err = abs(float(loss) - ref.loss)
        print("RATIOS head A=%d blocked=%s %s loss err/bound=%.3f" % (A, use_blocked, mode, err / ref.loss_bound))
        assert err <= ref.loss_bound
        loss.backward()
        d = (lg.grad.cpu().double() - ref.dlogit).abs()
        assert bool((d <= ref.dlogit_bound).all()), float((d / ref.dlogit_bound).max())
        assert torch.equal(lg.detach(), before)                              # logit is not modified
        if mode == "teacher":
            assert torch.equal(a_t.cpu(), target)
        elif mode == "argmax":
            assert torch.equal(a_t.cpu(), ht.head_argmax(logit, blocked))
        else:
            want, safe = ht.head_sample(logit, blocked, 12345)
            assert torch.equal(a_t.cpu()[safe], want[safe]) and int(safe.sum()) >= B - 1
            if blocked is not None:
                assert not bool(blocked[torch.arange(B), a_t.cpu()].any())  # never a blocked entry


def test_action_head_corners(dev):
    """A blocked target gives +inf; no counted row gives NaN; seed=None draws a fresh seed per call."""
    from visitron_amd.turn_based import action_feedback

    logit, target, _ = _head_inputs(9, 6, 5)
    target = target.clamp(min=0)
    blocked = torch.zeros(9, 6, dtype=torch.uint8)
    blocked[4, target[4]] = 1
    loss, _ = action_feedback(logit.to(dev), target.to(dev), blocked.to(dev))
    assert float(loss) == math.inf
    loss, _ = action_feedback(logit.to(dev), torch.full((9,), -100, device=dev), None)
    assert math.isnan(float(loss))
    flat = torch.zeros(64, 64, device=dev)
    picks = [action_feedback(flat, torch.zeros(64, dtype=torch.int64, device=dev), feedback="sample")[1] for _ in range(2)]
    assert not torch.equal(picks[0], picks[1])
    assert len(set(picks[0].tolist())) > 16                                  # 64 rows over 64 equal actions
