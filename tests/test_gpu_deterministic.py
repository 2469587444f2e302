"""Deterministic training mode (visitron_amd.set_deterministic): fixed-order dQ and dW sums, no float atomics.

  1. the attention backward over more than 256 keys leaves one dQ partial per key block in the planes of its workspace and
     dq is their fp32 sum in ascending key-block order, rounded once (the contract of include/visitron_hip.h);
  2. it is the same gradient: inside the derived bound of tests/helpers_attention.py, dk / dv bit-equal to the default path;
  3. one and two key blocks give the default path's bits;
  4. the persistent weight-gradient kernel accumulates into the same bits on every call;
  5. two engines, and two models behind the autograd bridge, agree bit for bit over three steps at S = 513, and no GEMM
     tuning launch runs.
Alone:  python -m pytest tests/test_gpu_deterministic.py -q -s"""
import pytest
import torch

import helpers_attention as ha

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NH, H = 2, 128


@pytest.fixture()
def det():
    """The switch on for the test, off (the default) afterwards; the test turns it off and on itself where it compares modes."""
    from visitron_amd import ops

    ops.set_deterministic(True)
    try:
        yield ops
    finally:
        ops.set_deterministic(False)


# ---- attention backward ------------------------------------------------------------------------------------------------------
_cases = {}


def _case(dev, S, layout, drop):
    """One forward at B = 2, nh = 2 (kept per (S, layout, drop): every test below reads the same inputs and the same fp64
    reference).  layout "masked": padded rows, a raw key mask that masks sequence 1's whole last key block (and three keys of
    sequence 0); "seq": compacted rows of lengths {S, 300} ({S, 200} where S <= 300); "plain": padded, no mask."""
    from visitron_amd import ops

    key = (S, layout, drop)
    if key in _cases:
        return _cases[key]
    B = 2
    g = torch.Generator().manual_seed(5 * S + len(layout))
    qkv = torch.randn(B * S, 3 * H, generator=g).to(BF16).float()
    dctx = (torch.randn(B * S, H, generator=g) * 0.7).to(BF16).float()
    lens, mask, seq, index = None, None, None, torch.arange(B * S)
    bias = torch.zeros(B, S, dtype=ha.F64)
    if layout == "masked":
        mask = torch.ones(B, S)
        mask[1, ((S - 1) // 256) * 256:] = 0
        mask[0, 5:8] = 0
        bias = ((1.0 - mask) * -10000.0).to(ha.F64)
    elif layout == "seq":
        lens = [S, 300 if S > 300 else 200]
        keepm = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
        seq = ops.SeqLayout(keepm.to(dev))
        index = seq.index.cpu()
        qkv, dctx = qkv * keepm.reshape(-1, 1).float(), dctx * keepm.reshape(-1, 1).float()
        bias = ha.length_bias(lens, S)
    rows = index.numel()
    kw = dict(seq=seq) if seq is not None else dict(mask=None if mask is None else mask.to(dev))
    dr, p_eff, words, keep = ops.NO_DROP, 0.0, None, None
    if drop:
        dr, p_eff = (0.1, 777 + S, ops.site_attn(1)), ops.attn_drop_p(0.1)
        words = torch.zeros(ops.keep_words(B, NH, S), dtype=torch.int32, device=dev)
        keep = torch.zeros(B, NH, S, S)
        for b in range(B):
            n = lens[b] if lens else S
            for h in range(NH):
                keep[b, h, :n, :n] = ops.attn_dropout_mask(n, dr, b * NH + h, device=dev).float().cpu()
    qd, dd = qkv[index].to(dev, BF16).contiguous(), dctx[index].to(dev, BF16).contiguous()
    lse = torch.zeros((B, NH, S), dtype=torch.float32, device=dev)
    ctx = ops.attention_fwd(qd, B, S, NH, lse=lse, drop=dr, keep_bits=words, **kw)
    torch.cuda.synchronize()

    def padded(x):   # kernel rows -> the padded geometry of the reference
        full = torch.zeros((B * S, x.shape[1]), dtype=torch.float32)
        full[index] = x.float().cpu()
        return full

    c = dict(B=B, S=S, rows=rows, lens=lens, qd=qd, dd=dd, ctx=ctx, lse=lse, dr=dr, words=words, kw=kw, padded=padded, terms=None)

    def terms():   # the fp64 reference and its margins, built on first use
        if c["terms"] is None:
            q, k, v = ha.split_qkv(qkv, B, S, NH)
            c["terms"] = ha.BackwardTerms(q, k, v, bias, ha.heads(dctx, B, S, NH), ha.heads(padded(ctx), B, S, NH), keep, p_eff)
        return c["terms"]

    c["get_terms"] = terms
    _cases[key] = c
    return c


def _bwd(c, ws=None, hash_keep=False):
    """hash_keep: the backward gets no keep words and re-derives the forward's decisions from the hash."""
    from visitron_amd import ops

    out = ops.attention_bwd(c["qd"], c["dd"], c["ctx"], c["lse"], c["B"], c["S"], NH, drop=c["dr"],
                            keep_bits=None if hash_keep else c["words"], dq32_ws=ws, **c["kw"])
    torch.cuda.synchronize()
    return out


LAYOUTS = [(513, "masked"), (513, "seq"), (767, "masked"), (767, "seq")]


@pytest.mark.parametrize("drop", [False, True], ids=["no dropout", "p=0.1"])
@pytest.mark.parametrize("S,layout", LAYOUTS)
def test_dq_is_the_ordered_sum_of_the_key_block_planes(dev, det, S, layout, drop):
    """Contract of vt_attention_bwd_bf16 under the switch: plane kb of the workspace holds key block kb's dQ partial for EVERY
    row (a NaN-filled workspace comes back without a NaN: no row is left to a zeroing pass) and dq = bf16((p0 + p1) + p2)."""
    c = _case(dev, S, layout, drop)
    nkb, rows = (S + 255) // 256, c["rows"]
    assert nkb == 3
    assert det.attention_bwd_ws_bytes(c["B"], S, NH, rows) == nkb * rows * H * 4
    ws = torch.full((nkb * rows * H,), float("nan"), device=dev)
    out = _bwd(c, ws)
    planes = ws.view(nkb, rows, H)
    assert not bool(torch.isnan(planes).any()), "a (plane, row) the kernels did not write"
    want = ((planes[0] + planes[1]) + planes[2]).to(BF16)
    assert torch.equal(out[:, :H], want)
    if layout == "seq":    # keys 512.. do not exist for the 300-row sequence: its rows of plane 2 are zeros
        assert float(planes[2, S:].abs().max()) == 0.0
    assert torch.equal(_bwd(c), out), "the library-sized workspace gives other bits than the caller's"


@pytest.mark.parametrize("drop", [False, True], ids=["no dropout", "p=0.1"])
@pytest.mark.parametrize("S,layout", LAYOUTS)
def test_same_gradient_as_the_default_path(dev, det, S, layout, drop):
    """dq, dk, dv under the switch against fp64 with the margins of tests/helpers_attention.py (the multipliers and the dS form
    of tests/test_gpu_attention_conformance.py for the kernel that serves several key blocks); dk and dv -- whose arithmetic
    the switch does not touch -- bit-equal to the default path."""
    import test_gpu_attention_conformance as conf

    c = _case(dev, S, layout, drop)
    on = _bwd(c)
    det.set_deterministic(False)
    off = _bwd(c)
    det.set_deterministic(True)
    assert torch.equal(on[:, H:], off[:, H:])
    gp = c["padded"](on)
    got = tuple(ha.heads(gp[:, i * H:(i + 1) * H], c["B"], S, NH) for i in range(3))
    ratios = ha.backward_ratios(c["get_terms"](), got, lens=c["lens"], ds_form=conf.DS_FORM[17])
    ha.assert_ratios("deterministic bwd S=%d %s%s" % (S, layout, " p=0.1" if drop else ""), ratios)


@pytest.mark.parametrize("S", [228, 257, 512])
def test_one_and_two_key_blocks_keep_their_bits(dev, det, S):
    """S <= 256 has no workspace and no second kernel in either mode; with two key blocks 0 + a + b (the atomics) and a + b
    (the planes) are the same fp32 number, so the modes must agree bit for bit: the plane sum adds nothing else."""
    for drop in (False, True):
        c = _case(dev, S, "plain", drop)
        assert det.attention_bwd_ws_bytes(c["B"], S, NH) == (0 if S <= 256 else 2 * c["rows"] * H * 4)
        on = _bwd(c)
        det.set_deterministic(False)
        off = _bwd(c)
        det.set_deterministic(True)
        assert torch.equal(on, off), "S=%d drop=%s" % (S, drop)


@pytest.mark.parametrize("drop", ["none", "keep words", "hash"])
@pytest.mark.parametrize("layout", ["masked", "seq"])
@pytest.mark.parametrize("waves", [4, 8, 10])
def test_every_key_block_kernel_under_the_switch(dev, det, waves, layout, drop):
    """The tests above run the default setting, which from two key blocks on is the 8-wave kernel forming delta itself, with keep
    words.  set_attn_bwd_waves 4 (the 4-wave kernel), 8 and 10 (the 8-wave kernel with delta in the kernel / from the separate
    pass), each without dropout, with the forward's keep words and with the decisions re-derived from the hash, reach every
    plane-storing instantiation.  S = 257 is the shortest length with two key blocks, the second of one key; in the compacted
    batch the second sequence has 200 rows, so key block 1 of it lies past its end and must store zeros.  Held to: the fp64
    reference with the margins of tests/helpers_attention.py; dq = bf16(p0 + p1) from a NaN-filled workspace; a second launch
    (library-sized workspace) with the same bits."""
    import test_gpu_attention_conformance as conf

    S = 257
    c = _case(dev, S, layout, drop != "none")
    rows, hash_keep = c["rows"], drop == "hash"
    ws = torch.full((2 * rows * H,), float("nan"), device=dev)
    det.set_attn_bwd_waves(waves)
    try:
        out = _bwd(c, ws, hash_keep)
        again = _bwd(c, None, hash_keep)
    finally:
        det.set_attn_bwd_waves(0)
    planes = ws.view(2, rows, H)
    assert not bool(torch.isnan(planes).any()), "a (plane, row) the kernels did not write"
    assert torch.equal(out[:, :H], (planes[0] + planes[1]).to(BF16))
    if layout == "seq":    # key 256 does not exist for the 200-row sequence: its rows of plane 1 are zeros
        assert rows == S + 200 and float(planes[1, S:].abs().max()) == 0.0
    assert torch.equal(again, out), "two launches differ"
    gp = c["padded"](out)
    got = tuple(ha.heads(gp[:, i * H:(i + 1) * H], c["B"], S, NH) for i in range(3))
    ratios = ha.backward_ratios(c["get_terms"](), got, lens=c["lens"], ds_form=conf.DS_FORM[waves])
    ha.assert_ratios("deterministic bwd waves %d S=%d %s %s" % (waves, S, layout, drop), ratios)


# ---- persistent weight gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1024, 256, 256), (2048, 256, 256), (4928, 2304, 2560)])
def test_wgrad_accumulates_in_a_fixed_order(dev, det, M, N, K):
    """vt_wgrad_bf16 behind hook 8 (the persistent kernel wherever it is eligible), with a bias, accumulating from a non-zero
    start.  By the host's rule (row ranges per tile = min(CUs / tiles, row blocks / 8), one instead of two up to 76 row blocks):
    N = K = 256, M = 1 024 is one tile of 16 row blocks in ONE range; M = 2 048 is 32 row blocks that the default mode cuts
    into four ranges (fp32 atomics): under the switch the launch goes to the one-tile kernel, the atomic form must not be
    reached; 2 304 x 2 560 at M = 4 928 is 90 tiles of 77 row blocks in TWO ranges on a 256-CU device -- the turn path, where
    range 1 waits for range 0.  Three calls from the same start must give the same bits, inside the bound
    tests/test_gpu_ops.py::test_wgrad_persistent_streamk_matches_plain_kernel_and_fp32 applies against fp64 dY^T X
    (2e-4 max|dW| + 1e-3; the fp64 product is formed on the device)."""
    ops = det
    g = torch.Generator().manual_seed(M)
    dyd = (torch.randn(M, N, generator=g) * 0.5).to(dev, BF16)
    xd = torch.randn(M, K, generator=g).to(dev, BF16)
    dw0, db0 = torch.randn(N, K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    w_dw, w_db = dyd.double().t() @ xd.double(), dyd.double().sum(0)
    ops.wgrad_turn_timeouts()
    ops.set_wgrad_kernel(8)
    try:
        runs = []
        for _ in range(3):
            p = dict(dy=dyd, x=xd, dw=dw0.clone(), db=db0.clone(), accumulate=True)
            ops.wgrad([p], M)
            torch.cuda.synchronize()
            runs.append((p["dw"], p["db"]))
    finally:
        ops.set_wgrad_kernel(0)
    assert ops.wgrad_turn_timeouts() == 0
    for dw, db in runs:
        assert torch.equal(dw, runs[0][0]) and torch.equal(db, runs[0][1])
        assert float((dw.double() - dw0.double() - w_dw).abs().max()) < 2e-4 * float(w_dw.abs().max()) + 1e-3
        assert float((db.double() - db0.double() - w_db).abs().max()) < 2e-4 * float(w_db.abs().max()) + 1e-3


# ---- the training step ---------------------------------------------------------------------------------------------------------
def _cfg_batch(dev):
    from visitron_amd.config import mini_config
    from visitron_amd.synth import make_batch

    cfg = mini_config(max_position_embeddings=512, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    batch = make_batch(cfg, 2, text_len=300, region_len=213)      # S = 513: three key blocks, the last of one key
    return cfg, {k: v.to(dev) for k, v in batch.items()}


def _model(cfg, dev):
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict

    torch.manual_seed(4321)   # the engine draws its dropout seed base from torch's seed
    m = PreTrainOscar(cfg)
    m.load_state_dict(deterministic_state_dict(m, seed=5))
    return m.to(dev).train()


def test_two_engines_agree_bit_for_bit(dev, det, monkeypatch, capsys):
    """Three AdamW steps of two engines built from the same weights, dropout on, S = 513: losses, parameters and both moments.
    No tuning launch runs under the switch: the tuner's report (VT_TUNE_VERBOSE) stays silent and no shape is marked as timed."""
    from visitron_amd.training import PretrainEngine

    monkeypatch.setenv("VT_TUNE_VERBOSE", "1")
    timed_before = set(det._timed_keys)
    cfg, batch = _cfg_batch(dev)
    res = []
    for _ in range(2):
        eng = PretrainEngine(_model(cfg, dev), lr=1e-3, weight_decay=0.05, schedule="constant", warmup_steps=0)
        losses = [eng.train_step(batch)[0].detach().clone() for _ in range(3)]
        torch.cuda.synchronize()
        assert eng.state_dict()["hyper"]["deterministic"] is True
        assert eng._bufs[(2, 513)].ws_t["dq32"].numel() * 4 == det.attention_bwd_ws_bytes(2, 513, cfg.num_attention_heads)
        res.append((losses, eng.flat.p.clone(), eng.flat.m.clone(), eng.flat.v.clone()))
    assert "tune M=" not in capsys.readouterr().out and set(det._timed_keys) == timed_before
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    for i, what in ((1, "parameters"), (2, "exp_avg"), (3, "exp_avg_sq")):
        assert torch.equal(res[0][i], res[1][i]), what
    assert bool(torch.isfinite(res[0][1]).all()) and float(res[0][0][0]) > 0.0


def test_two_models_behind_the_autograd_bridge_agree_bit_for_bit(dev, det):
    """`loss = model(**batch)[0]; loss.backward()` three times on two models of the same weights: every .grad."""
    cfg, batch = _cfg_batch(dev)
    res = []
    for _ in range(2):
        m = _model(cfg, dev)
        out = []
        for _ in range(3):
            m.zero_grad()
            loss = m(**batch)[0]
            loss.backward()
            torch.cuda.synchronize()
            out.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}))
        res.append(out)
    for (la, ga), (lb, gb) in zip(*res):
        assert torch.equal(la, lb) and ga.keys() == gb.keys() and len(ga) > 20
        for n in ga:
            assert torch.equal(ga[n], gb[n]), n


def test_switch_turned_on_after_the_buffers_were_built(dev):
    """The engine reads the switch per step: buffers built in the default mode grow their dQ workspace to the planes."""
    from visitron_amd import ops
    from visitron_amd.training import PretrainEngine

    cfg, batch = _cfg_batch(dev)
    eng = PretrainEngine(_model(cfg, dev), lr=1e-3, schedule="constant", warmup_steps=0)
    eng.train_step(batch)
    nh = cfg.num_attention_heads
    assert eng._bufs[(2, 513)].ws_t["dq32"].numel() * 4 == ops.attention_bwd_ws_bytes(2, 513, nh) == 2 * 513 * nh * 64 * 4
    assert eng.state_dict()["hyper"]["deterministic"] is False
    ops.set_deterministic(True)
    try:
        loss = eng.train_step(batch)[0]
        torch.cuda.synchronize()
        assert eng._bufs[(2, 513)].ws_t["dq32"].numel() * 4 == 3 * 2 * 513 * nh * 64 * 4
        assert eng.state_dict()["hyper"]["deterministic"] is True and bool(torch.isfinite(loss))
    finally:
        ops.set_deterministic(False)
