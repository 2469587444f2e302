"""GPU: visitron_amd.optim -- the multi-tensor Adam / AdamW step, the gradient norm and the clip -- against the rules
evaluated in float64 from the same fp32 inputs, and inside the reference's two loops.

Bounds of a single step (u = 2^-24; one rounding per fp32 operation and per fp32-rounded constant, about 2 x headroom):
with gg = g * coef, Mmag = |b1 m| + |(1 - b1) gg|, den the fp64 denominator and Dmag = step_size * Mmag / den,
    |m - m64| <= 4 u Mmag,   |v - v64| <= 5 u v64,   |p - p64| <= u (2 |p64| + 2 |p_old| + 16 Dmag).
Every comparison records measured / bound through helpers.check_close (bound 1)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import check_close, maxabs, model_pair

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (g, m, v, p) magnitudes
SCALES = [(1e-3, 1e-3, 1e-6, 0.03), (1.0, 0.1, 1e-2, 1.0), (1e-6, 1e-7, 1e-14, 0.02), (30.0, 3.0, 50.0, 0.5),
          (0.0, 1e-3, 1e-6, 0.03)]
GROUPS = {
    "adamw": [dict(lr=1e-3, weight_decay=0.05, eps=1e-6), dict(lr=3e-4, weight_decay=0.0, eps=1e-8)],
    "adam": [dict(lr=1e-3, eps=1e-8), dict(lr=3e-4, eps=1e-6, betas=(0.8, 0.99))],
}


def _counts():
    from visitron_amd.optim import CHUNK as C

    return [1, 3, 4, 5, 255, 256, 257, 4095, 4097, C - 1, C, C + 1, 2 * C + 3]


def _put(host, dev, misaligned=False):
    """host -> device; misaligned: a view that starts 4 bytes into its buffer (4-byte aligned only)."""
    if not misaligned:
        return host.to(dev)
    buf = torch.empty(host.numel() + 1, device=dev)
    view = buf[1:]
    view.copy_(host)
    assert view.data_ptr() % 16 == 4
    return view


class World(object):
    """A parameter list in two groups with gradients, preset moments and step counts, and one parameter without gradient."""

    def __init__(self, dev, rule, t0=0, scale=SCALES[0], seed=0, counts=None, preset=True, **opt_kw):
        from visitron_amd import optim

        C = optim.CHUNK

        gs, ms, vs, ps = scale
        gen = torch.Generator().manual_seed(seed)
        self.rule, self.dev, self.cfg = rule, dev, GROUPS[rule]
        self.params, self.group_of = [], []
        moments = []
        for i, n in enumerate(counts or _counts()):
            p = nn.Parameter(_put(torch.randn(n, generator=gen) * ps, dev, misaligned=n in (257, C + 1)))
            p.grad = _put(torch.randn(n, generator=gen) * gs, dev, misaligned=n in (4097, C + 1))
            m = _put(torch.randn(n, generator=gen) * ms, dev, misaligned=n == 5)
            v = _put(torch.randn(n, generator=gen).abs() * vs, dev)
            self.params.append(p)
            self.group_of.append(i % 2)
            moments.append((m, v))
        self.skipped = nn.Parameter((torch.randn(100, generator=gen) * ps).to(dev))      # grad stays None
        groups = [dict(params=[p for p, k in zip(self.params, self.group_of) if k == j], **self.cfg[j]) for j in (0, 1)]
        groups[0]["params"].append(self.skipped)
        cls = optim.AdamW if rule == "adamw" else optim.Adam
        self.opt = cls(groups, **opt_kw)
        if preset:
            step = (lambda: t0) if rule == "adamw" else (lambda: torch.tensor(float(t0)))
            for p, (m, v) in zip(self.params, moments):
                self.opt.state[p] = dict(step=step(), exp_avg=m, exp_avg_sq=v)
            self.opt.state[self.skipped] = dict(step=step(), exp_avg=torch.full_like(self.skipped, 0.25),
                                                exp_avg_sq=torch.full_like(self.skipped, 0.5))

    def snapshot(self):
        torch.cuda.synchronize()
        out = []
        for p in self.params + [self.skipped]:
            st = self.opt.state[p]
            zero = torch.zeros(p.numel())
            out.append(dict(p=p.detach().cpu().clone(), g=None if p.grad is None else p.grad.cpu().clone(),
                            m=st["exp_avg"].cpu().clone() if st else zero, v=st["exp_avg_sq"].cpu().clone() if st else zero,
                            step=int(st["step"]) if st else 0))
        return out

    def set_grads(self, seed, scale):
        gen = torch.Generator().manual_seed(seed)
        for p in self.params:
            p.grad.copy_(torch.randn(p.numel(), generator=gen) * scale)


def rule64(rule, cfg, lr, t, p, g, m, v, coef=1.0):
    """One step of the rule in float64 from fp32 inputs -> (p64, m64, v64) and the three element-wise bounds."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    b1, b2 = cfg.get("betas", (0.9, 0.999))
    eps, wd = cfg["eps"], cfg.get("weight_decay", 0.0)
    gg = g * coef
    m64 = b1 * m + (1.0 - b1) * gg
    v64 = b2 * v + (1.0 - b2) * gg * gg
    if rule == "adamw":
        step_size = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        den = v64.sqrt() + eps
    else:
        step_size = lr / (1.0 - b1 ** t)
        den = v64.sqrt() / math.sqrt(1.0 - b2 ** t) + eps
    p64 = p - step_size * m64 / den
    if wd > 0.0:
        p64 = p64 - lr * wd * p64
    mmag = (b1 * m).abs() + ((1.0 - b1) * gg).abs()
    dmag = step_size * mmag / den
    return (p64, m64, v64), (U * (2 * p64.abs() + 2 * p.abs() + 16 * dmag), 4 * U * mmag, 5 * U * v64)


def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err),
                                                                           torch.full_like(err, float("inf"))))
    return float(r.max())


def check_step(tag, world, before, after, lrs=None, coef=1.0):
    """after == rule64(before) within the bounds for every parameter with a gradient; the other one bitwise untouched."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, (b, a) in enumerate(zip(before[:-1], after[:-1])):
        cfg = world.cfg[world.group_of[i]]
        lr = cfg["lr"] if lrs is None else lrs[world.group_of[i]]
        t = b["step"] + 1
        assert a["step"] == t, (tag, i)
        want, bounds = rule64(world.rule, cfg, lr, t, b["p"], b["g"], b["m"], b["v"], coef)
        for key, w, bd in zip(("p", "m", "v"), want, bounds):
            worst[key] = max(worst[key], _ratio(a[key], w, bd))
    for key in ("m", "v", "p"):
        check_close("%s: %s error / bound" % (tag, key), worst[key], 0.0, 1.0)
    b, a = before[-1], after[-1]
    assert a["step"] == b["step"] and all(torch.equal(a[k], b[k]) for k in ("p", "m", "v")), tag + ": skipped parameter"


@pytest.mark.parametrize("t0", [0, 5, 999])
@pytest.mark.parametrize("rule", ["adamw", "adam"])
def test_single_step_matches_the_rule_in_fp64(dev, rule, t0):
    for k, scale in enumerate(SCALES):
        world = World(dev, rule, t0, scale, seed=10 * t0 + k)
        before = world.snapshot()
        world.opt.step()
        after = world.snapshot()
        check_step("optim %s t0=%d scales %s" % (rule, t0, scale), world, before, after)
        for b, a in zip(before, after):                  # a plain step leaves the gradients alone
            assert b["g"] is None or torch.equal(b["g"], a["g"])
        assert world.skipped.grad is None and world.opt._table.builds == 1


def test_three_steps_under_the_warmup_schedule(dev):
    from oracle import optim as ooptim
    from visitron_amd.optim import WarmupLinearSchedule

    world = World(dev, "adamw", preset=False, seed=77)
    sched = WarmupLinearSchedule(world.opt, warmup_steps=2, t_total=10)
    start = world.snapshot()
    o_params = [nn.Parameter(s["p"].clone()) for s in start[:-1]]
    o_opt = ooptim.AdamW([dict(params=[p for p, k in zip(o_params, world.group_of) if k == j], **world.cfg[j])
                          for j in (0, 1)])
    o_sched = ooptim.WarmupLinearSchedule(o_opt, warmup_steps=2, t_total=10)
    for step in range(3):
        world.set_grads(seed=100 + step, scale=1e-2)
        before = world.snapshot()
        lrs = [g["lr"] for g in world.opt.param_groups]
        assert lrs == [g["lr"] for g in o_opt.param_groups]
        for p, s in zip(o_params, before):
            p.grad = s["g"].clone()
        world.opt.step()
        sched.step()
        o_opt.step()
        o_sched.step()
        check_step("optim schedule step %d" % step, world, before, world.snapshot(), lrs=lrs)
    assert world.opt._table.builds == 1      # gradients rewritten in place: same addresses, same table
    assert lrs[0] == pytest.approx(1e-3) and len(world.opt.state[world.skipped]) == 0
    for i, (p, w) in enumerate(zip(world.params, o_params)):
        delta = float((w.detach() - start[i]["p"]).abs().max())
        assert maxabs(p, w) < 1e-6 + 1e-4 * delta, i


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


@pytest.mark.parametrize("where", ["below", "above"])
def test_clip_grad_norm(dev, where):
    from visitron_amd.optim import clip_grad_norm_

    world = World(dev, "adamw", scale=SCALES[1], seed=5)
    params = world.params + [world.skipped]
    before = [p.grad.cpu().clone() for p in world.params]
    norm64 = _norm64(before)
    max_norm = norm64 * (0.37 if where == "below" else 1.5)
    total = clip_grad_norm_(params, max_norm)
    assert total.dim() == 0 and total.is_cuda and total.dtype == torch.float32
    torch.cuda.synchronize()
    # <= 32-element fp32 chains + an 8-level tree would give 41 u on the sum, half after the root, plus one rounding
    check_close("optim clip total_norm rel (%s)" % where, abs(float(total) - norm64) / norm64, 0.0, 2.0 ** -19)
    coef = np.float32(max_norm) / (np.float32(float(total)) + np.float32(1e-6))
    coef = min(np.float32(1.0), coef)
    assert (coef == 1.0) == (where == "above")
    for p, g in zip(world.params, before):
        want = g if coef == 1.0 else torch.from_numpy(g.numpy() * coef)
        assert torch.equal(p.grad.cpu(), want), p.numel()
    assert world.skipped.grad is None
    # two runs on equal inputs are bitwise equal
    again = World(dev, "adamw", scale=SCALES[1], seed=5)
    total2 = clip_grad_norm_(again.params + [again.skipped], max_norm)
    assert torch.equal(total2, total)
    for p, q in zip(world.params, again.params):
        assert torch.equal(p.grad, q.grad)


def test_clip_grad_norm_with_nothing_to_clip(dev):
    from visitron_amd.optim import clip_grad_norm_

    assert float(clip_grad_norm_([], 1.0)) == 0.0
    none = [nn.Parameter(torch.ones(7, device=dev)), nn.Parameter(torch.ones(3, device=dev))]
    total = clip_grad_norm_(none, 1.0)
    assert float(total) == 0.0 and total.device == none[0].device
    one = nn.Parameter(torch.ones(5, device=dev))
    one.grad = torch.full((5,), 2.0, device=dev)
    assert float(clip_grad_norm_(one, 100.0)) == pytest.approx(math.sqrt(20.0), rel=1e-6)      # a single tensor is a list of one


@pytest.mark.parametrize("rule", ["adamw", "adam"])
def test_fused_max_grad_norm_equals_clip_then_step(dev, rule):
    from visitron_amd.optim import clip_grad_norm_

    for frac in (0.25, 3.0):
        plain = World(dev, rule, 5, SCALES[1], seed=9)
        grads = [p.grad.cpu().clone() for p in plain.params]
        c = _norm64(grads) * frac
        fused = World(dev, rule, 5, SCALES[1], seed=9, max_grad_norm=c)
        before = fused.snapshot()
        total = clip_grad_norm_(plain.params + [plain.skipped], c)
        plain.opt.step()
        fused.opt.step()
        a, b = plain.snapshot(), fused.snapshot()
        for x, y, g in zip(a[:-1], b[:-1], grads):
            assert all(torch.equal(x[k], y[k]) for k in ("p", "m", "v")) and x["step"] == y["step"] == 6
            assert torch.equal(y["g"], g)                       # the fused step leaves p.grad unscaled
            assert torch.equal(x["g"], g) == (frac > 1.0)       # the clip call scaled them (below the norm)
        assert torch.equal(fused.opt.last_grad_norm, total)
        coef = min(1.0, float(np.float32(c) / (np.float32(float(total)) + np.float32(1e-6))))
        check_step("optim %s fused clip x%.2f" % (rule, frac), fused, before, b, coef=coef)


def _launches(fn):
    from visitron_amd import ops

    ops.profile_begin()
    fn()
    return {k: v["n"] for k, v in ops.profile_end().items()}


def test_launch_count_does_not_depend_on_the_list(dev):
    from visitron_amd import optim

    seen = []
    for n_tensors in (3, 300):
        def params():
            out = [nn.Parameter(torch.randn(1000, device=dev)) for _ in range(n_tensors)]
            for p in out:
                p.grad = torch.randn(1000, device=dev)
            return out

        ps = params()
        plain, fused = optim.AdamW(ps, lr=1e-3), optim.Adam(params(), lr=1e-3, max_grad_norm=1.0)
        counts = []
        for _ in range(2):       # the first call builds the table, the second reuses it
            counts.append((_launches(plain.step), _launches(fused.step), _launches(lambda: optim.clip_grad_norm_(ps, 1.0))))
        assert counts[0] == counts[1]
        seen.append(counts[0])
        assert plain._table.builds == fused._table.builds == 1
    assert seen[0] == seen[1]
    step, fused, clip = seen[0]
    assert step == {"multi_adam": 1}
    assert fused == {"multi_sumsq": 1, "norm_finish": 1, "multi_adam": 1}
    assert clip == {"multi_sumsq": 1, "norm_finish": 1, "multi_scale": 1}


@pytest.mark.parametrize("rule", ["adamw", "adam"])
def test_address_changes_rebuild_the_table(dev, rule):
    world = World(dev, rule, 5, SCALES[0], seed=21)
    opt = world.opt

    def step(tag):
        before = world.snapshot()
        opt.step()
        check_step("optim %s %s" % (rule, tag), world, before, world.snapshot())

    step("first step")
    assert opt._table.builds == 1
    old = [p.grad for p in world.params]                       # kept alive: the fresh ones cannot land on their addresses
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in world.params)
    gen = torch.Generator().manual_seed(4)
    for p in world.params:
        p.grad = (torch.randn(p.numel(), generator=gen) * 1e-3).to(dev)
    assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(world.params, old))
    step("after fresh gradients")
    assert opt._table.builds == 2
    step("same addresses again")
    assert opt._table.builds == 2
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))       # the moments move
    step("after load_state_dict")
    assert opt._table.builds == 3
    world.params[2].grad = None                                # the set of present gradients changes
    before = world.snapshot()
    opt.step()
    after = world.snapshot()
    assert opt._table.builds == 4
    assert after[2]["step"] == before[2]["step"] and all(torch.equal(after[2][k], before[2][k]) for k in ("p", "m", "v"))
    assert after[3]["step"] == before[3]["step"] + 1 and not torch.equal(after[3]["p"], before[3]["p"])


def test_torch_adam_state_loads_and_the_third_step_matches(dev):
    from visitron_amd import optim

    gen = torch.Generator().manual_seed(8)
    sizes = [1, 5, 257, 4097, optim.CHUNK + 1]
    init = [torch.randn(n, generator=gen) * 0.5 for n in sizes]
    grads = [[torch.randn(n, generator=gen) * 0.1 for n in sizes] for _ in range(3)]
    t_params = [nn.Parameter(w.clone()) for w in init]
    t_opt = torch.optim.Adam(t_params, lr=1e-3)
    for k in range(2):
        for p, g in zip(t_params, grads[k]):
            p.grad = g.clone()
        t_opt.step()
    ours_p = [nn.Parameter(p.detach().to(dev)) for p in t_params]
    ours = optim.Adam(ours_p, lr=1e-3)
    ours.load_state_dict(copy.deepcopy(t_opt.state_dict()))
    before = [dict(p=p.detach().clone(), m=t_opt.state[p]["exp_avg"].clone(), v=t_opt.state[p]["exp_avg_sq"].clone())
              for p in t_params]
    for p, q, g in zip(t_params, ours_p, grads[2]):
        p.grad = g.clone()
        q.grad = g.to(dev)
    t_opt.step()
    ours.step()
    torch.cuda.synchronize()
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    cfg = dict(lr=1e-3, eps=1e-8)
    for p, q, b, g in zip(t_params, ours_p, before, grads[2]):
        assert optim._step_value(ours.state[q]["step"]) == 3 == int(t_opt.state[p]["step"])
        _, bounds = rule64("adam", cfg, 1e-3, 3, b["p"], g, b["m"], b["v"])
        got = (q.detach().cpu(), ours.state[q]["exp_avg"].cpu(), ours.state[q]["exp_avg_sq"].cpu())
        want = (p.detach(), t_opt.state[p]["exp_avg"], t_opt.state[p]["exp_avg_sq"])
        for key, x, w, bd in zip(("p", "m", "v"), got, want, bounds):
            worst[key] = max(worst[key], _ratio(x, w.double(), bd))
    for key in ("m", "v", "p"):
        check_close("optim adam third step vs torch.optim.Adam: %s error / bound" % key, worst[key], 0.0, 1.0)


def test_refused_tensors(dev):
    from visitron_amd import optim

    def one(t, g=None):
        p = nn.Parameter(t)
        p.grad = torch.ones_like(t) if g is None else g
        return p

    with pytest.raises(RuntimeError, match="fp32"):
        optim.AdamW([one(torch.ones(8, device=dev, dtype=torch.float64))]).step()
    with pytest.raises(RuntimeError, match="contiguous"):
        optim.AdamW([one(torch.ones(8, 4, device=dev).t())]).step()
    with pytest.raises(RuntimeError, match="HIP device only"):
        optim.Adam([one(torch.ones(8, device=dev)), one(torch.ones(8))]).step()
    sparse = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (8,)).to(dev)
    with pytest.raises(RuntimeError, match="sparse"):
        optim.AdamW([one(torch.ones(8, device=dev), sparse)]).step()
    with pytest.raises(RuntimeError, match="sparse"):
        optim.clip_grad_norm_([one(torch.ones(8, device=dev), sparse)], 1.0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="one device per list"):
            optim.AdamW([one(torch.ones(8, device=dev)), one(torch.ones(8, device="cuda:1"))]).step()
    p = one(torch.ones(8, device=dev))
    with pytest.raises(RuntimeError):
        optim.AdamW([p, one(torch.ones(8, device=dev, dtype=torch.float64))]).step()
    torch.cuda.synchronize()
    assert float(p.detach().min()) == 1.0        # a refused step has written nothing


def test_pretrain_loop_with_the_hip_adamw(dev):
    """The body of test_reference_style_loop_with_torch_optimizer (pretrain.py:150-193) with visitron_amd.optim.AdamW on
    the product side, built BEFORE the first forward (the bridge re-points p.data into its slab at that forward)."""
    from oracle.modeling import PreTrainOscar as OModel
    from oracle.optim import AdamW as OAdamW, grouped_parameters
    from test_gpu_train import GRAD_TOL, _rel
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.optim import AdamW
    from visitron_amd.synth import make_batch

    cfg = mini_config()
    ref, prod = model_pair(OModel, PreTrainOscar, cfg, seed=12, device=dev)
    prod.train()
    ref.train()
    o_ref = OAdamW(grouped_parameters(ref, 0.05), lr=1e-3, eps=1e-8)
    o_prod = AdamW(grouped_parameters(prod, 0.05), lr=1e-3, eps=1e-8)
    b = make_batch(cfg, 4, text_len=16, region_len=8, seed=2)
    bd = {k: v.to(dev) for k, v in b.items()}
    before_last = None
    for it in range(4):
        ref.zero_grad(); o_ref.zero_grad()
        lr_ = ref(**b)[0]
        lr_.backward()
        o_ref.step()
        prod.zero_grad(); o_prod.zero_grad()
        out = prod(**bd)
        assert len(out) == 7 and out[0].requires_grad
        loss = out[0]
        loss /= 1.0  # the reference divides in place before backward (pretrain.py:170)
        loss.backward()
        if it == 0:
            wg = dict(ref.named_parameters())
            for n, p in prod.named_parameters():
                assert p.grad is not None, n
                assert _rel(p.grad, wg[n].grad) < GRAD_TOL, n
        if it == 3:
            prod.eval()
            with torch.no_grad():
                before_last = [t.clone() for t in prod(**bd)[:4]]
            prod.train()
        o_prod.step()
        assert abs(float(loss) - float(lr_)) < 0.15
    # eval / no_grad takes the inference path, whose packed bf16 copies must have followed the last step
    prod.eval()
    with torch.no_grad():
        out = prod(**bd)
    assert not out[0].requires_grad
    assert float(out[0]) != float(before_last[0])


def test_agent_loop_with_the_hip_adam_and_clip(dev):
    """The body of test_rollout_training_runs_with_dropout_and_adam (agent.py:497-518) with visitron_amd.optim.Adam and
    visitron_amd.optim.clip_grad_norm_ at 40.0."""
    from test_gpu_rollout_train import _rollout_pair
    from visitron_amd.optim import Adam, clip_grad_norm_

    cfg, _, p_enc, _, p_dec = _rollout_pair(dev, False, dropout=0.3)
    p_enc.train()
    p_dec.train()
    opt_e = Adam(p_enc.parameters(), lr=1e-3)
    opt_d = Adam(p_dec.parameters(), lr=1e-3)
    B, S, C = 4, 16, 5
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, cfg.vocab_size, (B, S), generator=g).to(dev)
    lens = [16, 12, 12, 7]
    pad = torch.zeros(B, S, dtype=torch.bool)
    for i, n in enumerate(lens):
        pad[i, n:] = True
    pad = pad.to(dev)
    action = torch.randn(B, 4, generator=g).to(dev)
    feature = (torch.randn(B, 36, 132, generator=g).abs() * 0.3).to(dev)
    cand = (torch.randn(B, C, 132, generator=g).abs() * 0.3).to(dev)
    target = torch.randint(0, C, (B,), generator=g).to(dev)

    def loss_of():
        ctx, h_t, c_t = p_enc(ids, lens, pad)
        _, _, logit, _ = p_dec(action, feature, cand, h_t, h_t, c_t, ctx, pad[:, : ctx.shape[1]])
        return nn.functional.cross_entropy(logit, target)

    losses = []
    for _ in range(8):
        opt_e.zero_grad()
        opt_d.zero_grad()
        loss = loss_of()
        loss.backward()
        clip_grad_norm_(p_enc.parameters(), 40.0)
        clip_grad_norm_(p_dec.parameters(), 40.0)
        opt_e.step()
        opt_d.step()
        losses.append(float(loss))
    assert all(math.isfinite(l) for l in losses) and min(losses[-3:]) < losses[0], losses
    p_enc.eval()
    p_dec.eval()
    with torch.no_grad():
        e1 = float(loss_of())
    p_enc.train()
    p_dec.train()
    for _ in range(3):
        opt_e.zero_grad()
        opt_d.zero_grad()
        loss_of().backward()
        opt_e.step()
        opt_d.step()
    p_enc.eval()
    p_dec.eval()
    with torch.no_grad():
        e2 = float(loss_of())
    assert e2 != e1                     # the eval path's packed weights follow the optimizer
