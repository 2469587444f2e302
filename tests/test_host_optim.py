"""CPU: the host side of visitron_amd.optim -- schedules, the per-step constants of both rules, the chunk-table builder and
its cache, the refusals, and the state_dict layout (no kernel runs here)."""
import copy
import math
import os
import re

import pytest
import torch

from visitron_amd import optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the element counts of the GPU tests' tensor list (tests/test_gpu_optim.py)
C = optim.CHUNK
COUNTS = [1, 3, 4, 5, 255, 256, 257, 4095, 4097, C - 1, C, C + 1, 2 * C + 3]


def test_table_geometry_is_the_header_s():
    src = open(os.path.join(ROOT, "include", "visitron_hip.h")).read()
    defs = dict(re.findall(r"#define (VT_OPTIM_\w+) (\d+)", src))
    assert int(defs["VT_OPTIM_CHUNK"]) == optim.CHUNK
    assert int(defs["VT_OPTIM_ENTRY_WORDS"]) == optim.ENTRY_WORDS
    assert int(defs["VT_OPTIM_HYPER_FLOATS"]) == optim.HYPER_FLOATS


def _opt(cls=optim.AdamW, **kw):
    return cls([torch.nn.Parameter(torch.zeros(3))], lr=1.0, **kw)


def test_schedules_agree_with_the_oracle_lambdas():
    from oracle.optim import warmup_constant_lambda, warmup_linear_lambda

    for warmup, total in ((0, 10), (2, 10), (3, 3), (5, 40)):
        lin = optim.WarmupLinearSchedule(_opt(), warmup_steps=warmup, t_total=total)
        con = optim.WarmupConstantSchedule(_opt(), warmup_steps=warmup)
        f_lin, f_con = warmup_linear_lambda(warmup, total), warmup_constant_lambda(warmup)
        for step in range(total + 3):
            assert lin.lr_lambda(step) == f_lin(step), (warmup, total, step)
            assert con.lr_lambda(step) == f_con(step), (warmup, step)


def test_schedule_drives_group_lr_like_the_oracle_class():
    from oracle import optim as ooptim

    ours, theirs = _opt(), ooptim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=1.0)
    s_ours = optim.WarmupLinearSchedule(ours, warmup_steps=2, t_total=10)
    s_theirs = ooptim.WarmupLinearSchedule(theirs, warmup_steps=2, t_total=10)
    assert isinstance(s_ours, torch.optim.lr_scheduler.LambdaLR)
    for _ in range(12):
        assert ours.param_groups[0]["lr"] == theirs.param_groups[0]["lr"]
        ours.step()      # nothing has a gradient: no launch, the schedule's call counter still moves
        theirs.step()
        s_ours.step()
        s_theirs.step()


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_host_constants_of_both_rules(t):
    lr, b1, b2, eps, wd = 3e-4, 0.9, 0.999, 1e-6, 0.05
    got = optim.adamw_constants(lr, (b1, b2), eps, wd, t)
    want = (b1, 1.0 - b1, b2, 1.0 - b2, lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t), 1.0, eps, lr * wd)
    assert len(got) == optim.HYPER_FLOATS and all(isinstance(x, float) for x in got)
    assert got == pytest.approx(want, rel=1e-15, abs=0.0)
    assert optim.adamw_constants(lr, (b1, b2), eps, wd, t, correct_bias=False)[4] == lr
    got = optim.adam_constants(lr, (b1, b2), 1e-8, t)
    want = (b1, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t), 1e-8, 0.0)
    assert got == pytest.approx(want, rel=1e-15, abs=0.0)
    # 1 - b2 is formed in double: its fp32 rounding is NOT 1.0f - 0.999f (1.3e-5 off)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    assert abs(f32(got[3]) - 0.001) < 0.001 * 2.0 ** -24
    assert abs((1.0 - f32(0.999)) - 0.001) > 0.001 * 1e-5


def _entries(base=1 << 20):
    """Fake addresses: tensor i has p, g, m, v in four disjoint 'arenas'; tensor 3 starts 4 bytes off (a view)."""
    out, off = [], 0
    for i, n in enumerate(COUNTS):
        shift = 4 if i == 3 else 0
        out.append(tuple(arena * (1 << 40) + base + off + shift for arena in range(1, 5)) + (n, i % 2))
        off += 4 * n + 64
    return out


def test_chunk_table_covers_every_element_once():
    entries = _entries()
    rows = optim.build_chunk_table(entries)
    assert all(len(r) == optim.ENTRY_WORDS for r in rows)
    assert len(rows) == sum((n + C - 1) // C for n in COUNTS)
    for col in range(4):
        covered = {}
        for r in rows:
            assert 1 <= r[4] <= C
            assert r[col] % 4 == 0
            for tensor, e in enumerate(entries):
                if e[col] <= r[col] < e[col] + 4 * e[4]:
                    assert (r[col] - e[col]) % (4 * C) == 0          # cut at multiples of the chunk: alignment is kept
                    assert r[col] + 4 * r[4] <= e[col] + 4 * e[4]    # never past the tensor's end
                    assert r[5] == e[5]                              # the tensor's hyper slot
                    assert (r[0] - e[0]) == (r[col] - e[col])        # the four addresses move together
                    covered.setdefault(tensor, []).append(((r[col] - e[col]) // 4, r[4]))
                    break
            else:
                raise AssertionError("a chunk outside every tensor: %r" % (r,))
        for tensor, e in enumerate(entries):
            pos = 0
            for lo, n in sorted(covered[tensor]):
                assert lo == pos
                pos += n
            assert pos == e[4]


def test_chunk_table_keeps_null_addresses_and_skips_empty_tensors():
    rows = optim.build_chunk_table([(0, 4096, 0, 0, C + 2, 0), (0, 1 << 30, 0, 0, 0, 0)])
    assert rows == [[0, 4096, 0, 0, C, 0], [0, 4096 + 4 * C, 0, 0, 2, 0]]


def test_chunk_table_is_rebuilt_only_on_a_change():
    entries = _entries()
    table = optim.ChunkTable()
    assert table.update(entries) and table.builds == 1
    rows = table.rows
    for _ in range(3):
        assert not table.update(list(entries)) and table.builds == 1 and table.rows is rows
    moved = list(entries)
    moved[5] = moved[5][:1] + (moved[5][1] + 256,) + moved[5][2:]      # one gradient at a new address
    assert table.update(moved) and table.builds == 2
    assert not table.update(moved)
    assert table.update(moved[:-1]) and table.builds == 3              # one gradient is None now
    assert table.update(moved) and table.builds == 4                   # and back
    reslot = [e[:5] + (0,) for e in moved]
    assert table.update(reslot) and table.builds == 5
    assert table.n_chunks == len(optim.build_chunk_table(reslot)) and table.numel == sum(COUNTS)


def test_optimizer_slots_follow_group_and_step(monkeypatch):
    """step() hands the builder one slot per (group, step count); the table is reused while addresses stay."""
    seen = []
    monkeypatch.setattr(optim, "_check", lambda *a: None)

    class Stop(Exception):
        pass

    def update(self, entries):
        seen.append(list(entries))
        raise Stop()            # no device here: end the step where the launch would follow

    monkeypatch.setattr(optim.ChunkTable, "update", update)
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 7))
    opt = optim.AdamW([{"params": [a, b], "weight_decay": 0.1}, {"params": [c], "lr": 0.5}], lr=1e-3)
    for p in (a, c):
        p.grad = torch.ones_like(p)
    opt.state[c].update(step=4, exp_avg=torch.zeros(7), exp_avg_sq=torch.zeros(7))
    with pytest.raises(Stop):
        opt.step()
    (entries,) = seen
    assert [(e[4], e[5]) for e in entries] == [(3, 0), (7, 1)]      # b has no gradient; group 1 is another slot
    assert entries[0][0] == a.data_ptr() and entries[0][1] == a.grad.data_ptr()
    assert entries[1][2] == opt.state[c]["exp_avg"].data_ptr()
    assert opt.state[a]["step"] == 0 and opt.state[c]["step"] == 4 and len(opt.state[b]) == 0   # nothing advanced


def test_refusals():
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="weight_decay"):
        optim.Adam(p, weight_decay=0.01)
    with pytest.raises(ValueError, match="amsgrad"):
        optim.Adam(p, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        optim.Adam(p, maximize=True)
    with pytest.raises(ValueError, match="serves lr, betas and eps"):
        optim.Adam(p, amsgrad=True)
    with pytest.raises(ValueError, match="norm_type"):
        optim.clip_grad_norm_(p, 1.0, norm_type=1)
    with pytest.raises(ValueError, match="norm_type"):
        optim.clip_grad_norm_(p, 1.0, norm_type=float("inf"))
    p[0].grad = torch.ones(4)
    for opt in (optim.AdamW(p), optim.Adam(p)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            opt.step()
        assert float(p[0].detach().abs().max()) == 0.0 and int(opt.state[p[0]]["step"]) == 0
    with pytest.raises(RuntimeError, match="HIP device only"):
        optim.clip_grad_norm_(p, 1.0)
    assert torch.equal(p[0].grad, torch.ones(4))
    # nothing to do is not an error, on any device
    assert float(optim.clip_grad_norm_([], 1.0)) == 0.0
    assert float(optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0


def test_closure_is_honoured_and_gradless_parameters_are_skipped():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = optim.AdamW([p])
    calls = []

    def closure():
        calls.append(torch.is_grad_enabled())
        return torch.tensor(2.5)

    assert float(opt.step(closure)) == 2.5 and calls == [True]
    assert len(opt.state[p]) == 0        # grad is None: no state, no step


def _grouped(model):
    from oracle.optim import grouped_parameters

    return grouped_parameters(model, 0.05)


def test_state_dict_layout_equals_the_oracle_class():
    from oracle.optim import AdamW as OAdamW

    def model():
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.LayerNorm(3), torch.nn.Linear(3, 2))
        m[1].register_parameter("unused", torch.nn.Parameter(torch.zeros(2)))
        return m

    m_o, m_p = model(), model()
    o = OAdamW(_grouped(m_o), lr=1e-3, eps=1e-8)
    ours = optim.AdamW(_grouped(m_p), lr=1e-3, eps=1e-8)
    for p in m_o.parameters():
        p.grad = torch.ones_like(p)
    m_o[1].unused.grad = None
    o.step()
    want = o.state_dict()
    # our state after one step, written by hand (the kernel does not run here): same names, same types
    for group in ours.param_groups:
        for p in group["params"]:
            if p is not m_p[1].unused:
                ours.state[p].update(step=1, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    got = ours.state_dict()
    assert [sorted(g) for g in got["param_groups"]] == [sorted(g) for g in want["param_groups"]]
    for g, w in zip(got["param_groups"], want["param_groups"]):
        assert g == w
    assert sorted(got["state"]) == sorted(want["state"])
    for k in want["state"]:
        assert sorted(got["state"][k]) == sorted(want["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        assert type(got["state"][k]["step"]) is type(want["state"][k]["step"]) is int
        assert got["state"][k]["exp_avg"].shape == want["state"][k]["exp_avg"].shape
    # and each loads into the other
    ours.load_state_dict(want)
    o.load_state_dict(got)
    assert ours.state[m_p[0].weight]["step"] == 1
    assert torch.equal(ours.state[m_p[0].weight]["exp_avg"], want["state"][0]["exp_avg"])
    assert float(o.state[m_o[0].weight]["exp_avg"].abs().max()) == 0.0


def test_adam_state_dict_interchanges_with_torch_adam():
    w_t, w_p = torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(5))
    t_opt, ours = torch.optim.Adam([w_t], lr=1e-3), optim.Adam([w_p], lr=1e-3)
    w_t.grad = torch.full((5,), 0.5)
    t_opt.step()
    t_opt.step()
    ours.load_state_dict(copy.deepcopy(t_opt.state_dict()))     # (torch hands out its `step` tensors themselves)
    st = ours.state[w_p]
    assert optim._step_value(st["step"]) == 2 and torch.equal(st["exp_avg"], t_opt.state[w_t]["exp_avg"])
    assert ours._constants(ours.param_groups[0], 3) == optim.adam_constants(1e-3, (0.9, 0.999), 1e-8, 3)
    back = torch.optim.Adam([torch.nn.Parameter(torch.ones(5))], lr=1e-3)
    back.load_state_dict(ours.state_dict())
    back.param_groups[0]["params"][0].grad = torch.full((5,), 0.5)
    back.step()          # torch accepts what we hand back and takes its third step from it
    assert float(back.state[back.param_groups[0]["params"][0]]["step"]) == 3.0
    # a fresh state of ours has torch's layout too
    fresh = optim.Adam([w_p])
    assert isinstance(fresh._new_step(), torch.Tensor) and fresh._new_step().dtype == torch.float32
