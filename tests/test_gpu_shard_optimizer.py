"""GPU: AdamW sharded over data-parallel ranks -- the two table-driven kernels (vt_shard_adamw, vt_shard_settle) in one
process, bit for bit against ops.adamw_flat / torch's conversions; the whole mode under 2 and 4 ranks sharing this device
(tests/dp_shard_worker.py, gloo), bit for bit against the replicated engine; the refusals; and, where two devices exist,
the same worker over nccl."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
HYPER = dict(lr=1e-3, step_size=7.3e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)
# slab layout of the kernel test: (segment start, elements, decay) -- 8, 24 and 1 032 elements, decay on and off in one
# table, gaps between the segments (sentinels), and one segment of 5 Mi elements: 2 560 chunks of ops.SHARD_CHUNK, more than
# the 2 048 workgroups of the capped grid, so workgroups stride to a second chunk
SEGMENTS = [(64, 8, True), (128, 24, False), (192, 1032, True), (1280, 24, True), (2048, 5 * 1024 * 1024, False), (2048 + 5 * 1024 * 1024 + 64, 8, False)]
TOTAL = 2048 + 5 * 1024 * 1024 + 128


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


@pytest.fixture(scope="module")
def slabs(dev):
    """Seeded p, g (fp32 and its bf16 copy), m, v over the whole slab, made once and never written."""
    g_ = torch.Generator().manual_seed(1234)
    p = (torch.randn(TOTAL, generator=g_) * 0.05).to(dev)
    g = (torch.randn(TOTAL, generator=g_) * 1e-2).to(dev)
    m = (torch.randn(TOTAL, generator=g_) * 1e-3).to(dev)
    v = (torch.rand(TOTAL, generator=g_) * 1e-5).to(dev)
    return dict(p=p, g=g, g16=g.to(BF16), m=m, v=v)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("g_bf16", [False, True], ids=["g32", "g16"])
def test_shard_adamw_matches_adamw_flat_bitwise(dev, slabs, g_bf16, grad_scale):
    from visitron_amd import ops

    assert (5 * 1024 * 1024) // ops.SHARD_CHUNK > 2048
    g = slabs["g16"] if g_bf16 else slabs["g"]
    # the yardstick: adamw_flat per segment on copies of the slabs (moments at the slab offsets)
    want = {k: slabs[k].clone() for k in ("p", "m", "v")}
    want["mirror"] = torch.full((TOTAL,), -7.0, dtype=BF16, device=dev)
    for s, n, dec in SEGMENTS:
        sl = slice(s, s + n)
        ops.adamw_flat(want["p"][sl], g[sl], want["m"][sl], want["v"][sl], want["mirror"][sl], HYPER["lr"], HYPER["step_size"],
                       HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["wd"] if dec else 0.0, grad_scale)
    # the sharded kernel: moments in a shard-local storage, back to back in REVERSE segment order behind 8 sentinels
    p, mirror = slabs["p"].clone(), torch.full((TOTAL,), -7.0, dtype=BF16, device=dev)
    owned = sum(n for _, n, _ in SEGMENTS)
    m_sh = torch.full((owned + 16,), 3.0, device=dev)
    v_sh = torch.full((owned + 16,), 3.0, device=dev)
    segs, mo = [], 8
    for s, n, dec in reversed(SEGMENTS):
        segs.append((s, s + n, dec, mo))
        m_sh[mo:mo + n] = slabs["m"][s:s + n]
        v_sh[mo:mo + n] = slabs["v"][s:s + n]
        assert mo != s
        mo += n
    g_before = g.clone()
    table = ops.shard_adamw_table(p, g, m_sh, v_sh, mirror, segs)
    assert table.n_chunks == sum(-(-n // ops.SHARD_CHUNK) for _, n, _ in SEGMENTS) and table.numel == owned
    ops.shard_adamw(table, g_bf16, HYPER["lr"], HYPER["step_size"], HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["wd"], grad_scale)
    torch.cuda.synchronize()
    assert same(p, want["p"]) and same(mirror, want["mirror"])     # inside the segments updated alike, outside untouched alike
    assert same(g, g_before)
    touched = torch.zeros(TOTAL, dtype=torch.bool, device=dev)
    for s, e, dec, mo in segs:
        assert same(m_sh[mo:mo + e - s], want["m"][s:e]) and same(v_sh[mo:mo + e - s], want["v"][s:e]), (s, e)
        touched[s:e] = True
        assert not same(p[s:e], slabs["p"][s:e])                    # ... and the update did happen
    assert same(p[~touched], slabs["p"][~touched]) and bool((mirror[~touched] == -7.0).all())
    assert bool((m_sh[:8] == 3.0).all() and (m_sh[-8:] == 3.0).all() and (v_sh[:8] == 3.0).all() and (v_sh[-8:] == 3.0).all())
    # weight decay did act where the flag says so: the decay-free update of a decay segment differs
    s, n, _ = SEGMENTS[2]
    nodecay = {k: slabs[k][s:s + n].clone() for k in ("p", "m", "v")}
    ops.adamw_flat(nodecay["p"], g[s:s + n], nodecay["m"], nodecay["v"], None, HYPER["lr"], HYPER["step_size"], HYPER["b1"],
                   HYPER["b2"], HYPER["eps"], 0.0, grad_scale)
    assert not same(nodecay["p"], p[s:s + n])


def _special_values(dev):
    tiny = 2.0 ** -140                                            # fp32 subnormal
    base = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, tiny, -tiny, 2.0 ** -133, 1.0, -1.0,
                         1.00390625, 1.01171875, 3.3895314e38, -3.3895314e38, 1e-40, 65504.0], device=dev)
    g_ = torch.Generator().manual_seed(5)
    return torch.cat([base, torch.randn(4096 - 16, generator=g_).to(dev) * 3.0])


def test_shard_settle_both_directions(dev):
    from visitron_amd import ops

    n = 4096
    src32 = _special_values(dev)
    src16 = src32.to(BF16)
    src16[5], src16[6] = torch.tensor(2.0 ** -130, dtype=BF16), torch.tensor(-(2.0 ** -130), dtype=BF16)   # bf16 subnormals
    # slab of 3 n: [0, n) direction 0 (p = float(mirror)), [n, 2 n) untouched, [2 n + 8, 3 n) direction 1 (mirror = bf16(p))
    p = torch.full((3 * n,), 9.0, device=dev)
    mirror = torch.full((3 * n,), -9.0, dtype=BF16, device=dev)
    mirror[:n] = src16
    p[2 * n:] = src32
    p0, mirror0 = p.clone(), mirror.clone()
    table = ops.shard_settle_table(p, mirror, [(0, n, 0), (2 * n + 8, 3 * n, 1)], chunk=1024)
    assert table.n_chunks == 4 + 4
    ops.shard_settle(table)
    torch.cuda.synchronize()
    want_p, want_m = src16.float(), src32.to(BF16)
    nan_p, nan_m = torch.isnan(want_p), torch.isnan(want_m)
    assert bool(nan_p[0]) and bool(nan_m[0]) and int(nan_p.sum()) == 1
    assert bool(torch.equal(torch.isnan(p[:n]), nan_p)) and same(p[:n][~nan_p], want_p[~nan_p])
    got_m = mirror[2 * n + 8:]
    assert bool(torch.equal(torch.isnan(got_m), nan_m[8:])) and same(got_m[~nan_m[8:]], want_m[8:][~nan_m[8:]])
    assert bool(torch.isnan(mirror[2 * n:2 * n + 8]).sum() == 0) and same(mirror[n:2 * n + 8], mirror0[n:2 * n + 8])   # outside: untouched
    assert same(mirror[:n], mirror0[:n]) and same(p[n:][~torch.isnan(p0[n:])], p0[n:][~torch.isnan(p0[n:])])
    # the signs of the zeros and the subnormals came through both ways
    assert bits(p[:n])[4].item() == -2 ** 31 and float(p[5]) == 2.0 ** -130 and float(p[6]) == -(2.0 ** -130)
    assert bits(mirror)[2 * n + 8 + 0].item() == bits(want_m)[8].item()


def test_misaligned_addresses_are_refused_and_nothing_is_launched(dev):
    from visitron_amd import _lib, ops

    lib = _lib.load()
    n = 64
    p, g, m, v = (torch.full((n + 8,), float(i + 1), device=dev) for i in range(4))
    g16 = torch.full((n + 8,), 2.0, dtype=BF16, device=dev)
    mirror = torch.full((n + 8,), 5.0, dtype=BF16, device=dev)
    stream = ops._stream()

    def adamw(tab, g_is_bf16):
        return lib.vt_shard_adamw(ops._ptr(tab.dev), ops._ptr(tab.host), tab.n_chunks, int(g_is_bf16), 1e-3, 1e-3, 0.9, 0.999,
                                  1e-8, 0.05, 1.0, stream)

    good = ops.shard_adamw_table(p, g, m, v, mirror, [(0, 32, True, 0), (32, 64, False, 32)])
    cases = [
        (ops.shard_adamw_table(p[1:], g, m, v, mirror, [(0, 32, True, 0), (32, 64, False, 32)]), False),        # p 4 bytes off
        (ops.shard_adamw_table(p, g[2:], m, v, mirror, [(0, 32, True, 0)]), False),                             # fp32 g 8 bytes off
        (ops.shard_adamw_table(p, g16[1:], m, v, mirror, [(0, 32, True, 0)]), True),                            # bf16 g 2 bytes off
        (ops.shard_adamw_table(p, g, m, v, mirror, [(0, 32, True, 0), (32, 64, True, 34)]), False),             # moments 8 bytes off
        (ops.shard_adamw_table(p, g, m, v, mirror[2:], [(0, 32, True, 0)]), False),                             # mirror 4 bytes off
    ]
    for tab, is16 in cases:
        assert adamw(tab, is16) == _lib.VT_ERR_BAD_ALIGN
    assert adamw(ops.shard_adamw_table(p, g16[4:], m, v, mirror, [(0, 32, True, 0)]), False) == _lib.VT_ERR_BAD_ALIGN   # 8 bytes: bf16 only
    with pytest.raises(RuntimeError, match="code -2"):
        ops.shard_adamw(cases[0][0], False, 1e-3, 1e-3, 0.9, 0.999, 1e-8, 0.05)
    bad_settle = ops.shard_settle_table(p[2:], mirror, [(0, 32, 0)])
    assert lib.vt_shard_settle(ops._ptr(bad_settle.dev), ops._ptr(bad_settle.host), bad_settle.n_chunks, stream) == _lib.VT_ERR_BAD_ALIGN
    bad_settle = ops.shard_settle_table(p, mirror[1:], [(0, 32, 1)])
    assert lib.vt_shard_settle(ops._ptr(bad_settle.dev), ops._ptr(bad_settle.host), bad_settle.n_chunks, stream) == _lib.VT_ERR_BAD_ALIGN
    odd = ops.shard_settle_table(p, mirror, [(0, 30, 1)])           # a count that is no multiple of 4
    assert lib.vt_shard_settle(ops._ptr(odd.dev), ops._ptr(odd.host), odd.n_chunks, stream) == _lib.VT_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    for t, val in ((p, 1.0), (g, 2.0), (m, 3.0), (v, 4.0), (mirror, 5.0)):
        assert bool((t == val).all())                               # nothing ran
    assert adamw(good, False) == _lib.VT_OK
    torch.cuda.synchronize()
    assert bool((p[:64] != 1.0).all()) and bool((p[64:] == 1.0).all())


# ---- the mode under several ranks ------------------------------------------------------------------------------------------
def _run_worker(nproc, backend, port, timeout):
    script = os.path.join(ROOT, "tests", "dp_shard_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % nproc, "--master-addr", "127.0.0.1",
           "--master-port", str(port), script, backend]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)   # a failure, abort or time-out fails the test
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    for rank in range(nproc):
        assert "rank %d ok" % rank in r.stdout


@pytest.mark.parametrize("world,port", [(2, 29681), (4, 29683)])
def test_sharded_engine_matches_the_replicated_engine_bitwise(dev, world, port):
    """tests/dp_shard_worker.py, every rank on this device, gloo: the scenarios (i) - (vii) marked in the worker."""
    _run_worker(world, "gloo", port, 600)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices: the real reduce_scatter_tensor / all_gather_into_tensor")
def test_sharded_engine_over_nccl_on_two_devices(dev):
    """The same worker with backend nccl, rank r on device r: the in-place reduce_scatter_tensor and all_gather_into_tensor
    run.  Two ranks add commutatively, so the bits of the replicated engine are still expected."""
    _run_worker(2, "nccl", 29685, 600)


def test_one_rank_and_fp32_precision_keep_their_behaviour(dev):
    from visitron_amd import ops
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PreTrainOscar
    from visitron_amd.synth import deterministic_state_dict, make_batch
    from visitron_amd.training import PretrainEngine

    cfg = mini_config()
    batch = {k: v.to(dev) for k, v in make_batch(cfg, 3, text_len=20, region_len=10, seed=9).items()}
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        engines = []
        for shard in (False, True):
            m = PreTrainOscar(cfg)
            m.load_state_dict(deterministic_state_dict(m, seed=5))
            m.tie_weights()
            e = PretrainEngine(m.to(dev).eval(), lr=1e-3, schedule="constant", shard_optimizer=shard)
            assert e.world == 1 and e.shard is False and e.plan is None and e.flat.m is not None
            outs = [torch.stack([torch.as_tensor(x, dtype=torch.float32, device=dev) for x in e.train_step(batch)]) for _ in range(2)]
            engines.append((e, outs))
            e.consolidate()                                       # nothing to do on one rank
            e.all_reduce_grads()
        (a, oa), (b, ob) = engines
        assert all(same(x, y) for x, y in zip(oa, ob))
        assert same(a.flat.p, b.flat.p) and same(a.flat.m, b.flat.m) and same(a.flat.v, b.flat.v) and same(a.flat.mirror, b.flat.mirror)
        assert b.state_dict()["hyper"]["shard_optimizer"] is True and a.state_dict()["hyper"]["shard_optimizer"] is False
    finally:
        ops.set_deterministic(was)
    # precision="fp32": one rank trains as before, with or without the flag
    m = PreTrainOscar(cfg)
    m.load_state_dict(deterministic_state_dict(m, seed=5))
    m.tie_weights()
    e = PretrainEngine(m.to(dev).eval(), lr=1e-3, schedule="constant", precision="fp32", shard_optimizer=True)
    assert e.precision == "fp32" and e.shard is False
    out = e.train_step(batch)
    assert bool(torch.isfinite(out[0]))
