"""Measurements for the decoder widths that are no multiple of 4 (feature width 2058 = 2054 + 4, the reference's default);
needs an MI355X.

    python tools/decoder_widths_bench.py [--parent-lib libvisitron_hip.so of the parent commit] [--rounds 3] [out file]

Every round starts one fresh child process on this build and, with --parent-lib, one on the parent's library (VT_HIP_LIB: the
same Python tree, the other kernels), alternating, so that the two are compared inside one session on one machine and the
spread of the parent's own repeated runs is known.  A child measures, each as the median of 5 windows after warm-ups:

  * one inference decoder step (hidden 512, 36 views, 9 candidates, instruction length 80) issued directly and replayed
    from its HIP graph, B = 8 and B = 64, feature widths 2052 and 2058: host clock around 100 steps ending in a synchronise
  * vt_softdot_attention_f32 alone at [64, 36, 2052] and [64, 36, 2058]: device events around 200 launches
  * the feature store at D = 2054 (8-byte pieces here, element by element in the parent), B = 16 and B = 64, 8 candidates, a
    store of 1024 viewpoints (303 MB): store.get_input_feat (host clock, ends in a synchronise) and the gather kernel alone
    (device events, behind a fill of a 512 MB buffer so that it finds nothing in a cache)

The parent's library refuses 2058: those entries are absent from its children.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = 5


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _host_us(fn, steps, warm):
    import torch

    for _ in range(warm):
        fn()
    out = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e6)
    return _median(out)


def _event_us(fn, launches, warm):
    import torch

    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / launches * 1e3)
    return _median(out)


def child():
    import math

    import numpy as np
    import torch

    from visitron_amd import FeatureStore, observations, ops
    from visitron_amd.rollout import AttnDecoderLSTM

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    res = {}
    g = torch.Generator().manual_seed(0)
    hs, L, C = 512, 80, 9
    for feat in (2052, 2058):
        torch.manual_seed(1)
        dec = AttnDecoderLSTM(4, 64, hs, 0.5, feature_size=feat).eval().to(dev)
        for B in (8, 64):
            args = [torch.randn(B, 4, generator=g), torch.randn(B, 36, feat, generator=g).abs() * 0.3,
                    torch.randn(B, C, feat, generator=g).abs() * 0.3, None, torch.randn(B, hs, generator=g) * 0.3,
                    torch.randn(B, hs, generator=g) * 0.3, torch.randn(B, L, hs, generator=g) * 0.5,
                    torch.zeros(B, L, dtype=torch.bool)]
            args = [a if a is None else a.to(dev) for a in args]
            for graph in (False, True):
                dec.use_graph = graph
                try:
                    with torch.no_grad():
                        res["step_%s_B%d_%d" % ("graph" if graph else "direct", B, feat)] = _host_us(lambda: dec(*args), 100, 20)
                except RuntimeError:      # a library that refuses the width
                    pass
    for D in (2052, 2058):
        t, c = torch.randn(64, D, generator=g).to(dev), torch.randn(64, 36, D, generator=g).to(dev)
        try:
            res["softdot_64x36x%d" % D] = _event_us(lambda: ops.softdot_attention(t, c, None, True, True, True), 200, 20)
        except RuntimeError:
            pass
    N, V, D, CANDS = 1024, 36, 2054, 8
    keys = ["scan_%05d" % i for i in range(N)]
    store = FeatureStore((keys, torch.rand(N, V, D, generator=g)), dev, view_angle_table=observations.default_view_angle_table())
    scratch = torch.empty(128 << 20, device=dev)
    rng = np.random.RandomState(0)
    for B in (16, 64):
        pool = []
        for _ in range(8):
            obs = []
            for _ in range(B):
                scan, vp = keys[int(rng.randint(N))].split("_")
                cands = [{"pointId": int(rng.randint(V)), "heading": float(rng.uniform(-3, 7)), "elevation": float(rng.uniform(-0.6, 0.6))}
                         for _ in range(CANDS)]
                obs.append({"scan": scan, "viewpoint": vp, "viewIndex": int(rng.randint(V)), "heading": float(rng.uniform(0, 6.28)),
                            "elevation": float(rng.uniform(-0.5, 0.5)), "candidate": cands})
            pool.append(obs)
        Cmax = CANDS + 1
        records = []
        for obs in pool:
            buf = np.zeros(ops.obs_record_bytes(B, Cmax)[0], dtype=np.uint8)
            observations.pack_record(buf, *store.obs_fields(obs))
            records.append(torch.from_numpy(buf).to(dev))
        out = (torch.empty((B, 4), device=dev), torch.empty((B, V, D + 4), device=dev), torch.empty((B, Cmax, D + 4), device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, Cmax), dtype=torch.bool, device=dev))
        turn = [0]

        def host_path():
            turn[0] += 1
            store.get_input_feat(pool[turn[0] % len(pool)])
            torch.cuda.synchronize()

        res["store_get_input_feat_B%d_%d" % (B, D)] = _host_us(host_path, 50, 10)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for r in range(10 + 60):
            scratch.fill_(float(r))
            ev[0].record()
            ops.obs_gather(store.features, store.view_angle_table, records[r % len(records)], B, Cmax, out=out)
            ev[1].record()
            torch.cuda.synchronize()
            if r >= 10:
                ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
        res["store_gather_kernel_B%d_%d" % (B, D)] = _median(ts)
        assert math.isfinite(float(out[1].sum()))
    import visitron_amd

    visitron_amd.check_errors()
    print("RESULT " + json.dumps(res), flush=True)


def emit(fh, line):
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    if a.child:
        return child()
    fh = open(a.out, "a") if a.out else None
    runs = {"this": [], "parent": []}
    for _ in range(a.rounds):
        for who in ("this", "parent"):
            if who == "parent" and not a.parent_lib:
                continue
            env = dict(os.environ)
            env.pop("VT_HIP_LIB", None)
            if who == "parent":
                env["VT_HIP_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE,
                               universal_newlines=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("the %s child ended with status %d" % (who, p.returncode))
            runs[who].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    emit(fh, "decoder widths bench: %d fresh processes per build, alternating; per process the median of %d windows; us"
         % (a.rounds, WINDOWS))
    names = list(runs["this"][0])
    med = {}
    for n in names:
        line = "  %-34s this %s" % (n, " ".join("%8.1f" % r[n] for r in runs["this"]))
        med[n] = _median([r[n] for r in runs["this"]])
        pv = [r[n] for r in runs["parent"] if n in r]
        if pv:
            line += "   parent %s   this / parent (medians) %.3f, parent's own spread %.3f" % (
                " ".join("%8.1f" % v for v in pv), med[n] / _median(pv), max(pv) / min(pv))
        emit(fh, line)
    for n in names:
        if n.endswith("_2058") or n.endswith("x2058"):
            base = n[:-4] + "2052"
            emit(fh, "  %-34s 2058 / 2052 = %.3f" % (n, med[n] / med[base]))
    if fh is not None:
        fh.close()


if __name__ == "__main__":
    main()
