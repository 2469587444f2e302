"""Measurements for the observation gather (visitron_amd/observations.py, csrc/observations.hip); needs an MI355X.

One panoramic step's input tensors at B = 16 and B = 64, 8 candidates per agent, D = 2048, 36 views, a store of 1024
viewpoints (302 MB: larger than the 256 MB last-level cache).  Four variants alternate in one process, 20 warm-ups and then
200 timed rounds each; the median is reported:

  (a) the reference's host path: the numpy fills of Agent._feature_variable / _candidate_variable / get_input_feat restated
      (agent.py:186-228) over observations that already carry their "feature" arrays, plus .to(device) and a synchronise
  (b) store.get_input_feat(obs): host packing, the one copy, the kernel, and a synchronise
  (c) the gather kernel alone, between device events (the record already on the device)
  (d) the yardstick: dst.copy_(src), device to device, of exactly the bytes the gather writes, between device events
      (c) and (d) each run behind a fill of a 512 MB scratch buffer on the same stream: the host has both events and the
      launch queued before the device reaches them (no enqueue time between the events), and neither finds its source or
      its destination in a cache

and (c)'s achieved GB/s, counting the bytes it reads (live image rows, table rows, the record) plus the bytes it writes.
Every round uses another of 16 prepared batches of random viewpoints, so no variant re-reads what the previous round left in
a cache.  What builds the observation dicts (the loader's _get_obs) is outside every variant.

    python tools/observations_bench.py [out file]
"""
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, D, CANDS, POOL, WARM, ROUNDS = 1024, 36, 2048, 8, 16, 20, 200


def emit(fh, line):
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def make_obs(host_store, table, keys, B, rng):
    obs = []
    for _ in range(B):
        slot, view = int(rng.randint(N)), int(rng.randint(V))
        scan, vp = keys[slot].split("_")
        cands = []
        for j in range(CANDS):
            p, h, e = int(rng.randint(V)), float(rng.uniform(-3, 7)), float(rng.uniform(-0.6, 0.6))
            ang = np.array([math.sin(h), math.cos(h), math.sin(e), math.cos(e)], dtype=np.float32)
            cands.append({"pointId": p, "heading": h, "elevation": e, "feature": np.concatenate((host_store[slot, p], ang), -1)})
        obs.append({"scan": scan, "viewpoint": vp, "viewIndex": view, "heading": float(rng.uniform(0, 6.28)),
                    "elevation": float(rng.uniform(-0.5, 0.5)), "candidate": cands,
                    "feature": np.concatenate((host_store[slot], table[view]), -1)})
    return obs


def reference_host_path(obs, dev):
    """agent.py:186-228 restated: the three numpy fills and the three uploads."""
    a = np.zeros((len(obs), 4), np.float32)
    for i, ob in enumerate(obs):
        a[i] = [math.sin(ob["heading"]), math.cos(ob["heading"]), math.sin(ob["elevation"]), math.cos(ob["elevation"])]
    input_a_t = torch.from_numpy(a).to(dev)
    features = np.empty((len(obs), V, D + 4), dtype=np.float32)
    for i, ob in enumerate(obs):
        features[i, :, :] = ob["feature"]
    f_t = torch.from_numpy(features).to(dev)
    leng = [len(ob["candidate"]) + 1 for ob in obs]
    cand = np.zeros((len(obs), max(leng), D + 4), dtype=np.float32)
    for i, ob in enumerate(obs):
        for j, c in enumerate(ob["candidate"]):
            cand[i, j, :] = c["feature"]
    return input_a_t, f_t, torch.from_numpy(cand).to(dev), leng


def main():
    from visitron_amd import FeatureStore, observations, ops

    assert torch.cuda.is_available(), "needs a HIP device"
    fh = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    host_store = rng.rand(N, V, D).astype(np.float32)
    keys = ["scan_%05d" % i for i in range(N)]
    table = observations.default_view_angle_table()
    store = FeatureStore((keys, host_store), dev, view_angle_table=table)
    emit(fh, "observations bench: %s, store [%d, %d, %d] fp32 = %.0f MB, %d candidates, %d warm-ups + %d rounds, median"
         % (torch.cuda.get_device_name(0), N, V, D, store.nbytes / 1e6, CANDS, WARM, ROUNDS))
    for B in (16, 64):
        pool = [make_obs(host_store, table, keys, B, rng) for _ in range(POOL)]
        Cmax = CANDS + 1
        records = []
        for obs in pool:
            nbytes = ops.obs_record_bytes(B, Cmax)[0]
            buf = np.zeros(nbytes, dtype=np.uint8)
            observations.pack_record(buf, *store.obs_fields(obs))
            records.append(torch.from_numpy(buf).to(dev))
        out = (torch.empty((B, 4), device=dev), torch.empty((B, V, D + 4), device=dev), torch.empty((B, Cmax, D + 4), device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, Cmax), dtype=torch.bool, device=dev))
        written = 4 * (B * 4 + B * V * (D + 4) + B * Cmax * (D + 4)) + 4 * B + B * Cmax
        read = 4 * B * (V + CANDS) * D + 16 * B * V + nbytes
        src = torch.rand(written // 4, device=dev)
        dst = torch.empty_like(src)
        # the variants agree before anything is timed
        want = reference_host_path(pool[0], dev)
        got = store.get_input_feat(pool[0])
        assert torch.equal(got[1], want[1]) and torch.equal(got[2][..., :D], want[2][..., :D]) and got[3] == want[3]
        assert float((got[2] - want[2]).abs().max()) < 1e-6 and float((got[0] - want[0]).abs().max()) < 1e-6
        scratch = torch.empty(128 << 20, device=dev)                  # 512 MB of fp32
        times = {k: [] for k in "abcd"}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for r in range(WARM + ROUNDS):
            obs, rec = pool[r % POOL], records[r % POOL]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reference_host_path(obs, dev)
            torch.cuda.synchronize()
            ta = time.perf_counter() - t0
            t0 = time.perf_counter()
            store.get_input_feat(obs)
            torch.cuda.synchronize()
            tb = time.perf_counter() - t0
            scratch.fill_(1.0)
            ev[0].record()
            ops.obs_gather(store.features, store.view_angle_table, rec, B, Cmax, out=out)
            ev[1].record()
            torch.cuda.synchronize()
            tc = ev[0].elapsed_time(ev[1]) * 1e-3
            scratch.fill_(2.0)
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            td = ev[0].elapsed_time(ev[1]) * 1e-3
            if r >= WARM:
                for k, t in zip("abcd", (ta, tb, tc, td)):
                    times[k].append(t)
        med = {k: float(np.median(v)) for k, v in times.items()}
        lo = {k: float(np.percentile(v, 10)) for k, v in times.items()}
        hi = {k: float(np.percentile(v, 90)) for k, v in times.items()}
        emit(fh, "B = %d: the step's tensors are %.2f MB (written), %.2f MB read by the gather" % (B, written / 1e6, read / 1e6))
        for k, name in (("a", "(a) reference host path: numpy fills + .to(device) + sync"),
                        ("b", "(b) store.get_input_feat: pack + copy + kernel + sync"),
                        ("c", "(c) gather kernel alone (device events)"),
                        ("d", "(d) dst.copy_(src) of the written bytes (device events)")):
            emit(fh, "  %-62s %9.1f us  (10%% %.1f, 90%% %.1f)" % (name, med[k] * 1e6, lo[k] * 1e6, hi[k] * 1e6))
        emit(fh, "  (c) moves %.1f GB/s (read + written); (c) / (d) = %.2f; (a) / (b) = %.1f"
             % ((read + written) / med["c"] / 1e9, med["c"] / med["d"], med["a"] / med["b"]))
    import visitron_amd

    visitron_amd.check_errors()
    if fh is not None:
        fh.close()


if __name__ == "__main__":
    main()
