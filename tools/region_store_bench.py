"""Measurements for the region store (visitron_amd/regions.py, csrc/regions.hip); needs an MI355X.

B = 256, T = 128, R = 100, D = 2054, a bf16 store of N = 2000 random viewpoints with 5 rows in every view (1.5 GB: the
gathers miss the 256 MB last-level cache).  Every round uses another of 8 prepared batches of random viewpoints.  The
variants of a part alternate in one process; medians and the 10 % / 90 % points are reported.

  (a) the packed gather kernel alone against dst.copy_(src), device to device, of exactly the bytes it writes; both between
      device events, each behind a fill of a 512 MB scratch buffer on the same stream (the host has both events and the
      launch queued before the device reaches them, and neither finds its source or destination in a cache)
  (b) store.pretrain_batch(packed=True) end to end (host packing, the copy, the kernel, a synchronise) against the path it
      replaces: per item np.concatenate of 36 [5, D] arrays (data_loader_pretrain.py:615-634), stack, pinned upload,
      data.assemble_batch, ops.pack_concat, a synchronise; microseconds per batch and samples/s of input
  (c) with --step: the B = 256 training step (bench.py's model and hyper-parameters) fed the packed batch against the same
      step fed img_feats / img_location_embeddings resident on the device -- the route the step had before it took
      img_packed, its code unchanged -- alternating, with both spreads

    python tools/region_store_bench.py [--step] [out file]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, V, P, D, B, T, R, POOL = 2000, 36, 5, 2054, 256, 128, 100, 8


def emit(fh, line):
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def stats(v):
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def main():
    import visitron_amd
    from visitron_amd import RegionStore, data, ops

    args = [a for a in sys.argv[1:] if a != "--step"]
    with_step = "--step" in sys.argv[1:]
    assert torch.cuda.is_available(), "needs a HIP device"
    fh = open(args[0], "a") if args else None
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    keys = ["scan_%05d" % i for i in range(N)]
    # every viewpoint holds the same random rows (a stride-0 view: the host stays small); the gather moves addresses, not values
    one = torch.rand(V, P, D, generator=g).numpy()
    feats = np.lib.stride_tricks.as_strided(one, shape=(N, V, P, D), strides=(0,) + one.strides)
    counts = np.full((N, V), P, dtype=np.uint8)
    store = RegionStore((keys, feats, counts), dev)
    kpad = ops.round_up(D + 128, 64)
    emit(fh, "region store bench: %s, store [%d, %d, %d, %d] bf16 = %.2f GB, B = %d, T = %d, R = %d, kpad = %d"
         % (torch.cuda.get_device_name(0), N, V, P, store.ld, store.nbytes / 1e9, B, T, R, kpad))
    ids = torch.randint(1000, 30000, (B, T), generator=g).to(dev)
    labels = torch.where(torch.rand(B, T, generator=g) < 0.15, ids.cpu(), torch.full((B, T), -1)).to(dev)
    att = torch.ones(B, T, dtype=torch.long, device=dev)
    tok = torch.where(torch.rand(B, T, generator=g) < 0.1, torch.randint(0, 1601, (B, T), generator=g), torch.full((B, T), -1)).to(dev)
    nxt = torch.randint(0, 36, (B,), generator=g).to(dev)
    pool = [(np.random.RandomState(i).randint(N, size=B), np.random.RandomState(100 + i).randint(V, size=B)) for i in range(POOL)]
    rows = [torch.from_numpy(np.stack(p, 1).astype(np.int32)).to(dev) for p in pool]

    # ---- (a) the kernel against a copy of the bytes it writes
    out = (torch.empty((B * R, kpad), dtype=torch.bfloat16, device=dev),) + tuple(
        torch.empty((B, T + R), dtype=torch.int64, device=dev) for _ in range(3))
    written = B * R * kpad * 2 + 3 * B * (T + R) * 8
    read = B * R * (D * 2 + 512) + 3 * B * T * 8 + B * (8 + V)
    src = torch.rand(written // 4, device=dev)
    dst = torch.empty_like(src)
    scratch = torch.empty(128 << 20, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    tk, tc = [], []
    for r in range(10 + 100):
        scratch.fill_(1.0)
        ev[0].record()
        ops.region_gather(store.features, store.counts, store.loc_table, rows[r % POOL], D, labels, att, tok, R, kpad=kpad, out=out)
        ev[1].record()
        torch.cuda.synchronize()
        a = ev[0].elapsed_time(ev[1]) * 1e-3
        scratch.fill_(2.0)
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        if r >= 10:
            tk.append(a)
            tc.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    (mk, lk, hk), (mc, lc, hc) = stats(tk), stats(tc)
    emit(fh, "(a) packed gather: %.2f MB written, %.2f MB read" % (written / 1e6, read / 1e6))
    emit(fh, "    kernel alone (device events)            %8.1f us  (10%% %.1f, 90%% %.1f)  %.0f GB/s read + written"
         % (mk * 1e6, lk * 1e6, hk * 1e6, (read + written) / mk / 1e9))
    emit(fh, "    dst.copy_(src) of the written bytes     %8.1f us  (10%% %.1f, 90%% %.1f)" % (mc * 1e6, lc * 1e6, hc * 1e6))
    emit(fh, "    kernel / copy = %.2f (the expectation to report against: at most 1.25)" % (mk / mc))

    # ---- (b) end to end against the path it replaces
    host_rows = [[one[v] for v in range(V)] for _ in range(4)]      # the 36 [5, D] records of an item, as the reader hands them
    pinned = torch.empty((B, V * P, D), dtype=torch.float32).pin_memory()
    view_ids = torch.arange(V).repeat_interleave(P)[None, :].expand(B, V * P).contiguous().to(dev)
    region_counts = torch.full((B,), V * P, dtype=torch.long, device=dev)

    def replaced(cur):
        items = [np.concatenate(host_rows[b % 4], axis=0) for b in range(B)]
        pinned.copy_(torch.from_numpy(np.stack(items)))
        img = pinned.to(dev, non_blocking=True)
        bt = data.assemble_batch(ids, labels, att, img, region_counts, view_ids, torch.from_numpy(cur).to(dev), nxt, R,
                                 token_classes=tok)
        return ops.pack_concat(bt["img_feats"].view(B * R, D), bt["img_location_embeddings"].view(B * R, 128), kpad)

    want = replaced(pool[0][1])
    got = store.pretrain_batch(np.zeros(B, dtype=np.int64), pool[0][1], ids, labels, att, nxt, R, token_classes=tok, packed=True)
    assert torch.equal(got["img_packed"].view(torch.int16), want.view(torch.int16)), "the two paths disagree"
    ts, tr = [], []
    for r in range(3 + 20):
        slots, cur = pool[r % POOL]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store.pretrain_batch(slots, cur, ids, labels, att, nxt, R, token_classes=tok, packed=True)
        torch.cuda.synchronize()
        a = time.perf_counter() - t0
        t0 = time.perf_counter()
        replaced(cur)
        torch.cuda.synchronize()
        if r >= 3:
            ts.append(a)
            tr.append(time.perf_counter() - t0)
    (ms, ls, hs), (mr, lr, hr_) = stats(ts), stats(tr)
    emit(fh, "(b) one batch of input, end to end with a synchronise")
    emit(fh, "    store.pretrain_batch(packed=True)        %9.1f us  (10%% %.1f, 90%% %.1f)  %.0f samples/s"
         % (ms * 1e6, ls * 1e6, hs * 1e6, B / ms))
    emit(fh, "    concatenate + upload + assemble + pack   %9.1f us  (10%% %.1f, 90%% %.1f)  %.0f samples/s"
         % (mr * 1e6, lr * 1e6, hr_ * 1e6, B / mr))

    # ---- (c) the training step
    if with_step:
        from visitron_amd.config import BertConfig
        from visitron_amd.modeling import PreTrainOscar
        from visitron_amd.training import PretrainEngine

        cfg = BertConfig(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
        torch.manual_seed(0)
        eng = PretrainEngine(PreTrainOscar(cfg).to(dev).train(), lr=5e-5, weight_decay=0.05, eps=1e-8, schedule="linear",
                             warmup_steps=0, t_total=20000)
        slots, cur = pool[0]
        bp = store.pretrain_batch(slots, cur, ids, labels, att, nxt, R, token_classes=tok, packed=True)
        bu = store.pretrain_batch(slots, cur, ids, labels, att, nxt, R, token_classes=tok, packed=False)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        tp, tu = [], []
        for r in range(10 + 40):
            for batch, acc in (((bp, tp), (bu, tu)) if r % 2 == 0 else ((bu, tu), (bp, tp))):   # neither always goes first
                e[0].record()
                eng.train_step(batch)
                e[1].record()
                torch.cuda.synchronize()
                if r >= 10:
                    acc.append(e[0].elapsed_time(e[1]) * 1e-3)
        (mp, lp, hp), (mu, lu, hu) = stats(tp), stats(tu)
        emit(fh, "(c) B = %d training step, alternating, 40 timed steps each" % B)
        emit(fh, "    fed img_packed                           %9.2f ms  (10%% %.2f, 90%% %.2f)  %.0f samples/s"
             % (mp * 1e3, lp * 1e3, hp * 1e3, B / mp))
        emit(fh, "    fed img_feats + location (resident fp32)  %9.2f ms  (10%% %.2f, 90%% %.2f)  %.0f samples/s"
             % (mu * 1e3, lu * 1e3, hu * 1e3, B / mu))
    visitron_amd.check_errors()
    if fh is not None:
        fh.close()


if __name__ == "__main__":
    main()
