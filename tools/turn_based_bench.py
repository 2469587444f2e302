"""Measurements for the turn-based decoder step (visitron_amd/turn_based.py); needs an MI355X.

  --epsilon   the error of the fast sigmoid / tanh of the LSTM kernels: vt_lstm_step_train_f32 with zero recurrent weights (the
              gates then equal xproj) against float64 over [-20, 20] -> the EPS_MEASURED of tests/helpers_turn_based.py
  (default)   one inference step at B = 8 and B = 64 (hidden 512, embedding 64, feature 2054, L = 80):
                * visitron_amd.turn_based.AttnDecoderLSTM
                * a plain-torch module of the same arithmetic (fp32 nn.Embedding / nn.LSTMCell / bmm / softmax) on the same GPU
                * the fused cell launch alone against the launches it replaces (this library's gather / pack / GEMM /
                  vt_lstm_step_f32 chain, and torch's embedding + cat + LSTMCell)
                * the [-inf writes, CrossEntropyLoss, softmax, Categorical.sample] chain of agent.py:316-338 in torch against
                  turn_based.action_feedback
              Both sides are warmed up, then timed in alternating windows that end in a device synchronise; the median
              window per side is reported.

Appends its lines to the file given with --out (default: stdout only).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(fh, line):
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def measure_epsilon(fh):
    from visitron_amd import ops

    dev = torch.device("cuda:0")
    hs, B = 128, 64
    n = B * hs
    # 4 * n points per gate: a uniform grid over [-20, 20] and a dense one over [-1, 1] (where 1 - e cancels in tanh)
    worst = {"sigmoid": 0.0, "tanh": 0.0}
    w_hh = torch.zeros((4 * hs, hs), dtype=torch.bfloat16, device=dev)
    for lo, hi in ((-20.0, 20.0), (-1.0, 1.0), (-0.01, 0.01)):
        for rep in range(8):
            g = torch.Generator().manual_seed(rep)
            z = (torch.rand(B, 4 * hs, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()
            h0 = torch.zeros((B, hs), dtype=torch.float32, device=dev)
            c0 = torch.zeros((B, hs), dtype=torch.float32, device=dev)
            _, _, (gates, _, _) = ops.lstm_step_train(z.to(dev).contiguous(), h0, c0, w_hh)
            got = gates.cpu().double()
            z64 = z.double()
            ref = torch.cat((torch.sigmoid(z64[:, :2 * hs]), torch.tanh(z64[:, 2 * hs:3 * hs]), torch.sigmoid(z64[:, 3 * hs:])), 1)
            err = (got - ref).abs()
            worst["tanh"] = max(worst["tanh"], float(err[:, 2 * hs:3 * hs].max()))
            worst["sigmoid"] = max(worst["sigmoid"], float(torch.cat((err[:, :2 * hs], err[:, 3 * hs:]), 1).max()))
    emit(fh, "epsilon: fast sigmoid max |err| = %.4e, fast tanh max |err| = %.4e over [-20, 20] (%d points per range)"
         % (worst["sigmoid"], worst["tanh"], 8 * n * 4))
    emit(fh, "epsilon: EPS_MEASURED = %.4e" % max(worst.values()))


class TorchDecoder(nn.Module):
    """The same arithmetic in plain torch (fp32)."""

    def __init__(self, a_in, a_out, E, hs, F):
        super().__init__()
        self.embedding = nn.Embedding(a_in, E)
        self.lstm = nn.LSTMCell(E + F, hs)
        self.linear_in = nn.Linear(hs, hs, bias=False)
        self.linear_out = nn.Linear(2 * hs, hs, bias=False)
        self.decoder2action = nn.Linear(hs, a_out)

    def forward(self, action, feature, h_0, c_0, ctx, ctx_mask):
        x = torch.cat((self.embedding(action.reshape(-1)), feature), 1)
        h_1, c_1 = self.lstm(x, (h_0, c_0))
        attn = torch.bmm(ctx, self.linear_in(h_1).unsqueeze(2)).squeeze(2)
        attn = torch.softmax(attn.masked_fill(ctx_mask.bool(), -float("inf")), 1)
        weighted = torch.bmm(attn.unsqueeze(1), ctx).squeeze(1)
        h_tilde = torch.tanh(self.linear_out(torch.cat((weighted, h_1), 1)))
        return h_1, c_1, attn, self.decoder2action(h_tilde)


def alternate(fns, iters, windows):
    """Median seconds per call of each fn over `windows` alternating windows of `iters` calls."""
    times = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters)
    return [float(np.median(t)) for t in times], [float(np.min(t)) for t in times], [float(np.max(t)) for t in times]


def bench(fh, iters, windows):
    from visitron_amd import turn_based as tb

    dev = torch.device("cuda:0")
    a_in, a_out, E, hs, F, L = 8, 6, 64, 512, 2054, 80
    torch.manual_seed(0)
    ours = tb.AttnDecoderLSTM(a_in, a_out, E, hs, 0.5, feature_size=F).to(dev).eval()
    plain = TorchDecoder(a_in, a_out, E, hs, F).to(dev).eval()
    for B in (8, 64):
        action = torch.randint(0, a_in, (B, 1), device=dev)
        feature = torch.rand(B, F, device=dev)
        h0, c0 = torch.randn(B, hs, device=dev) * 0.1, torch.randn(B, hs, device=dev) * 0.1
        ctx = torch.randn(B, L, hs, device=dev) * 0.1
        lens = torch.randint(L // 2, L + 1, (B,))
        mask = (torch.arange(L)[None, :] >= lens[:, None]).to(torch.uint8).to(dev)
        target = torch.randint(0, a_out, (B,), device=dev)
        rows = [r for r in range(B) if r % 3 == 0]                  # the rows that cannot move forward
        blocked_host = torch.zeros(B, a_out, dtype=torch.bool)
        blocked_host[rows, 1] = True
        crit = nn.CrossEntropyLoss(ignore_index=-100)

        def f_ours():
            with torch.no_grad():
                return ours(action, feature, h0, c0, ctx, mask)

        def f_plain():
            with torch.no_grad():
                return plain(action, feature, h0, c0, ctx, mask)

        logit = f_plain()[3].clone()

        def head_torch():
            lg = logit.clone()
            for r in rows:                                           # one device write per row, as agent.py:316-318
                lg[r, 1] = -float("inf")
            loss = crit(lg, target)
            a_t = torch.distributions.Categorical(torch.softmax(lg, 1)).sample()
            return loss, a_t

        def head_ours():
            return tb.action_feedback(logit, target, blocked_host.to(dev, non_blocking=True), feedback="sample")

        for fn in (f_ours, f_plain, head_torch, head_ours):         # warm-up: code objects, packed weights, allocator
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        (m_o, m_p), (lo_o, lo_p), (hi_o, hi_p) = alternate((f_ours, f_plain), iters, windows)
        emit(fh, "step  B=%-3d hs=%d F=%d L=%d: turn_based %.1f us (%.1f-%.1f), plain torch %.1f us (%.1f-%.1f), ratio %.2f"
             % (B, hs, F, L, m_o * 1e6, lo_o * 1e6, hi_o * 1e6, m_p * 1e6, lo_p * 1e6, hi_p * 1e6, m_p / m_o))
        # the fused cell alone against what it replaces: the library's own chain of launches (gather + cat in torch, pack,
        # the input-projection GEMM, vt_lstm_step_f32) and torch's embedding + cat + LSTMCell
        from visitron_amd import ops, rollout
        w = ours._weights()

        def cell_fused():
            return ops.turn_lstm_cell((action.reshape(-1), w["table"]), feature, h0, c0, w["w_ih"], w["w_hh"], w["b"])

        def cell_chain():
            x = torch.cat((w["table"][action.reshape(-1)], feature), 1)
            xproj = rollout._dense((x,), w["w_ih"], w["b"])
            h1, c1 = torch.empty_like(h0), c0.clone()
            ops.lstm_step(xproj.contiguous(), h0, h1, c1, w["w_hh"])
            return h1, c1

        def cell_torch():
            with torch.no_grad():
                return plain.lstm(torch.cat((plain.embedding(action.reshape(-1)), feature), 1), (h0, c0))

        for fn in (cell_fused, cell_chain, cell_torch):
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        med, lo, hi = alternate((cell_fused, cell_chain, cell_torch), iters, windows)
        emit(fh, "cell  B=%-3d hs=%d E=%d F=%d: fused %.1f us (%.1f-%.1f), library chain %.1f us (%.1f-%.1f), torch %.1f us (%.1f-%.1f)"
             % (B, hs, E, F, med[0] * 1e6, lo[0] * 1e6, hi[0] * 1e6, med[1] * 1e6, lo[1] * 1e6, hi[1] * 1e6, med[2] * 1e6,
                lo[2] * 1e6, hi[2] * 1e6))
        (m_o, m_p), (lo_o, lo_p), (hi_o, hi_p) = alternate((head_ours, head_torch), iters, windows)
        emit(fh, "head  B=%-3d A=%d (%d blocked rows): action_feedback %.1f us (%.1f-%.1f), torch chain %.1f us (%.1f-%.1f), ratio %.2f"
             % (B, a_out, len(rows), m_o * 1e6, lo_o * 1e6, hi_o * 1e6, m_p * 1e6, lo_p * 1e6, hi_p * 1e6, m_p / m_o))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epsilon", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("turn_based_bench: needs a HIP device (a CPU run gives no time)")
    fh = None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        fh = open(args.out, "a")
    if args.epsilon:
        measure_epsilon(fh)
    else:
        bench(fh, args.iters, args.windows)


if __name__ == "__main__":
    main()
