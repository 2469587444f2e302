"""The rectangular attention (S new positions over Sh + S keys) against the square kernels run over all St = Sh + S rows -- the
detour the 2-D-mask inference history route still takes -- forward and backward, B = 8, 12 heads, head size 64.

One process; per shape the two forms alternate in ROUNDS rounds of ITERS launches each (device events around each group, after a
warm-up of both), and the table gives each form's median round and the spread of its rounds.  A measurement, no decision: no
default is switched on it.     python tools/attn_rect_bench.py [out.txt]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from visitron_amd import ops

B, NH, ROUNDS, ITERS = 8, 12, 7, 200
SHAPES = ((32, 228), (228, 228), (256, 16), (511, 1))   # (Sh, S)
H = NH * 64
dev = "cuda:0"


def group_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e3


def alternate(fns):
    for fn in fns:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    rounds = [[] for _ in fns]
    for _ in range(ROUNDS):
        for r, fn in zip(rounds, fns):
            r.append(group_us(fn))
    return [(statistics.median(r), min(r), max(r)) for r in rounds]


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = ["# rectangular attention vs the square kernels over St rows: B = %d, %d heads, no dropout, 2-D mask; us per launch," % (B, NH),
             "# median of %d alternating rounds of %d launches (min .. max of the rounds)" % (ROUNDS, ITERS),
             "# %-4s %-4s %-5s | %-28s %-28s %-6s | %-28s %-28s %-6s" % ("Sh", "S", "St", "fwd rect", "fwd square(St)", "ratio",
                                                                       "bwd rect", "bwd square(St)", "ratio")]
    g = torch.Generator(device="cpu").manual_seed(0)
    for Sh, S in SHAPES:
        St = Sh + S
        qkv = (torch.randn(B * St, 3 * H, generator=g) * 0.8).to(dev, torch.bfloat16)
        mask = torch.ones(B, St, device=dev)
        mask[:, 1] = 0
        d_rect = torch.randn(B * S, H, generator=g).to(dev, torch.bfloat16)
        d_sq = torch.zeros(B, St, H, device=dev, dtype=torch.bfloat16)
        d_sq[:, Sh:] = d_rect.view(B, S, H)
        d_sq = d_sq.view(B * St, H)
        lse_r, lse_s = torch.zeros(B, NH, S, device=dev), torch.zeros(B, NH, St, device=dev)
        ctx_r, ctx_s = torch.empty(B * S, H, device=dev, dtype=torch.bfloat16), torch.empty(B * St, H, device=dev, dtype=torch.bfloat16)
        g_r, g_s = (torch.empty(B * St, 3 * H, device=dev, dtype=torch.bfloat16) for _ in range(2))
        delta = torch.empty(B, NH, St, device=dev)
        need = ops.attention_bwd_ws_bytes(B, St, NH, B * St)
        dq32 = torch.empty(max(need // 4, 1), dtype=torch.float32, device=dev)
        fwd = alternate([lambda: ops.attention_rect_fwd(qkv, B, S, St, NH, mask=mask, out=ctx_r, lse=lse_r),
                         lambda: ops.attention_fwd(qkv, B, St, NH, mask=mask, out=ctx_s, lse=lse_s)])
        same = float((ctx_r.view(B, S, H).float() - ctx_s.view(B, St, H)[:, Sh:].float()).abs().max())
        bwd = alternate([lambda: ops.attention_rect_bwd(qkv, d_rect, ctx_r, lse_r, B, S, St, NH, mask=mask, out=g_r),
                         lambda: ops.attention_bwd(qkv, d_sq, ctx_s, lse_s, B, St, NH, mask=mask, out=g_s, delta_ws=delta,
                                                   dq32_ws=dq32 if need else None)])
        cell = lambda t: "%9.1f (%8.1f .. %8.1f)" % t
        lines.append("  %-4d %-4d %-5d | %-28s %-28s %-6.2f | %-28s %-28s %-6.2f   max|ctx rect - square| %.4f" % (
            Sh, S, St, cell(fwd[0]), cell(fwd[1]), fwd[0][0] / fwd[1][0], cell(bwd[0]), cell(bwd[1]), bwd[0][0] / bwd[1][0], same))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
