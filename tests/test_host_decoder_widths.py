"""CPU: the host rules behind the decoder widths that are no multiple of 4 (the reference's default feature width 2058):
how the weight-gradient operands are padded and sliced back, and which widths take which cell route.  Plain tensors; no
library call is made."""
import pytest
import torch

from visitron_amd import rollout
from visitron_amd import rollout_autograd as ra


@pytest.mark.parametrize("N,K", [(134, 262), (2048, 2122), (2058, 2058), (5, 1), (7, 6)])
def test_weight_gradient_operands_are_padded_and_the_results_are_views(N, K):
    """K % 4 != 0: both bf16 operands run at their zero-padded widths (multiples of 8), dW / db are written whole into padded
    buffers and the caller gets the [:N, :K] / [:N] views of exactly those buffers."""
    M = 3
    g = torch.Generator().manual_seed(N + K)
    dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    dy16, x16 = ra._bf16_rows(dy), ra._bf16_rows(x)
    Np, Kp = -(-N // 8) * 8, -(-K // 8) * 8
    assert dy16.shape == (M, Np) and x16.shape == (M, Kp) and dy16.dtype == x16.dtype == torch.bfloat16
    assert torch.equal(dy16[:, :N], dy.to(torch.bfloat16)) and torch.equal(x16[:, :K], x.to(torch.bfloat16))
    assert float(dy16[:, N:].float().abs().sum()) == 0.0 and float(x16[:, K:].float().abs().sum()) == 0.0   # zero columns
    pr = ra._wgrad_problem(dy16, x16, N, K)
    run = pr["run"]
    assert run["dy"] is dy16 and run["x"] is x16
    assert run["dw"].shape == (Np, Kp) and run["db"].shape == (Np,) and run["dw"].is_contiguous()
    assert run["dw"].dtype == run["db"].dtype == torch.float32
    # what the kernel's checks ask of a problem: K % 4 == 0, operand strides % 8 == 0, dW stride % 4 == 0
    assert run["dw"].shape[1] % 4 == 0 and run["dy"].stride(0) % 8 == 0 and run["x"].stride(0) % 8 == 0
    assert pr["dw"].shape == (N, K) and pr["db"].shape == (N,)
    assert pr["dw"].data_ptr() == run["dw"].data_ptr() and pr["dw"].stride() == (Kp, 1)
    assert pr["db"].data_ptr() == run["db"].data_ptr()
    # the padded product restricted to the views IS the product of the unpadded operands
    full = dy16.float().t() @ x16.float()
    assert torch.equal(full[:N, :K], dy.to(torch.bfloat16).float().t() @ x.to(torch.bfloat16).float())
    assert float(full[N:].abs().sum()) == 0.0 and float(full[:, K:].abs().sum()) == 0.0


@pytest.mark.parametrize("N,K", [(2048, 2116), (134, 128), (2058, 512), (6, 4)])
def test_weight_gradient_problem_at_multiples_of_4_is_what_it_was(N, K):
    """K % 4 == 0 (any N): the problem runs at its own size on column views of the operands, as before."""
    M = 2
    dy16, x16 = ra._bf16_rows(torch.ones(M, N)), ra._bf16_rows(torch.ones(M, K))
    pr = ra._wgrad_problem(dy16, x16, N, K)
    run = pr["run"]
    assert run["dw"] is pr["dw"] and run["db"] is pr["db"]
    assert pr["dw"].shape == (N, K) and pr["db"].shape == (N,) and pr["dw"].is_contiguous()
    assert run["dy"].shape == (M, N) and run["x"].shape == (M, K)
    assert run["dy"].data_ptr() == dy16.data_ptr() and run["x"].data_ptr() == x16.data_ptr()


def test_cell_route_by_input_width():
    """embedding + feature a multiple of 4: input projection + vt_lstm_step_f32, the shipped route.  Anything else: the fused
    cell, which reads [action_embeds | attn_feat] by address."""
    for emb, feat, fused in [(64, 2052, False), (64, 132, False), (64, 2048, False), (64, 2058, True), (64, 134, True),
                             (64, 2054, True), (64, 133, True), (62, 134, False), (63, 133, False), (62, 2052, True)]:
        assert rollout.fused_cell(emb, feat) is fused, (emb, feat)
    dec = rollout.AttnDecoderLSTM(4, 64, 128, 0.5, feature_size=134)
    assert dec.lstm.weight_ih.shape == (512, 198) and rollout.fused_cell(dec.embedding_size, dec.feature_size)
    assert not rollout.fused_cell(64, rollout.AttnDecoderLSTM(4, 64, 128, 0.5).feature_size)   # the default 2052


def test_dense_route_takes_the_skinny_kernel_at_every_width(monkeypatch):
    """rollout._dense: up to SKINNY_ROWS rows every input width goes to ops.skinny_linear (one launch); more rows take the
    packing pass and the tiled GEMM, as before."""
    calls = []
    monkeypatch.setattr(rollout.ops, "skinny_linear", lambda s0, w, b, s1, act: calls.append(("skinny", s0.shape[1], None if s1 is None else s1.shape[1])) or "S")
    monkeypatch.setattr(rollout.ops, "pack_concat", lambda s0, s1, kpad: calls.append(("pack", s0.shape[1])) or torch.zeros(s0.shape[0], kpad))
    monkeypatch.setattr(rollout.ops, "linear", lambda a, w, bias, act, out, out_f32: calls.append(("gemm", a.shape[0])))
    w = torch.zeros(8, 2176, dtype=torch.bfloat16)
    for k0, k1 in [(2058, None), (134, 128), (64, 2058), (3, None), (2052, 512)]:
        parts = (torch.zeros(5, k0),) + (() if k1 is None else (torch.zeros(5, k1),))
        assert rollout._dense(parts, w) == "S"
    assert calls == [("skinny", 2058, None), ("skinny", 134, 128), ("skinny", 64, 2058), ("skinny", 3, None), ("skinny", 2052, 512)]
    del calls[:]
    rollout._dense((torch.zeros(rollout.SKINNY_ROWS + 1, 2058),), w)
    assert [c[0] for c in calls] == ["pack", "gemm"]
