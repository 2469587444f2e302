"""Four glue kernels of csrc/rowops.hip that do one fp32 multiply (or none) and one rounding to bf16 -- dgelu_mul, scale_heads,
pack_concat, apply_dropout -- held bit for bit to the expression they compute, in sentinel-filled buffers.  Values are compared with
torch.equal on the float view (a scale or a mask of 0 makes -x * 0 = -0, which equals +0 there); bit patterns only where the
expression defines the sign of zero (a dropped element is the constant +0)."""
import numpy as np
import pytest
import torch

import helpers_gemm as hg

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SENTINEL = 12345.0
ROWS = (1, 5, 300)


def _bf16(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 2.0).to(BF16)


def _buffer(n_rows, ld, dev):
    return torch.full((n_rows + 1, ld), SENTINEL, dtype=BF16, device=dev)


def _intact(buf, rows, cols):
    s = torch.tensor(SENTINEL, dtype=BF16).float()
    b = buf.float().cpu()
    return bool((b[:rows, cols:] == s).all()) and bool((b[rows:] == s).all())


def _f32_product_rounded_to_bf16(a, b):
    """bf16(fl32(a * b)) for float tensors holding bf16 / fp32 values: the float64 product of a 8-bit and a 24-bit significand is
    exact, so .float() is the ONE fp32 rounding and .to(bf16) the second"""
    return (a.double() * b.double()).float().to(BF16)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("width", (8, 64, 200, 768))
def test_dgelu_mul_is_the_exact_product_rounded_once(dev, rows, width):
    from visitron_amd import ops

    g, h = _bf16((rows, width), 1), _bf16((rows, width), 2)
    g[0, 0], h[0, 1] = 0.0, 0.0
    buf = _buffer(rows, width, dev)                                   # (contiguous: the kernel is flat; the spare row is the sentinel)
    got = ops.dgelu_mul(g.to(dev), h.to(dev), out=buf[:rows])
    torch.cuda.synchronize()
    # the product of two bf16 values has 16 significant bits: exact in fp32, one rounding to bf16
    want = hg.round_out(g.double() * h.double(), "bf16")
    assert torch.equal(got.float().cpu().double(), want)
    assert torch.equal(ops.dgelu_mul(g.to(dev), h.to(dev)).float().cpu().double(), want)
    assert _intact(buf, rows, width)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nh", (1, 3, 12))
def test_scale_heads_strided_in_and_out(dev, rows, nh):
    from visitron_amd import ops

    W = nh * 64
    xb = torch.full((rows, W + 8), 7.0, dtype=BF16)
    xb[:, :W] = _bf16((rows, W), 3)
    g = torch.Generator().manual_seed(4)
    sc = torch.randn(nh, generator=g)
    sc[0] = 0.0 if nh > 1 else 0.37
    if nh > 2:
        sc[1] = 1.0
    buf = _buffer(rows, W + 16, dev)
    got = ops.scale_heads(xb.to(dev)[:, :W], sc.to(dev), out=buf[:rows, :W])
    torch.cuda.synchronize()
    want = _f32_product_rounded_to_bf16(xb[:, :W].float(), sc.repeat_interleave(64)[None, :])
    assert torch.equal(got.float().cpu(), want.float())
    assert _intact(buf, rows, W)
    fresh = ops.scale_heads(xb.to(dev)[:, :W], sc.to(dev))
    assert torch.equal(fresh.float().cpu(), want.float())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("d0,d1,kpad", [(5, 3, 8), (6, 2, 8), (37, 20, 64), (64, 0, 64), (131, 66, 200), (130, 66, 200),
                                        (501, 260, 768), (2054, 0, 2056)])
def test_pack_concat_is_a_plain_convert(dev, rows, d0, d1, kpad):
    from visitron_amd import ops

    g = torch.Generator().manual_seed(5)
    s0 = torch.randn((rows, d0), generator=g) * 3.0
    s1 = torch.randn((rows, d1), generator=g) * 3.0 if d1 else None
    buf = _buffer(rows, kpad, dev)
    got = ops.pack_concat(s0.to(dev), s1.to(dev) if d1 else None, kpad, out=buf[:rows])
    torch.cuda.synchronize()
    want = torch.zeros((rows, kpad), dtype=BF16)
    want[:, :d0] = s0.to(BF16)
    if d1:
        want[:, d0:d0 + d1] = s1.to(BF16)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))          # (the padding is the constant +0)
    assert _intact(buf, rows, kpad)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("width", (8, 64, 200, 768))
@pytest.mark.parametrize("p", (0.1, 0.5))
def test_apply_dropout_is_the_python_mask_and_scale(dev, rows, width, p):
    from visitron_amd import ops

    drop = (p, 1234 + rows, 17)
    x = _bf16((rows, width), 6)
    buf = _buffer(rows, width + 8, dev)
    buf[:rows, :width] = x.to(dev)
    ops.apply_dropout(buf[:rows, :width], drop)
    torch.cuda.synchronize()
    keep = torch.from_numpy(hg.keep_mask(rows * width, drop).astype(np.bool_)).view(rows, width)
    scale = torch.tensor(hg.drop_scale(p), dtype=torch.float32)
    want = torch.where(keep, _f32_product_rounded_to_bf16(x.float(), scale), torch.zeros((), dtype=BF16))
    got = buf[:rows, :width].cpu()
    assert torch.equal(got.float(), want.float())
    dropped = got.contiguous().view(torch.int16)[~keep]
    assert bool((dropped == 0).all())                                                 # a dropped element is +0, bit for bit
    assert 0 < int(keep.sum()) < keep.numel() or rows * width < 64
    assert _intact(buf, rows, width)
