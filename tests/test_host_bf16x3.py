"""CPU: the "bf16x3" precision (csrc/bf16x3_path.hip) -- the switch, the C ABI, the reference arithmetic the GPU tests check
against (tests/helpers_bf16x3.py: it must accept the right arithmetic and reject each way of getting it wrong), and the
generated gfx950 code of the kernel."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import helpers_bf16x3 as hx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visitron_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def test_precision_is_listed_and_tags_every_module():
    from visitron_amd import set_precision
    from visitron_amd.config import mini_config
    from visitron_amd.modeling import PRECISIONS, PreTrainOscar, _is_fp32, _products

    assert PRECISIONS == ("bf16", "fp32", "bf16x3")
    m = PreTrainOscar(mini_config()).eval()
    assert _products(m) == "fp32" and not _is_fp32(m)
    assert set_precision(m, "bf16x3") is m
    mods = list(m.modules())
    assert len(mods) > 10 and all(x._vt_precision == "bf16x3" for x in mods)
    assert all(_is_fp32(x) and _products(x) == "bf16x3" for x in mods)      # the fp32 route, its products on bf16x3
    set_precision(m, "fp32")
    assert all(_is_fp32(x) and _products(x) == "fp32" for x in mods)
    set_precision(m, "bf16")
    assert not any(_is_fp32(x) for x in mods)
    with pytest.raises(ValueError):
        set_precision(m, "bf16x2")


def test_header_declares_and_library_exports_the_entry_points():
    from visitron_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "visitron_hip.h")).read(), flags=re.S)

    def args(name):
        return re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % name, src, re.S).group(1))

    assert args("vt_linear_bf16x3") == args("vt_linear_f32")      # argument lists exactly those of the fp32 entry points
    assert args("vt_bmm_bf16x3") == args("vt_bmm_f32")
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vt_linear_bf16x3", "vt_bmm_bf16x3"):
        assert hasattr(raw, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("bf16x3", "f32")]
    assert _lib.load().vt_abi_version() >= 16


def test_ops_refuse_an_unknown_product_choice():
    from visitron_amd import ops

    assert ops.PRODUCTS == ("fp32", "bf16x3")
    with pytest.raises(ValueError):
        ops._products_ok("tf32")


def test_pretrain_engine_refuses_bf16x3_before_touching_the_model():
    from visitron_amd.training import PretrainEngine

    with pytest.raises(ValueError, match="'bf16' or 'fp32'"):
        PretrainEngine(None, precision="bf16x3")


def test_split_is_round_to_nearest_even_twice():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 4095.0, -4095.0, 1.0 + 2.0 ** -16, 3.0e38, 1e-30, 0.0])
    hi, lo = hx.split_rne(x)
    assert hi.tolist()[:5] == [1.0, 1.0, 1.0 + 2.0 ** -6, 4096.0, -4096.0]       # ties to even, both ways
    assert lo.tolist()[:5] == [0.0, 2.0 ** -8, -(2.0 ** -8), -1.0, 1.0]
    assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
    assert float(((x - hi - lo).abs() - hx.U16 * x.abs()).max()) <= 0.0
    v = hx.sixteen_bit_values((50, 60), 1)
    hi, lo = hx.split_rne(v)
    assert torch.equal(hi + lo, v) and not torch.equal(v[:50, :50], v[:50, :50].t())


@pytest.mark.parametrize("M,N,K,act,res,kn", hx.GEMM_CASES)
def test_helper_accepts_the_arithmetic_and_rejects_each_mistake(M, N, K, act, res, kn):
    a, w, b, r = hx.gemm_inputs(M, N, K, res, kn)
    w_nk = w.t().contiguous() if kn else w

    def ratios(prod):
        return hx.gemm_ratios(hx._epilogue(prod.double(), b, r, act, hx.ALPHA).float(), a, w_nk, b, r, act, hx.ALPHA)

    good = {"emulation": hx.emulated(a, w_nk),
            "fp32-accumulated three terms": hx.three_terms(a, w_nk, torch.float32),
            "with lo.lo": hx.three_terms(a, w_nk, torch.float32, ("ll", "lh", "hl", "hh"))}
    for name, prod in good.items():
        ra, rb = ratios(prod)
        print("ACCEPT %-30s (A) %.3f (B) %.3f" % (name, ra, rb))
        assert ra <= 1.0 and rb <= 1.0, (name, ra, rb)
    bad = {"one product": hx.three_terms(a, w_nk, torch.float32, ("hh",)),
           "missing hi.lo": hx.three_terms(a, w_nk, torch.float32, ("lh", "hh")),
           "missing lo.hi": hx.three_terms(a, w_nk, torch.float32, ("hl", "hh")),
           "lo taken as zero": hx.three_terms(a, w_nk, torch.float32, lo_zero=True)}
    for name, prod in bad.items():
        ra, rb = ratios(prod)
        print("REJECT %-30s (A) %.1f (B) %.1f" % (name, ra, rb))
        assert ra > 1.0 and rb > 1.0, (name, ra, rb)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernel_cross_compiles_without_scratch_on_the_bf16_matrix_cores(tmp_path):
    src = os.path.join(CSRC, "bf16x3_path.hip")
    out = os.path.join(str(tmp_path), "bf16x3_path.hip.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    ks = {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?\.end_amdhsa_kernel", asm, re.S | re.M)}
    gemm = [t for n, t in ks.items() if "gemm_bf16x3" in n]
    assert len(gemm) == 1
    text = gemm[0]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", text).group(1)) == 0
    assert re.search(r"^\s*v_mfma_f32_(32x32x16|16x16x32)_bf16\b", text, re.M)
    assert not re.search(r"^\s*v_mfma_f32_\d+x\d+x\d+_f32\b", text, re.M)
