"""CPU: the rectangular attention (csrc/attention_rect.hip) -- the comparison the GPU tests use must accept the minimal bf16
implementation and reject each way of moving the data wrongly (tests/helpers_attention_rect.py); the C ABI; the generated gfx950
code; and the semantics the model-level GPU tests hold the product to (the oracle's history gradient)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import helpers_attention as ha
import helpers_attention_rect as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visitron_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
P_DROP = 0.1

_cases = {}


def _case(shape, form, drop):
    key = (shape, form, drop)
    if key not in _cases:
        B, nh, Sh, Sq = shape
        keep = hr.random_keep(B, nh, Sq, Sh + Sq, P_DROP) if drop else None
        _cases[key] = hr.Case(B, nh, Sh, Sq, form, keep=keep, p_eff=P_DROP if drop else 0.0)
    return _cases[key]


def _judge(case, mutant=None):
    ctx, lse, dqkv = hr.packed_model(case, mutant)
    good_ctx = ctx if mutant is None else hr.packed_model(case)[0]
    out = hr.judge_forward(case, ctx, lse)
    out.update(hr.judge_backward(case, good_ctx, dqkv))
    return out


@pytest.mark.parametrize("shape", hr.SHAPES)
def test_comparison_accepts_the_minimal_bf16_model(shape):
    for form, drop in (("none", False), ("causal", True)):
        case = _case(shape, form, drop)
        ratios = _judge(case)
        print("ACCEPT %-36s %s" % (case.label(), "  ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
        assert ha.passes(ratios), (case.label(), ratios)


def test_keep_words_round_trip():
    keep = hr.random_keep(2, 3, 33, 333, 0.3)
    words = hr.pack_keep_words(keep)
    assert words.numel() == 2 * 3 * 2 * 352 and words.dtype == torch.int32
    assert torch.equal(hr.unpack_keep_words(words, 2, 3, 33, 333), keep)


@pytest.mark.parametrize("mutant", hr.MUTANTS)
def test_comparison_rejects_each_mutant(mutant):
    caught = []
    for shape in hr.SHAPES:
        if shape[2] + shape[3] > 400 and mutant != "dq_block_crossing_256_not_added":
            continue    # the small shapes show every other mutant; the large ones only cost time here
        case = _case(shape, "causal", True)
        if not ha.passes(_judge(case, mutant)):
            caught.append(case.label())
    print("REJECT %-36s on %d cases: %s" % (mutant, len(caught), "; ".join(caught)))
    assert caught, mutant


def test_header_declares_and_library_exports_the_entry_points():
    from visitron_amd import _lib, ops

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vt_attention_rect_fwd_bf16", "vt_attention_rect_bwd_bf16"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(raw, name), name
    assert len(_lib.SIGNATURES["vt_attention_rect_fwd_bf16"][1]) == 18
    assert len(_lib.SIGNATURES["vt_attention_rect_bwd_bf16"][1]) == 21
    assert _lib.load().vt_abi_version() >= 18
    assert ops.keep_words_rect(2, 3, 33, 333) == 2 * 3 * 2 * 352
    assert ops.keep_words_rect(2, 3, 100, 100) == ops.keep_words(2, 3, 100)
    qkv, c = torch.zeros(4, 192, dtype=torch.bfloat16), torch.zeros(2, 64, dtype=torch.bfloat16)   # B 1, Sq 2, Sk 4, one head
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.attention_rect_fwd(qkv, 1, 2, 4, 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        ops.attention_rect_bwd(qkv, c, c, torch.zeros(1, 1, 2), 1, 2, 4, 1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kernels_cross_compile_without_scratch_on_the_bf16_matrix_cores(tmp_path):
    src = os.path.join(CSRC, "attention_rect.hip")
    out = os.path.join(str(tmp_path), "attention_rect.hip.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    ks = {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?\.end_amdhsa_kernel", asm, re.S | re.M)}
    names = sorted(n for n in ks if "attention_rect" in n)
    assert len(names) == 3 and len(ks) == 3, sorted(ks)
    for n in names:
        text = ks[n]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", text).group(1)) == 0, n
        assert re.search(r"^\s*v_mfma_f32_(32x32x16|16x16x32)_bf16\b", text, re.M), n
        assert not re.search(r"^\s*(global|flat|buffer)_atomic", text, re.M), n


def test_oracle_history_states_receive_a_gradient():
    """oscar/modeling_bert.py:37-41, 148-155 under autograd: the history enters keys and values, so it has a gradient."""
    from oracle.modeling import BertImgModelwithLocationEmbeds
    from visitron_amd.config import mini_config

    cfg = mini_config()
    torch.manual_seed(0)
    m = BertImgModelwithLocationEmbeds(cfg).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    B, T, Sh = 2, 6, 4
    ids = torch.randint(1, cfg.vocab_size, (B, T))
    hist = [torch.randn(B, Sh, cfg.hidden_size, requires_grad=True) for _ in range(cfg.num_hidden_layers)]
    mask = torch.ones(B, Sh + T)
    mask[0, 1] = 0
    out = m(ids, attention_mask=mask, encoder_history_states=hist)
    out[0].square().sum().backward()
    for h in hist:
        assert h.grad is not None and float(h.grad.abs().max()) > 0
        assert float(h.grad[0, 1].abs().max()) < float(h.grad[0, 0].abs().max())   # the masked history key: next to nothing
