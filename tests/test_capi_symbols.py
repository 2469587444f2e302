"""CPU: the C-ABI library loads and exports every function include/visitron_hip.h declares, and the
ctypes binding, which is derived from that header, lists exactly those with the types written out here
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "visitron_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_entry_points():
    names = _declared()
    for must in ("vt_linear_bf16", "vt_attention_fwd_bf16", "vt_layernorm_bf16", "vt_embed_layernorm",
                 "vt_pack_concat_bf16", "vt_encoder_forward_bf16", "vt_error_string", "vt_abi_version"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from visitron_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    assert sorted(_lib.SIGNATURES) == _declared()
    loaded = _lib.load()
    assert loaded.vt_abi_version() >= 1
    assert loaded.vt_error_string(0) == b"ok" and loaded.vt_error_string(-4) == b"unsupported configuration"


def test_struct_layouts_match_the_header():
    from visitron_amd import _lib

    assert ctypes.sizeof(_lib.LayerWeights) == 12 * ctypes.sizeof(ctypes.c_void_p)
    # vt_layer_acts: 16 pointers, then two int32 (ln_residual_mode, reserved0: ABI 10)
    assert ctypes.sizeof(_lib.LayerActs) == 16 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert _lib.LayerActs.ln_residual_mode.offset == 16 * ctypes.sizeof(ctypes.c_void_p)
    src = open(os.path.join(ROOT, "include", "visitron_hip.h")).read()
    for struct, cls in (("vt_layer_weights", _lib.LayerWeights), ("vt_layer_acts", _lib.LayerActs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(?:\*|int32_t)\s*([a-z0-9_]+)\s*;", body)
        assert fields == [f[0] for f in cls._fields_], struct


# ---- the binding is derived from the header: pin the derivation from outside, with literals ----------------------------
_P, _I, _L, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_DROP = [_F, ctypes.c_uint64, ctypes.c_uint32]   # (p, step seed, site)


def _struct_ptr(name):
    from visitron_amd import _lib

    return ctypes.POINTER(getattr(_lib, name))


def _pinned():
    """name -> (restype, argtypes), written by hand from include/visitron_hip.h: one entry per rule of the binding."""
    return {
        # const char* return; int64_t, float and void returns
        "vt_error_string": (ctypes.c_char_p, [_I]),
        "vt_gemm_workspace_region_bytes": (_L, []),
        "vt_attn_dropout_effective": (_F, [_F]),
        "vt_gemm_tune": (None, [_I, _I, _I, _I, _I]),
        # the dropout triple (float, uint64_t, uint32_t) and vt_stream_t
        "vt_apply_dropout_bf16": (_I, [_P, _L, _L, _I] + _DROP + [_P]),
        # unsigned*
        "vt_wgrad_turn_timeouts": (_I, [ctypes.POINTER(ctypes.c_uint)]),
        # pointers to the mirrored structs (all seven over these four entries)
        "vt_encoder_backward_seq_bf16": (_I, [
            _struct_ptr("LayerWeights"), _struct_ptr("LayerWeightsT"), _struct_ptr("LayerActs"), _struct_ptr("LayerGrads"),
            _I, _P, _P, _struct_ptr("BwdWorkspace"), _struct_ptr("BwdWorkspace"), _I, _I, _I, _I, _I, _F, _I, _F, _F,
            ctypes.c_uint64, _I, _L, _P, _P, _P, _P]),
        "vt_encoder_forward_ln_bf16": (_I, [_struct_ptr("LayerWeightsLn"), _I] + [_P] * 10 + [
            _I, _P, _I, _I, _I, _I, _I, _F, _L, _P]),
        "vt_wgrad_bf16": (_I, [_struct_ptr("WgradProblem"), _I, _I, _P]),
        # pointer to pointer, const in every position
        "vt_transpose_batch_bf16": (_I, [_P, _P, _P, _P, _P, _P, _I, _P]),
        # the longest list: 34 arguments
        "vt_gemm_f32_ex": (_I, [_P, _L, _L, _L, _I, _P, _L, _L, _L, _I, _P, _P, _L, _P, _L, _L, _L, _P, _I, _I, _I, _I, _F,
                                _I, _I, _I, _I, _I, _I, _P, _F, ctypes.c_uint64, ctypes.c_uint32, _P]),
    }


def test_derived_signatures_match_the_written_ones():
    from visitron_amd import _lib

    lib = _lib.load()
    for name, (restype, argtypes) in _pinned().items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is restype, name
        assert len(got_args) == len(argtypes), name
        assert got_args == argtypes, name
        fn = getattr(lib, name)   # and load() installs exactly that on the symbol
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_struct_sizes_and_offsets_are_the_abi():
    from visitron_amd import _lib

    # the same seven numbers are static_asserts beside the includes of visitron_amd/csrc/capi.hip
    sizes = {"LayerWeights": 96, "LayerActs": 136, "LayerWeightsLn": 96, "LayerWeightsT": 32, "LayerGrads": 96,
             "BwdWorkspace": 80, "WgradProblem": 72}
    for name, size in sizes.items():
        cls = getattr(_lib, name)
        assert issubclass(cls, ctypes.Structure) and cls.__name__ == name
        assert ctypes.sizeof(cls) == size, name
    # first non-pointer field of the two structs that have one
    assert _lib.WgradProblem.ldy.offset == 8 and _lib.WgradProblem.ldy.size == 8
    assert _lib.WgradProblem.N.offset == 56 and _lib.WgradProblem.accumulate.offset == 64
    assert _lib.LayerActs.ln_residual_mode.offset == 128 and _lib.LayerActs.ln_residual_mode.size == 4
    assert _lib.LayerActs.reserved0.offset == 132


def test_binding_refuses_what_it_has_no_rule_for(monkeypatch, tmp_path):
    from visitron_amd import _lib

    for base, stars in (("double", ""), ("size_t", ""), ("char", "*"), ("vt_layer_acts", "**"), ("unsigned", "")):
        with pytest.raises(ImportError, match="no ctypes rule"):
            _lib._ctype(base, stars, "int vt_x(%s%s a)" % (base, stars))
    missing = str(tmp_path / "include" / "visitron_hip.h")
    monkeypatch.setattr(_lib, "_HEADER", missing)
    with pytest.raises(ImportError, match=re.escape(missing)):
        _lib._parse_header()


def test_header_constants_are_the_literals_the_modules_carried():
    from visitron_amd import _lib, ops, optim

    assert _lib.CONSTANTS == {
        "VT_OK": 0, "VT_ERR_BAD_SHAPE": -1, "VT_ERR_BAD_ALIGN": -2, "VT_ERR_NULL": -3, "VT_ERR_UNSUPPORTED": -4, "VT_ERR_HIP": -5,
        "VT_ACT_NONE": 0, "VT_ACT_GELU": 1, "VT_ACT_TANH": 2, "VT_ACT_MUL": 3,
        "VT_OPTIM_CHUNK": 65536, "VT_OPTIM_ENTRY_WORDS": 6, "VT_OPTIM_HYPER_FLOATS": 8}
    assert (_lib.VT_OK, _lib.VT_ERR_BAD_SHAPE, _lib.VT_ERR_BAD_ALIGN, _lib.VT_ERR_NULL, _lib.VT_ERR_UNSUPPORTED,
            _lib.VT_ERR_HIP) == (0, -1, -2, -3, -4, -5)
    assert (ops.ACT_NONE, ops.ACT_GELU, ops.ACT_TANH, ops.ACT_MUL) == (0, 1, 2, 3)
    assert (optim.CHUNK, optim.ENTRY_WORDS, optim.HYPER_FLOATS) == (65536, 6, 8)


@pytest.mark.parametrize("define", [
    "#define VT_X",                      # no value
    "#define VT_X 0x10",                 # not a decimal integer
    "#define VT_X (1 << 4)",             # an expression
    "#define VT_X(a) ((a) + 1)",         # a function-like macro that is not on the list
    "#define VT_KEEP_WORDS_2(B) (B)",    # a listed name as a prefix only
    "#define VT_OK 0",                   # a constant twice
    "#define OTHER 1",
])
def test_binding_refuses_a_define_outside_the_rule(monkeypatch, tmp_path, define):
    from visitron_amd import _lib

    src = open(os.path.join(ROOT, "include", "visitron_hip.h")).read()
    hdr = tmp_path / "visitron_hip.h"
    hdr.write_text(src.replace("#define VT_OPTIM_CHUNK 65536", define + "\n#define VT_OPTIM_CHUNK 65536"))
    assert define in hdr.read_text()
    monkeypatch.setattr(_lib, "_HEADER", str(hdr))
    with pytest.raises(ImportError, match=re.escape(define)):
        _lib._parse_header()
