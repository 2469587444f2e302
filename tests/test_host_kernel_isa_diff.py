"""tools/kernel_isa_diff.py: its splitter and normaliser on synthetic assembly (no compiler, no GPU)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
kid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kid)

# two kernels as the compiler lays them out; %(f)d = the function's position in its file, %(t)d = a file-wide label counter
ASM = """
	.text
	.protected	_Z3fooPf
	.globl	_Z3fooPf
_Z3fooPf:                               ; @_Z3fooPf
.Lfunc_begin%(f)d:
; %%bb.0:                                ; %(note)s
	s_load_dwordx2 s[0:1], s[0:1], 0x0
	v_mov_b32_e32 v1, %(imm)s
.Ltmp%(t)d:
	s_cbranch_execz .LBB%(f)d_2
.LBB%(f)d_1:                                ; =>This Inner Loop Header: Depth=1
	global_store_dword v0, v1, s[0:1]
	s_cbranch_scc1 .LBB%(f)d_1
.LBB%(f)d_2:
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z3fooPf
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr %(vgpr)d
	.end_amdhsa_kernel
	.text
.Lfunc_end%(f)d:
	.size	_Z3fooPf, .Lfunc_end%(f)d-_Z3fooPf
	.set _Z3fooPf.num_vgpr, %(vgpr)d
_ZN12_GLOBAL__N_13barEv:                ; @_ZN12_GLOBAL__N_13barEv
	s_endpgm
	.amdhsa_kernel _ZN12_GLOBAL__N_13barEv
		.amdhsa_next_free_vgpr 1
	.end_amdhsa_kernel
"""
BASE = dict(f=0, t=3, note="first in its file", imm="0", vgpr=2)


def _norm(**kw):
    return {sym: kid.normalise(text) for sym, text in kid.kernels(ASM % dict(BASE, **kw)).items()}


def test_split_finds_each_kernel_from_label_to_descriptor_end():
    ks = kid.kernels(ASM % BASE)
    assert sorted(ks) == ["_Z3fooPf", "_ZN12_GLOBAL__N_13barEv"]
    assert ks["_Z3fooPf"].startswith("_Z3fooPf:") and ks["_Z3fooPf"].endswith(".end_amdhsa_kernel")
    assert "barEv" not in ks["_Z3fooPf"] and ".Lfunc_end" not in ks["_Z3fooPf"]
    assert "s_endpgm" in ks["_Z3fooPf"] and ".amdhsa_next_free_vgpr 2" in ks["_Z3fooPf"]


def test_label_numbers_and_comments_do_not_count():
    a, b = _norm(), _norm(f=57, t=1204, note="58th in its file ; moved")
    assert a == b and kid.compare(a, b) == []
    assert a["_Z3fooPf"][:3] == ["_Z3fooPf:", ".Lfunc_begin0:", "s_load_dwordx2 s[0:1], s[0:1], 0x0"]
    # the labels inside a kernel stay distinct: the two branch targets are not merged
    assert "s_cbranch_execz .LBB_2" in a["_Z3fooPf"] and "s_cbranch_scc1 .LBB_1" in a["_Z3fooPf"]


def test_one_instruction_or_one_descriptor_value_is_reported():
    a = _norm()
    for changed in (dict(imm="1"), dict(vgpr=3)):
        rep = kid.compare(a, _norm(f=57, **changed))
        assert len(rep) == 1 and rep[0].startswith("changed  _Z3fooPf"), rep
    rep = kid.compare(a, _norm(imm="1"))
    assert "v_mov_b32_e32 v1, 0" in rep[0] and "v_mov_b32_e32 v1, 1" in rep[0]


def test_added_and_removed_symbols_are_reported():
    a = _norm()
    less = {k: v for k, v in a.items() if k == "_Z3fooPf"}
    assert kid.compare(a, less) == ["removed  _ZN12_GLOBAL__N_13barEv"]
    assert kid.compare(less, a) == ["added    _ZN12_GLOBAL__N_13barEv"]
