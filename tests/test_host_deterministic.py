"""Deterministic training mode, the parts that need no device: the three entry points in the header and the library, the
workspace arithmetic of vt_attention_bwd_ws_bytes, the switch's round trip, and ops.attention_bwd refusing a workspace that is
too small before anything is launched."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vt_set_deterministic", "vt_get_deterministic", "vt_attention_bwd_ws_bytes")


@pytest.fixture()
def ops():
    from visitron_amd import ops as o

    o.set_deterministic(False)
    try:
        yield o
    finally:
        o.set_deterministic(False)


def test_header_declares_the_three_entry_points_once():
    import ctypes

    from visitron_amd import _lib

    src = open(os.path.join(ROOT, "include", "visitron_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    for name in NEW:
        assert len(re.findall(r"\b%s\s*\(" % name, code)) == 1, name
    assert _lib.SIGNATURES["vt_set_deterministic"] == (None, [ctypes.c_int])
    assert _lib.SIGNATURES["vt_get_deterministic"] == (ctypes.c_int, [])
    assert _lib.SIGNATURES["vt_attention_bwd_ws_bytes"] == (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64])
    lib = _lib.load()
    assert lib.vt_abi_version() >= 15
    internal = open(os.path.join(ROOT, "visitron_amd", "csrc", "dispatch.hpp")).read()
    assert len(re.findall(r"\bvt_attention_bwd_ws_bytes_impl\s*\(", internal)) == 1


def test_switch_round_trips(ops):
    import visitron_amd

    assert ops.is_deterministic() is False            # the default
    visitron_amd.set_deterministic(True)
    assert visitron_amd.is_deterministic() is True and ops.is_deterministic() is True
    visitron_amd.set_deterministic(7)                 # any truth value
    assert ops.is_deterministic() is True
    visitron_amd.set_deterministic(False)
    assert visitron_amd.is_deterministic() is False


@pytest.mark.parametrize("B,S,nh,rows", [(2, 513, 2, None), (2, 767, 12, None), (8, 767, 12, 4321), (2, 513, 2, 813), (1, 257, 1, None),
                                         (3, 512, 4, None), (2, 1025, 2, None), (70000, 767, 12, None)])
def test_workspace_bytes(ops, B, S, nh, rows):
    r = B * S if rows is None else rows
    slab = r * nh * 64 * 4
    assert ops.attention_bwd_ws_bytes(B, S, nh, rows) == slab
    ops.set_deterministic(True)
    assert ops.attention_bwd_ws_bytes(B, S, nh, rows) == slab * ((S + 255) // 256)
    ops.set_deterministic(False)
    assert ops.attention_bwd_ws_bytes(B, S, nh, rows) == slab


@pytest.mark.parametrize("S", [1, 228, 255, 256])
def test_no_workspace_up_to_256_keys(ops, S):
    for on in (False, True):
        ops.set_deterministic(on)
        assert ops.attention_bwd_ws_bytes(4, S, 12) == 0
        assert ops.attention_bwd_ws_bytes(4, S, 12, 3 * S + 1) == 0


def test_attention_bwd_refuses_an_undersized_workspace(ops, monkeypatch):
    """The size check sits in front of the launch and asks the library: what is enough with the switch off (one slab) is
    refused with it on (three planes), and a workspace of the wrong dtype is refused in either mode.  No device here: the
    tensors are CPU tensors and only the device check is stood down -- the call must raise before it reaches the library."""
    import torch

    B, S, nh = 2, 513, 2
    H = nh * 64
    monkeypatch.setattr(ops, "_require_hip", lambda *a: None)
    z = lambda *shape: torch.zeros(shape, dtype=torch.bfloat16)
    args = (z(B * S, 3 * H), z(B * S, H), z(B * S, H), torch.zeros(B, nh, S), B, S, nh)
    kw = dict(out=z(B * S, 3 * H), delta_ws=torch.zeros(B, nh, S))
    slab = B * S * H
    ops.set_deterministic(True)
    for ws in (torch.zeros(slab), torch.zeros(3 * slab - 1), torch.zeros(3 * slab, dtype=torch.float64)):
        with pytest.raises(ValueError, match="dq32_ws"):
            ops.attention_bwd(*args, dq32_ws=ws, **kw)
    ops.set_deterministic(False)
    with pytest.raises(ValueError, match="dq32_ws"):
        ops.attention_bwd(*args, dq32_ws=torch.zeros(slab - 1), **kw)
