"""The dx-only form of the LayerNorm backward (dgamma = dbeta = None: a frozen LayerNorm) against the full kernel, and one child
process of tests/test_gpu_ln_bwd_dx_only.py for the instantiations behind a non-default VT_LN_BWD_ROWS (read once per process):

    python tests/ln_dx_only_worker.py <value of VT_LN_BWD_ROWS>

Every case runs the full call and the dx-only call on the same operands: dx, and dx_dropped where asked for, must be bitwise
equal (the dx-only kernels go through the same instructions in the same order), and a sentinel-filled partial workspace must come
back untouched (no partial row is written, nothing is reduced).  One `SAME <case>` line per case, `DONE <cases>` at the end."""
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

SENTINEL = -12345.5
# H: 128 -> the chunked kernel at every switch value; 256 / 768 -> the row kernels (C4 only / C8 + C4) unless the switch is 0.
# M: fewer rows than one workgroup's four waves (times R rows each), and several workgroups with a ragged tail.
CASES = [dict(H=H, M=M, dropped=dropped, f16=f16)
         for H, M, dropped, f16 in itertools.product((128, 256, 768), (5, 130), (False, True), (False, True))]


def case_name(c):
    return "H%d M%d %s %s" % (c["H"], c["M"], "dropped" if c["dropped"] else "plain", "f16" if c["f16"] else "bf16")


def run_case(c, dev):
    """-> list of what differs (empty: the case holds)."""
    from visitron_amd import ops

    H, M = c["H"], c["M"]
    g = torch.Generator().manual_seed(1000 * H + 10 * M + int(c["dropped"]))
    x = (torch.randn(M, H, generator=g) * 1.5 + 0.3).to(dev).to(ops.F16 if c["f16"] else ops.BF16)
    dy = torch.randn(M, H, generator=g).to(dev).to(ops.BF16)
    gamma = (1.0 + 0.1 * torch.randn(H, generator=g)).to(dev)
    drop = (0.1, 0x1234ABCD5678, ops.site_out(1)) if c["dropped"] else ops.NO_DROP

    def call(full):
        dx = torch.full((M, H), 7.0, dtype=ops.BF16, device=dev)
        dxd = torch.full((M, H), 7.0, dtype=ops.BF16, device=dev) if c["dropped"] else None
        ws = torch.full((ops.LN_BWD_WS_ROWS * 2 * H,), SENTINEL, dtype=torch.float32, device=dev)
        dg = torch.zeros(H, dtype=torch.float32, device=dev) if full else None
        db = torch.zeros(H, dtype=torch.float32, device=dev) if full else None
        ops.layernorm_bwd(x, dy, gamma, 1e-12, dg, db, dx=dx, ws=ws, dx_dropped=dxd, drop=drop)
        torch.cuda.synchronize()
        return dx, dxd, ws, dg

    dx_f, dxd_f, ws_f, dg_f = call(True)
    dx_o, dxd_o, ws_o, _ = call(False)
    bad = []
    if not torch.equal(dx_f.view(torch.int16), dx_o.view(torch.int16)):
        bad.append("dx differs from the full kernel's in %d elements" % int((dx_f.view(torch.int16) != dx_o.view(torch.int16)).sum()))
    if c["dropped"] and not torch.equal(dxd_f.view(torch.int16), dxd_o.view(torch.int16)):
        bad.append("dx_dropped differs from the full kernel's")
    if c["dropped"] and torch.equal(dxd_o.view(torch.int16), dx_o.view(torch.int16)):
        bad.append("dx_dropped carries no dropout")
    if not bool((ws_o == SENTINEL).all()):
        bad.append("the dx-only call wrote into partial_ws")
    # (the comparison means something: the full call did write its partial rows and a gradient)
    if bool((ws_f == SENTINEL).all()) or not bool(dg_f.abs().sum() > 0) or not bool(torch.isfinite(dx_o.float()).all()):
        bad.append("the full call left no trace to compare with")
    return bad


def run_without_workspace(dev):
    """The dx-only call needs no partial workspace at all; dgamma without dbeta is refused."""
    from visitron_amd import _lib, ops

    x = torch.randn(6, 256, device=dev).to(ops.BF16)
    dy = torch.randn(6, 256, device=dev).to(ops.BF16)
    gamma = torch.ones(256, device=dev)
    dx = torch.empty_like(x)
    rc = _lib.load().vt_layernorm_bwd_bf16(
        ops._ptr(x), 256, ops._ptr(dy), 256, ops._ptr(gamma), ops._ptr(dx), 256, None, None, None, 6, 256, 1e-12, 0, None, 0,
        0.0, 0, 0, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.VT_OK
    want = ops.layernorm_bwd(x, dy, gamma, 1e-12, torch.zeros(256, device=dev), torch.zeros(256, device=dev))
    assert torch.equal(dx.view(torch.int16), want.view(torch.int16))
    rc = _lib.load().vt_layernorm_bwd_bf16(
        ops._ptr(x), 256, ops._ptr(dy), 256, ops._ptr(gamma), ops._ptr(dx), 256, ops._ptr(torch.zeros(256, device=dev)), None,
        None, 6, 256, 1e-12, 0, None, 0, 0.0, 0, 0, ops._stream())
    assert rc == _lib.VT_ERR_NULL


def main():
    assert os.environ.get("VT_LN_BWD_ROWS") == sys.argv[1], "VT_LN_BWD_ROWS must be %s in this process" % sys.argv[1]
    dev = torch.device("cuda", 0)
    failed = 0
    for c in CASES:
        bad = run_case(c, dev)
        print("%s %s%s" % ("DIFF" if bad else "SAME", case_name(c), "".join("\n    " + b for b in bad)))
        failed += bool(bad)
    print("DONE %d" % len(CASES))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
