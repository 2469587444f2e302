"""The loss heads (csrc/loss_heads.hip: ce_softmax_rows, ce_softmax_rows_reg<8|32>, ce_double_softmax_rows, action_head_rows; bf16 and
fp32 gradient rows) against the float64 reference and the derived per-element bounds of tests/helpers_loss.py, through
visitron_amd.ops only.  Alone:  python -m pytest tests/test_gpu_loss_conformance.py -m gpu -q -s

Every input row has +50.0 behind its last column, every gradient lands in a sentinel-filled buffer with a spare row and a row stride
above Vpad, every case runs twice (identical bits: there are no atomics) and once more without a gradient where the wrapper allows
it (identical loss and argmax bits).  measured / bound of every check goes through helpers.check_close against 1; exact
constructions, ties, padding and sentinels carry the bound 0 (any difference is an infinite ratio)."""
import collections

import pytest
import torch

import helpers_loss as hl
from helpers import check_close

pytestmark = pytest.mark.gpu

EXACT = ("onehot", "uniform", "ties")


def _group(c):
    if c.head == "ce":
        return "%s %s" % (c.reaches, "exact constructions and ties" if c.kind in EXACT else "random rows")
    if c.head == "double":
        return "ce_double_softmax_rows"
    return "action_head_rows %s" % ("ties" if c.kind == "ties" else "B = %d" % c.rows)


GROUPS = collections.OrderedDict()
for _c in hl.all_cases():
    GROUPS.setdefault(_group(_c), []).append(_c)

@pytest.fixture(scope="module")
def bf16_rows():
    """case name -> (case, dz [rows, V] float64) of the bf16 runs of this module, for the pooled signed statistic: test_loss_heads
    leaves its results here, and the statistic's test runs whatever is missing (alone, under -k, on another worker) itself"""
    return {}


def _assert_ratios(name, rs):
    failed = []
    for key in sorted(rs):
        try:
            check_close("loss conformance %s: %s" % (name, key), abs(rs[key]) if rs[key] == rs[key] else hl.INF, 0.0, 1.0)
        except AssertionError as e:
            failed.append(str(e))
    return failed


def _run_case(case, fmt, dev, bf16_rows):
    I = hl.inputs(case)
    out = hl.run(case, fmt, dev)
    rs = hl.judge(case, fmt, out)
    rs["two calls give the same bits"] = 0.0 if hl.same_bits(out, hl.run(case, fmt, dev)) else hl.INF
    if case.head != "action":
        bare = hl.run(case, fmt, dev, grad=False)
        same = hl.same_bits({"loss": out["loss"], "amax": out["amax"]}, {"loss": bare["loss"], "amax": bare["amax"]})
        rs["dz = None gives the same loss and argmax bits"] = 0.0 if same else hl.INF
    if fmt == "bf16":
        bf16_rows[case.name] = (case, out["dzbuf"][:I.rows, :case.V].to(torch.float64))
    return rs


@pytest.mark.parametrize("group", list(GROUPS))
def test_loss_heads(dev, bf16_rows, group):
    failed = []
    top = collections.defaultdict(float)
    for case in GROUPS[group]:
        for fmt in hl.FMTS:
            rs = _run_case(case, fmt, dev, bf16_rows)
            failed += _assert_ratios("%s %s" % (case.name, fmt), rs)
            for k, v in rs.items():
                key = (case.reaches, fmt, case.kind, k.split(" err/bound")[0] if "err/bound" in k else "exact checks")
                top[key] = max(top[key], abs(v) if v == v else hl.INF)
    for key in sorted(top):
        print("LOSS-GPU %s | %s | %s | %s | %.3f" % (key + (top[key],)))
    assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed[:40]))


@pytest.mark.parametrize("head", ("ce", "double", "action"))
def test_bf16_gradients_are_rounded_to_nearest(dev, bf16_rows, head):
    """helpers_attention.signed_stat pooled over the random bf16 cases of a head (the module's fixture holds the rows that
    test_loss_heads has run; the rest are run here): a truncating convert sits tens of units outside
    (tests/test_host_loss_reference.py)"""
    pairs = []
    for case in hl.cases(head):
        if not hl.mutant_applies("truncating_bf16_convert", case, "bf16") or hl.reference(case, "bf16").loss is None:
            continue
        if case.name not in bf16_rows:
            out = hl.run(case, "bf16", dev)
            bf16_rows[case.name] = (case, out["dzbuf"][:hl.inputs(case).rows, :case.V].to(torch.float64))
        pairs.append(bf16_rows[case.name])
    stat, n = hl.signed_pool(pairs)
    print("LOSS-GPU signed statistic | %s | N = %d | %.3f" % (head, n, stat))
    assert n >= 100000, n
    check_close("loss conformance %s: signed bias of the bf16 gradient" % head, abs(stat), 0.0, 1.0)


# ---- shapes and alignments the library refuses: the error code only, nothing is launched ---------------------------------------------
def _code(fn):
    with pytest.raises(RuntimeError) as e:
        fn()
    return str(e.value)


def test_refused_shapes_and_alignments(dev):
    from visitron_amd import _lib, ops

    shape, align, unsup = ("(code %d)" % c for c in (_lib.VT_ERR_BAD_SHAPE, _lib.VT_ERR_BAD_ALIGN, _lib.VT_ERR_UNSUPPORTED))
    rows, V = 3, 40
    z = torch.zeros((rows, 64), device=dev)[:, :V]
    y = torch.zeros(rows, dtype=torch.int64, device=dev)
    for f, dt in ((ops.ce_softmax_rows, torch.bfloat16), (ops.ce_softmax_rows_g32, torch.float32),
                  (ops.ce_double_softmax_rows, torch.bfloat16), (ops.ce_double_softmax_rows_g32, torch.float32)):
        buf = torch.zeros((rows + 1, 64), dtype=dt, device=dev)
        assert shape in _code(lambda: f(z, y, V, buf[:rows, :32], 1.0))                                       # Vpad < V
        assert shape in _code(lambda: f(z, y, V, buf[:rows, :44], 1.0))                                       # Vpad % 8
        assert shape in _code(lambda: f(z, y, V, torch.as_strided(buf, (rows, 48), (40, 1)), 1.0))            # lddz < Vpad
        assert align in _code(lambda: f(z, y, V, torch.as_strided(buf, (rows, 40), (60, 1)), 1.0))            # lddz % 8
        assert align in _code(lambda: f(z, y, V, torch.as_strided(buf, (rows, 40), (64, 1), 2), 1.0))         # dz off 16 bytes
        assert bool((buf == 0).all())
    zw = torch.zeros((rows, 2064), device=dev)
    for f, dt in ((ops.ce_double_softmax_rows, torch.bfloat16), (ops.ce_double_softmax_rows_g32, torch.float32)):
        buf = torch.zeros((rows, 2064), dtype=dt, device=dev)
        assert unsup in _code(lambda: f(zw[:, :2050], y, 2050, buf[:, :2056], 1.0))                          # the row is held in registers
        assert bool((buf == 0).all())
    assert unsup in _code(lambda: ops.ce_double_softmax_rows(zw[:, :2050], y, 2050, None, 1.0))
    for f, dt in ((ops.action_head, torch.bfloat16), (ops.action_head_g32, torch.float32)):
        assert shape in _code(lambda: f(torch.zeros((rows, 72), device=dev), y, 65, 1.0, 72))                 # A > 64
        assert shape in _code(lambda: f(z, y, 40, 1.0, 32))                                                   # Ap < A
        buf = torch.zeros((rows, 64), dtype=dt, device=dev)
        assert shape in _code(lambda: f(z, y, 40, 1.0, 48, dz=torch.as_strided(buf, (rows, 48), (40, 1))))    # lddz < Ap
    torch.cuda.synchronize()
