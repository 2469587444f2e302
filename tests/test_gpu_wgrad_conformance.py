"""The weight-gradient family (csrc/gemm_wgrad.hip, gemm_wgrad_v8.hip with wgrad_v8_step.inc) against the float64 reference, the
derived per-element bound, the exact constructions and the turn-order fingerprint of tests/helpers_wgrad.py, through
visitron_amd.ops only.  Alone:  python -m pytest tests/test_gpu_wgrad_conformance.py -m gpu -q -s

Every case of the table names the form it is meant to reach (one-tile 128 / 256, persistent kernel with one row range, with two
ranges in ticket or in deterministic order, with fp32 atomics); before a case runs, the dispatch rule restated in helpers_wgrad (as a
function of the problems, M, the tuning hook, the deterministic switch, the VT_WGRAD_* values of this process and the device's CU
count) must name the same one.  Every operand is a view inside a NaN-filled buffer, every output lives in a sentinel-filled buffer;
measured / bound of every check goes through helpers.check_close against 1 (exact constructions, padding and the fingerprint's set
carry the bound 0: any difference is an infinite ratio).  The forms behind non-default values of VT_WGRAD_SPLIT / VT_WGRAD_ORDER /
VT_WGRAD_PERSISTENT_MIN_ROWS run in three fresh child processes (tests/wgrad_conformance_worker.py), one at a time; nothing is
started after a failed one."""
import collections
import os
import subprocess
import sys

import pytest
import torch

import helpers_wgrad as hw
from helpers import check_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _group(case):
    if case.big:
        return "production group"
    if case.reaches in (hw.FORM_128, hw.FORM_256) and case.hook in (128, 256):
        return "%s %s" % (case.reaches, case.data)
    if case.det:
        return "deterministic mode to the one-tile kernel"
    return case.reaches if case.hook == 8 else "automatic below the row threshold"


GROUPS = collections.OrderedDict()
for _c in hw.cases("default"):
    GROUPS.setdefault(_group(_c), []).append(_c)


def _timeouts_check(name):
    from visitron_amd import ops

    check_close("wgrad conformance %s: turn timeouts" % name, 0.0 if ops.wgrad_turn_timeouts() == 0 else hw.INF, 0.0, 1.0)


@pytest.mark.parametrize("group", list(GROUPS))
def test_default_switches(dev, group):
    top, failed, checks = 0.0, [], 0
    for case in GROUPS[group]:
        rs, bad = hw.run_and_judge(case, dev, os.environ)
        failed += bad
        checks += len(rs)
        top = max([top] + [abs(v) for v in rs.values()])
    _timeouts_check(group)
    print("WGRAD-GPU %s: %d cases, %d checks, largest measured / bound %.4f" % (group, len(GROUPS[group]), checks, top))
    assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed[:40]))


def test_deterministic_mode_under_hook_8_is_the_one_tile_kernel_bit_for_bit(dev):
    """M = 2 048, 256 x 256 would take four row ranges: under the deterministic switch hook 8 must launch what hook -8 launches."""
    case = [c for c in hw.cases("default") if c.name == "det M2048 256x256 to the one-tile kernel random"][0]
    assert hw.case_dispatch(case, os.environ, torch.cuda.get_device_properties(dev).multi_processor_count)["form"] == hw.FORM_128
    got = hw.run(case, dev)
    never = hw.Case(case.name, hw.FORM_128, case.why, case.M, case.probs, -8, det=False, data=case.data)
    # (`never` draws the same data: the seed is the name)
    want = hw.run(never, dev)
    for (gw, gb), (ww, wb) in zip(got, want):
        same = torch.equal(gw.view(torch.int32), ww.view(torch.int32)) and torch.equal(gb.view(torch.int32), wb.view(torch.int32))
        check_close("wgrad conformance det hook 8 against hook -8: bitwise", 0.0 if same else hw.INF, 0.0, 1.0)
    _timeouts_check("deterministic hook 8")


def test_twenty_launches_back_to_back(dev):
    """One range, fp32 atomics, fp32 atomics onto dW0, and round again: 20 launches on one stream over the 8 slots with no
    synchronisation between them, each into a dW of its own with integer data; every result exact, no turn ran out of its wait."""
    rs = hw.run_sequence(hw.sequence_cases("default"), dev, os.environ)
    failed = []
    for key in sorted(rs):
        try:
            check_close("wgrad conformance one stream %s" % key, abs(rs[key]), 0.0, 1.0)
        except AssertionError as e:
            failed.append(str(e))
    print("WGRAD-GPU 20 launches back to back: %d checks, largest measured / bound %.4f" % (len(rs), max(abs(v) for v in rs.values())))
    assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed[:40]))


_CHILD_FAILED = []


@pytest.mark.parametrize("family", [f for f in hw.FAMILY_ENV if f != "default"])
def test_switched_forms_in_a_child_process(dev, family):
    assert not _CHILD_FAILED, "not started: the child of %s failed" % _CHILD_FAILED[0]
    _CHILD_FAILED.append(family)                      # (taken back at the end: anything that leaves early counts as failed)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.update(hw.FAMILY_ENV[family])
    cmd = [sys.executable, os.path.join(ROOT, "tests", "wgrad_conformance_worker.py"), family]
    # a failure, abort or time-out fails the test
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=hw.CHILD_TIMEOUT[family])
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    out = r.stdout.splitlines()
    lines = [ln[len("RATIO "):] for ln in out if ln.startswith("RATIO ")]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    cases = [c for c in hw.cases(family) if hw.applicable(c, cus)]
    want = {"%s %s" % (family, c.name) for c in cases} | {"%s turn timeouts after the table" % family}
    n = len(cases)
    if family == "split2":
        for tag, cs in (("one stream", hw.sequence_cases(family)), ("two streams", hw.two_stream_cases())):
            want |= {"%s %s %s" % (family, tag, c.name) for c in cs} | {"%s %s turn timeouts" % (family, tag)}
            n += len(cs)
    assert "DONE %d" % n in out
    seen, top, failed = set(), 0.0, []
    for ln in lines:
        name, ratio = ln.rsplit("\t", 1)
        try:
            check_close("wgrad conformance %s" % name, float(ratio), 0.0, 1.0)
        except AssertionError as e:
            failed.append(str(e))
        seen.add(name.split(": ")[0])
        top = max(top, float(ratio))
    failed += [ln for ln in out if ln.startswith("CENSUS ")]
    assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed[:40]))
    assert seen == want, sorted(seen ^ want)[:10]
    for ln in out:
        if ln.startswith("FINGERPRINT "):
            print("WGRAD-GPU " + ln)
    print("WGRAD-GPU child %s (%s): %d cases, %d checks, largest measured / bound %.4f" % (
        family, " ".join("%s=%s" % kv for kv in sorted(hw.FAMILY_ENV[family].items())), n, len(lines), top))
    _CHILD_FAILED.remove(family)


# ---- host validation: nothing is launched, the library's error is raised, dW / db stay as they were --------------------------------
def _plain(dev, M=64, N=8, K=8, ldy=None, ldx=None, ldw=None, off_y=0, off_w=0):
    ldy, ldx, ldw = ldy or N, ldx or K, ldw or K
    dy = torch.zeros(M * ldy + 16, dtype=torch.bfloat16, device=dev)[off_y:off_y + M * ldy].view(M, ldy)[:, :N]
    x = torch.zeros(M, ldx, dtype=torch.bfloat16, device=dev)[:, :K]
    dwb = torch.full((N * ldw + 16,), hw.SENTINEL, dtype=torch.float32, device=dev)
    dbb = torch.full((N,), hw.SENTINEL, dtype=torch.float32, device=dev)
    return dict(dy=dy, x=x, dw=dwb[off_w:off_w + N * ldw].view(N, ldw)[:, :K], db=dbb), dwb, dbb


@pytest.mark.parametrize("what", ["nprob 0", "nprob 9", "M 0", "K % 4", "ldy % 8", "ldw % 4", "dY base 8 bytes off", "dW base 8 bytes off"])
def test_host_validation(dev, what):
    from visitron_amd import ops

    kw = {"K % 4": dict(K=6, ldx=8, ldw=8), "ldy % 8": dict(ldy=12), "ldw % 4": dict(K=4, ldw=6), "dY base 8 bytes off": dict(off_y=4),
          "dW base 8 bytes off": dict(off_w=2)}.get(what, {})
    built = [_plain(dev, **kw) for _ in range(9 if what == "nprob 9" else 1)]
    problems = [] if what == "nprob 0" else [b[0] for b in built]
    with pytest.raises(RuntimeError, match="visitron_hip vt_wgrad_bf16 failed"):
        ops.wgrad(problems, 0 if what == "M 0" else 64)
    torch.cuda.synchronize(dev)
    for _, dwb, dbb in built:
        assert bool((dwb == hw.SENTINEL).all()) and bool((dbb == hw.SENTINEL).all())
