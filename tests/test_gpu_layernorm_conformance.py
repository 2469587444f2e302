"""The LayerNorm family (csrc/layernorm.hip, fp32_path.hip, fp32_train.hip, ln_deferred.hip) against the float64 reference and the
derived per-element bounds of tests/helpers_layernorm.py, through visitron_amd.ops only.  Alone:
python -m pytest tests/test_gpu_layernorm_conformance.py -m gpu -q -s

Every case of the table names the kernel instantiation it is meant to reach; before a case runs, the dispatch rule restated in
helpers_layernorm (as a function of H, the row remap, gamma's alignment and the switch values of this process) must name the same
one.  Every output lives in a sentinel-filled buffer; measured / bound of every check goes through helpers.check_close against 1
(exact constructions, dropped elements and padding carry the bound 0: any difference is an infinite ratio).  The instantiations
behind non-default values of VT_LN_FWD_ROWS / VT_LN_FWD_BLOCKS / VT_LN_BWD_ROWS run in three fresh child processes
(tests/ln_conformance_worker.py), one at a time; nothing is started after a failed one."""
import collections
import os
import subprocess
import sys

import pytest

import helpers_layernorm as hl
from helpers import check_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _group(case):
    large = case.p["M"] * case.p["H"] > (1 << 20)
    return "%s%s" % (case.reaches.split("<")[0], " large" if large else "")


GROUPS = collections.OrderedDict()
for _c in hl.cases("default"):
    GROUPS.setdefault(_group(_c), []).append(_c)


@pytest.mark.parametrize("group", list(GROUPS))
def test_default_switches(dev, group):
    top, failed = 0.0, []
    for case in GROUPS[group]:
        reached = hl.case_dispatch(case, os.environ)[0]
        assert reached == case.reaches, "%s runs %s, not %s" % (case, reached, case.reaches)
        rs = hl.judge(case, hl.run(case, dev))
        failed += hl.assert_ratios(case.name, rs)
        top = max([top] + [abs(v) for v in rs.values()])
    print("LN-GPU %s: %d cases, largest measured / bound %.3f" % (group, len(GROUPS[group]), top))
    assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed[:40]))


_CHILD_FAILED = []


@pytest.mark.parametrize("family", [f for f in hl.FAMILY_ENV if f != "default"])
def test_switched_instantiations_in_a_child_process(dev, family):
    assert not _CHILD_FAILED, "not started: the child of %s failed" % _CHILD_FAILED[0]
    _CHILD_FAILED.append(family)                      # (taken back at the end: anything that leaves early counts as failed)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.update(hl.FAMILY_ENV[family])
    cmd = [sys.executable, os.path.join(ROOT, "tests", "ln_conformance_worker.py"), family]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)   # a failure, abort or time-out fails the test
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    lines = [ln[len("RATIO "):] for ln in r.stdout.splitlines() if ln.startswith("RATIO ")]
    cases = hl.cases(family)
    assert "DONE %d" % len(cases) in r.stdout.splitlines()
    seen = set()
    top = 0.0
    failed = []
    for ln in lines:
        name, ratio = ln.rsplit("\t", 1)
        try:
            check_close("ln conformance %s" % name, float(ratio), 0.0, 1.0)
        except AssertionError as e:
            failed.append(str(e))
        seen.add(name.split(": ")[0])
        top = max(top, float(ratio))
    assert not failed, "%d check(s) failed:\n%s" % (len(failed), "\n".join(failed[:40]))
    assert seen == {"%s %s" % (family, c.name) for c in cases}
    print("LN-GPU child %s (%s): %d cases, %d checks, largest measured / bound %.3f" % (
        family, " ".join("%s=%s" % kv for kv in sorted(hl.FAMILY_ENV[family].items())), len(cases), len(lines), top))
    _CHILD_FAILED.remove(family)
