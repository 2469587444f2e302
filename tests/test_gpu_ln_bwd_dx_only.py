"""GPU: the LayerNorm backward's dx-only form (no parameter gradients: a frozen LayerNorm) is bit for bit the full kernel's dx,
writes no partial row and reduces nothing -- in every instantiation vt_layernorm_bwd_dispatch can reach: the chunked kernel
(H = 128; every H under VT_LN_BWD_ROWS=0) and the row kernels at H = 256 / 768 with 1 (this process), 2 and 4 rows per wave
(fresh child processes, tests/ln_dx_only_worker.py: the switch is read once per process), x as bf16 and as fp16."""
import os
import subprocess
import sys

import pytest

import ln_dx_only_worker as worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", worker.CASES, ids=worker.case_name)
def test_dx_only_is_the_full_kernels_dx(dev, case):
    assert os.environ.get("VT_LN_BWD_ROWS", "1") == "1"   # the default: one row per wave
    bad = worker.run_case(case, dev)
    assert not bad, "%s: %s" % (worker.case_name(case), "; ".join(bad))


def test_dx_only_needs_no_workspace_and_refuses_half_a_request(dev):
    from visitron_amd import ops
    import torch

    worker.run_without_workspace(dev)
    x = torch.zeros(4, 128, dtype=ops.BF16, device=dev)
    with pytest.raises(ValueError, match="dgamma and dbeta together, or neither"):
        ops.layernorm_bwd(x, x, torch.ones(128, device=dev), 1e-12, torch.zeros(128, device=dev), None)


_CHILD_FAILED = []


@pytest.mark.parametrize("rows", ["0", "2", "4"])
def test_dx_only_under_the_other_rows_per_wave(dev, rows):
    assert not _CHILD_FAILED, "not started: the child with VT_LN_BWD_ROWS=%s failed" % _CHILD_FAILED[0]
    _CHILD_FAILED.append(rows)                      # (taken back at the end: anything that leaves early counts as failed)
    env = dict(os.environ, PYTHONPATH=ROOT, VT_LN_BWD_ROWS=rows)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "ln_dx_only_worker.py"), rows]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)   # a failure, abort or time-out fails the test
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-6000:]
    lines = r.stdout.splitlines()
    assert "DONE %d" % len(worker.CASES) in lines
    assert [ln for ln in lines if ln.startswith("SAME ")] == ["SAME " + worker.case_name(c) for c in worker.CASES]
    _CHILD_FAILED.remove(rows)
