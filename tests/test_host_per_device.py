"""CPU: csrc/per_device.hpp, the one store of per-device host state, raced under ThreadSanitizer by a stand-alone host program
(tests/host/per_device_tsan.cpp): one construction per device index, null outside the range, no data race."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visitron_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang++ beside the HIP compiler")
def test_per_device_store_builds_each_slot_once_under_tsan(tmp_path):
    exe = str(tmp_path / "per_device_tsan")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "per_device_tsan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, timeout=600, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"))
    out = run.stdout.decode() + run.stderr.decode()
    assert run.returncode == 0 and "ThreadSanitizer" not in out, out
    assert out.split()[:4] == ["built", "4", "bad", "0"], out
