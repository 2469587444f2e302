"""CPU: csrc/gemm_variants.def is the one list of GEMM kernel variants; what visitron_amd.ops derives from it is pinned here
to the literals the module carried before the list existed (candidate order is timing order)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = ("import json, sys; sys.path.insert(0, %r); from visitron_amd import ops; V = ops.GEMM_VARIANTS; print(json.dumps(dict("
        "gemm=ops.GEMM_CANDIDATES, ln=ops.LN_GEMM_CANDIDATES, persistent=ops.PERSISTENT_VARIANTS, shared=ops.SHARED_TILE_VARIANTS, "
        "twins={v: e['twin'] for v, e in V.items() if e['twin'] is not None}, "
        "bf16_only=[v for v, e in V.items() if 'BF16_IO_ONLY' in e['flags']], ids=list(V))))" % ROOT)


@pytest.mark.parametrize("streamk", [None, "1"])
def test_derived_variant_tuples_equal_the_literals(streamk):
    env = {k: v for k, v in os.environ.items() if k != "VT_GEMM_STREAMK"}
    if streamk is not None:
        env["VT_GEMM_STREAMK"] = streamk
    got = json.loads(subprocess.check_output([sys.executable, "-c", DUMP], env=env, cwd=ROOT).decode().splitlines()[-1])
    extra = [31, 32] if streamk == "1" else []
    assert got["gemm"] == [1, 14, 9, 10, 11, 15, 16, 18, 19, 20, 21, 22, 23, 33, 35] + extra
    assert got["ln"] == [15, 16, 18, 19, 20, 21, 22, 23] + extra
    assert got["persistent"] == [16, 18, 19, 20, 21, 28, 29, 30, 31, 32]
    assert got["shared"] == [28, 29, 30, 31, 32, 33]
    assert got["twins"] == {"28": 16, "29": 18, "30": 19, "31": 20, "32": 21}
    assert set(got["bf16_only"]) == {9, 10}
    assert sorted(got["ids"]) == [1, 9, 10, 11, 14, 15, 16] + list(range(18, 34)) + [35]


@pytest.mark.parametrize("line", [
    "VT_GEMM_VARIANT(16, V8, 8, PERSISTENT | SOMETIMES)",          # unknown flag
    "VT_GEMM_VARIANT(16, V8, 8, PERSISTENT)\nVT_GEMM_VARIANT(16, V8, 7, PERSISTENT)",   # a number twice
    "VT_GEMM_VARIANT(16, V8, PERSISTENT)",                         # a field missing
    "VT_GEMM_VARIANT(16, V8, 8, PERSISTENT|LN_EPILOGUE)",          # outside the closed format
    "VT_GEMM_VARIANT(28, V8_SHARED, 8, PLAIN_TWIN(16) | PERSISTENT)",   # the twin is the last flag
    "#define PERSISTENT 1",
    "int x;",
])
def test_malformed_variant_lines_raise(line):
    from visitron_amd import ops

    assert list(ops._parse_variants("// ok\nVT_GEMM_VARIANT(1, V2_RING2, 0, 0)   // plain\n")) == [1]
    with pytest.raises(ImportError):
        ops._parse_variants(line)
