"""CPU: csrc/switches.def is the one list of environment switches.  What visitron_amd.switches (Python) and csrc/switches.hpp
(the library) read from it is pinned here to the expressions and defaults every site carried before the list existed; and the
three rules that live in both languages (dropout sites, keep-word count, the autotuner's key) are pinned to each other."""
import itertools
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "visitron_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
RAW = [None, "", "0", "1", "2", "8", "-1", " 1", "abc"]   # None: unset


def _env(name, raw):
    return {} if raw is None else {name: raw}


# ---- Python side -----------------------------------------------------------------------------------------------------------
def _legacy():
    """name -> (the expression the site carried, over a mapping e; the site's expression now, over the same mapping)."""
    from visitron_amd import switches as sw

    on, integer, text = sw.on, sw.integer, sw.text
    return {
        "VT_HIP_LIB": (lambda e: e.get("VT_HIP_LIB", "<in-tree>"),
                       lambda e: "<in-tree>" if text("VT_HIP_LIB", e) is None else text("VT_HIP_LIB", e)),
        "VT_SYNC_ERRORS": (lambda e: e.get("VT_SYNC_ERRORS") == "1", lambda e: on("VT_SYNC_ERRORS", e)),
        "VT_AUTOTUNE": (lambda e: e.get("VT_AUTOTUNE", "1") == "0", lambda e: not on("VT_AUTOTUNE", e)),
        "VT_TUNE_FILE": (lambda e: e.get("VT_TUNE_FILE"), lambda e: text("VT_TUNE_FILE", e)),
        "VT_TUNE_VERBOSE": (lambda e: bool(e.get("VT_TUNE_VERBOSE")), lambda e: on("VT_TUNE_VERBOSE", e)),
        "VT_TUNE_BUCKET_SMALL": (lambda e: int(e.get("VT_TUNE_BUCKET_SMALL", "512")), lambda e: integer("VT_TUNE_BUCKET_SMALL", e)),
        "VT_TUNE_BUCKET_LARGE": (lambda e: int(e.get("VT_TUNE_BUCKET_LARGE", "256")), lambda e: integer("VT_TUNE_BUCKET_LARGE", e)),
        "VT_GEMM_STREAMK": (lambda e: e.get("VT_GEMM_STREAMK", "0") == "1", lambda e: on("VT_GEMM_STREAMK", e)),
        "VT_GEMM_TAIL_SPLIT": (lambda e: -2 if e.get("VT_GEMM_TAIL_SPLIT") == "1" else -1,
                               lambda e: -2 if on("VT_GEMM_TAIL_SPLIT", e) else -1),
        "VT_GEMM_WS_REGIONS": (lambda e: int(e.get("VT_GEMM_WS_REGIONS", "2")), lambda e: integer("VT_GEMM_WS_REGIONS", e)),
        "VT_SPLITK": (lambda e: e.get("VT_SPLITK", "1") == "0", lambda e: not on("VT_SPLITK", e)),
        "VT_GEMM_RESERVE_CUS": (lambda e: e.get("VT_GEMM_RESERVE_CUS"), lambda e: text("VT_GEMM_RESERVE_CUS", environ=e)),
        "VT_FORCE_MULTI_RANK_GEMM": (lambda e: e.get("VT_FORCE_MULTI_RANK_GEMM") == "1", lambda e: on("VT_FORCE_MULTI_RANK_GEMM", e)),
        "VT_F16_STREAM": (lambda e: e.get("VT_F16_STREAM", "1") != "0", lambda e: on("VT_F16_STREAM", e)),
        "VT_LN_RESIDUAL": (lambda e: e.get("VT_LN_RESIDUAL", "1") != "0", lambda e: on("VT_LN_RESIDUAL", e)),
        "VT_DEFERRED_LN": (lambda e: e.get("VT_DEFERRED_LN", "1") != "0", lambda e: on("VT_DEFERRED_LN", e)),
        "VT_DEFERRED_LN_MIN_ROWS": (lambda e: int(e.get("VT_DEFERRED_LN_MIN_ROWS", 2800)), lambda e: integer("VT_DEFERRED_LN_MIN_ROWS", e)),
        "VT_PRECISE_FINAL": (lambda e: e.get("VT_PRECISE_FINAL", "0") == "1", lambda e: on("VT_PRECISE_FINAL", e)),
        "VT_ATTN_DROPOUT_BITS": (lambda e: 8 if e.get("VT_ATTN_DROPOUT_BITS") == "8" else 16,
                                 lambda e: 8 if text("VT_ATTN_DROPOUT_BITS", e) == "8" else 16),
        "VT_ATTN_KEEP_BITS": (lambda e: e.get("VT_ATTN_KEEP_BITS", "1") != "0", lambda e: on("VT_ATTN_KEEP_BITS", e)),
        "VT_GRAD_COMM": (lambda e: e.get("VT_GRAD_COMM", "bf16"), lambda e: text("VT_GRAD_COMM", e)),
        "VT_OVERLAP_WGRAD": (lambda e: e.get("VT_OVERLAP_WGRAD", "0") != "0", lambda e: on("VT_OVERLAP_WGRAD", e)),
        "VT_OVERLAP_ADAMW": (lambda e: e.get("VT_OVERLAP_ADAMW", "0") != "0", lambda e: on("VT_OVERLAP_ADAMW", e)),
        "VT_COMPACT_ROWS": (lambda e: e.get("VT_COMPACT_ROWS", "1") != "0", lambda e: on("VT_COMPACT_ROWS", e)),
        "VT_COMPACT_MIN_ROWS": (lambda e: int(e.get("VT_COMPACT_MIN_ROWS", "0")), lambda e: integer("VT_COMPACT_MIN_ROWS", e)),
        "VT_STEP_OVERLAP_READBACK": (lambda e: e.get("VT_STEP_OVERLAP_READBACK", "1") == "0", lambda e: not on("VT_STEP_OVERLAP_READBACK", e)),
        "VT_LSTM_PERSISTENT": (lambda e: e.get("VT_LSTM_PERSISTENT", "1") != "0", lambda e: on("VT_LSTM_PERSISTENT", e)),
        "VT_DECODER_GRAPH": (lambda e: e.get("VT_DECODER_GRAPH", "0") == "1", lambda e: on("VT_DECODER_GRAPH", e)),
    }


def _outcome(fn, env):
    try:
        return fn(env)
    except Exception as exc:   # noqa: BLE001 -- the exception's type is the outcome
        return type(exc)


def test_python_readers_keep_the_legacy_semantics(monkeypatch):
    from visitron_amd import switches

    legacy = _legacy()
    assert set(legacy) == {n for n, s in switches.SWITCHES.items() if s["reader"] in ("PY", "BOTH")}
    for name, (old, new) in legacy.items():
        for raw in RAW:
            want = _outcome(old, _env(name, raw))
            assert _outcome(new, _env(name, raw)) == want, (name, raw)
            # without environ= the process environment is read, when the call is made
            monkeypatch.delenv(name, raising=False)
            if raw is not None:
                monkeypatch.setenv(name, raw)
            assert _outcome(lambda e: new(None), None) == want, (name, raw)
        monkeypatch.delenv(name, raising=False)
    assert _outcome(legacy["VT_COMPACT_MIN_ROWS"][0], {"VT_COMPACT_MIN_ROWS": "abc"}) is ValueError
    for reader in (switches.on, switches.integer, switches.text):
        with pytest.raises(KeyError):
            reader("VT_COMPACT_ROW")           # a misspelt name is refused, not ignored
    with pytest.raises(TypeError):
        switches.on("VT_COMPACT_MIN_ROWS")
    with pytest.raises(TypeError):
        switches.integer("VT_COMPACT_ROWS")


def test_module_constants_keep_their_names_and_values():
    code = ("import json, sys; sys.path.insert(0, %r); from visitron_amd import _lib, ops, training; print(json.dumps(["
            "ops.F16_STREAM, ops.LN_RESIDUAL, ops.STREAMK, ops.AUTO_VARIANT, ops.LSTM_PERSISTENT, training.KEEP_BITS, _lib.LIB_PATH]))" % ROOT)
    names = ("VT_F16_STREAM", "VT_LN_RESIDUAL", "VT_GEMM_STREAMK", "VT_GEMM_TAIL_SPLIT", "VT_LSTM_PERSISTENT", "VT_ATTN_KEEP_BITS", "VT_HIP_LIB")
    base = {k: v for k, v in os.environ.items() if k not in names}
    run = lambda env: json.loads(subprocess.check_output([sys.executable, "-c", code], env=dict(base, **env), cwd=ROOT).decode().splitlines()[-1])
    in_tree = os.path.join(PKG, "lib", "libvisitron_hip.so")
    assert run({}) == [True, True, False, -1, True, True, in_tree]
    assert run({n: "0" for n in names}) == [False, False, False, -1, False, False, "0"]
    assert run({n: "1" for n in names}) == [True, True, True, -2, True, True, "1"]
    assert run({"VT_F16_STREAM": "0"}) == [False, False, False, -1, True, True, in_tree]     # LN_RESIDUAL needs the fp16 stream


# ---- library side ----------------------------------------------------------------------------------------------------------
# the defaults the sites hard-coded before the list existed
LIB_DEFAULTS = {"VT_WGRAD_PERSISTENT_MIN_ROWS": 12288, "VT_WGRAD_SPLIT": 0, "VT_WGRAD_ORDER": 1,
                "VT_LN_FWD_ROWS": 2, "VT_LN_FWD_BLOCKS": 1024, "VT_LN_BWD_ROWS": 1,
                "VT_GEMM_SK": 2, "VT_GEMM_REVERSE_K": 0,
                "VT_PREFETCH_INFER": 3, "VT_PREFETCH_WEIGHTS": 4, "VT_PREFETCH_MAX_ROWS": 16384,
                "VT_ATTN_DROPOUT_BITS": 16}   # capi.hip: (e && atoi(e) == 8) ? 8 : 16 -- 16 is any value that is not 8


def _atol(s):
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", s)
    return int(m.group(1)) if m else 0


def _host_program(tmp, name, body):
    src = tmp / (name + ".cpp")
    src.write_text(body)
    exe = str(tmp / name)
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def switch_dump(tmp_path_factory):
    return _host_program(tmp_path_factory.mktemp("switches"), "switch_dump", """
#include <stdio.h>
#include "switches.hpp"
int main() {
  for (unsigned i = 0; i < sizeof(SWITCH_TABLE) / sizeof(SWITCH_TABLE[0]); ++i) printf("%s %ld\\n", SWITCH_TABLE[i].name, vt_switch((Switch)i));
  return 0;
}
""")


def test_library_reader_keeps_atol_and_the_hard_coded_defaults(switch_dump):
    from visitron_amd import switches

    assert set(LIB_DEFAULTS) == {n for n, s in switches.SWITCHES.items() if s["reader"] in ("LIB", "BOTH")}
    base = {k: v for k, v in os.environ.items() if k not in LIB_DEFAULTS}
    for raw in RAW:
        env = dict(base) if raw is None else dict(base, **{n: raw for n in LIB_DEFAULTS})
        out = subprocess.check_output([switch_dump], env=env).decode().split()
        got = dict(zip(out[0::2], map(int, out[1::2])))
        assert got == {n: d if raw is None else _atol(raw) for n, d in LIB_DEFAULTS.items()}, raw


def test_library_reads_its_switches_without_a_gpu():
    code = ("import sys; sys.path.insert(0, %r); from visitron_amd import _lib; lib = _lib.load(); "
            "print(lib.vt_get_attn_dropout_bits(), lib.vt_get_weight_prefetch(0), lib.vt_get_weight_prefetch(1))" % ROOT)
    names = ("VT_ATTN_DROPOUT_BITS", "VT_PREFETCH_WEIGHTS", "VT_PREFETCH_INFER", "VT_PREFETCH_MAX_ROWS", "VT_HIP_LIB")
    base = {k: v for k, v in os.environ.items() if k not in names}
    run = lambda env: subprocess.check_output([sys.executable, "-c", code], env=dict(base, **env), cwd=ROOT).decode().split()[-3:]
    assert run({}) == ["16", "4", "3"]
    assert run({"VT_ATTN_DROPOUT_BITS": "8", "VT_PREFETCH_WEIGHTS": "0", "VT_PREFETCH_INFER": "0"}) == ["8", "0", "0"]
    assert run({"VT_ATTN_DROPOUT_BITS": " 8"}) == ["8", "4", "3"] and run({"VT_ATTN_DROPOUT_BITS": "abc"}) == ["16", "4", "3"]


# ---- completeness ----------------------------------------------------------------------------------------------------------
def _package_sources():
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".inc", ".def", ".h")):
                yield os.path.join(d, f), open(os.path.join(d, f)).read()


def test_every_read_goes_through_the_list_and_every_switch_is_read():
    from visitron_amd import switches

    sources = dict(_package_sources())
    for path, src in sources.items():
        if os.path.basename(path) not in ("switches.py", "switches.hpp"):
            assert "os.environ" not in src and "getenv(" not in src, path
    readers = "\n".join(src for path, src in sources.items() if os.path.basename(path) not in ("switches.def", "switches.py", "switches.hpp"))
    py = "\n".join(src for path, src in sources.items() if path.endswith(".py") and not path.endswith("switches.py"))
    lib = "\n".join(src for path, src in sources.items() if path.endswith((".hip", ".hpp", ".inc")) and not path.endswith("switches.hpp"))
    for name, s in switches.SWITCHES.items():
        if s["reader"] in ("PY", "BOTH"):
            assert re.search(r'switches\.(on|integer|text)\([^)]*"%s"' % name, py), name
        if s["reader"] in ("LIB", "BOTH"):
            assert "vt_switch(%s)" % name in lib, name
    # and no read names a switch that is not listed (the Python readers raise KeyError; the library's would not compile)
    for name in re.findall(r'switches\.(?:on|integer|text)\([^)]*?"(VT_\w+)"', readers):
        assert name in switches.SWITCHES, name


def test_integration_md_lists_exactly_the_switches():
    from visitron_amd import switches

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index("## 6. Environment switches"):]
    section = section[:section.index("\n## ", 4)]
    rows = re.findall(r"^\| `(VT_\w+)` \| (.*?) \| (\w+) \| (.*) \|$", section, flags=re.M)
    assert [r[0] for r in rows] == list(switches.SWITCHES)                  # the file's order, each once, nothing else
    assert set(re.findall(r"\bVT_[A-Z0-9_]+\b", section)) == set(switches.SWITCHES)
    for name, default, reader, doc_line in rows:
        s = switches.SWITCHES[name]
        assert default == ("unset" if s["default"] is None else "`%s`" % s["default"]), name
        assert reader == {"PY": "Python", "LIB": "library", "BOTH": "both"}[s["reader"]], name
        assert doc_line == s["doc"].replace("|", "\\|"), name


@pytest.mark.parametrize("src", [
    'VT_SWITCH(VT_X, MAYBE, "1", PY)   // unknown rule',
    'VT_SWITCH(VT_X, NOT0, "1", PY)   // a name twice\nVT_SWITCH(VT_X, NOT0, "1", PY)   // a name twice',
    'VT_SWITCH(VT_X, NOT0, "1")   // a field missing',
    'VT_SWITCH(VT_X, NOT0, 1, PY)   // the default is text',
    'VT_SWITCH(VT_X, NOT0, "1", PY)',                         # no description
    'VT_SWITCH(VT_X, NOT0, "1", GPU)   // unknown reader',
    'VT_SWITCH(VT_X, INT, NONE, PY)   // a number without a default',
    'VT_SWITCH(X, NOT0, "1", PY)   // not a VT_ name',
    'VT_SWITCH(VT_X,NOT0,"1",PY)   // outside the closed format',
    "#define VT_X 1",
    "int x;",
])
def test_malformed_switch_lines_raise(src):
    from visitron_amd import switches

    ok = switches._parse_switches('// ok\n\nVT_SWITCH(VT_X, NOT0, "1", PY)   // fine\nVT_SWITCH(VT_Y, TEXT, NONE, LIB)   // fine too\n')
    assert ok == {"VT_X": {"rule": "NOT0", "default": "1", "reader": "PY", "doc": "fine"},
                  "VT_Y": {"rule": "TEXT", "default": None, "reader": "LIB", "doc": "fine too"}}
    with pytest.raises(ImportError):
        switches._parse_switches(src)


# ---- the three rules written in both languages -----------------------------------------------------------------------------
LAYERS = (0, 1, 11, 63)
SHAPES = list(itertools.product((1, 3), (1, 12), (1, 31, 32, 33, 767)))
KINDS = list(itertools.product(range(4), (0, 1), (0, 1), (0, 1), range(3)))   # act, residual, pre_act, out_f32, ln_mode


@pytest.fixture(scope="module")
def rules_dump(tmp_path_factory):
    return _host_program(tmp_path_factory.mktemp("rules"), "rules_dump", """
#include <stdio.h>
#include "visitron_hip.h"
int main() {
  const int layers[] = {%s}, Bs[] = {1, 3}, nhs[] = {1, 12}, Ss[] = {1, 31, 32, 33, 767};
  printf("emb %%u img %%u\\n", VT_SITE_EMB, VT_SITE_IMG);
  for (int l : layers) printf("site %%d %%u %%u %%u\\n", l, VT_SITE_ATTN(l), VT_SITE_SELFOUT(l), VT_SITE_OUT(l));
  for (int B : Bs) for (int nh : nhs) for (int S : Ss) printf("keep %%d %%d %%d %%lld\\n", B, nh, S, (long long)VT_KEEP_WORDS(B, nh, S));
  for (int act = 0; act < 4; ++act) for (int r = 0; r < 2; ++r) for (int c2 = 0; c2 < 2; ++c2) for (int f = 0; f < 2; ++f)
    for (int ln = 0; ln < 3; ++ln) printf("kind %%d %%d %%d %%d %%d %%d\\n", act, r, c2, f, ln, VT_TUNE_KIND(act, r, c2, f, ln));
  return 0;
}
""" % ", ".join(map(str, LAYERS)))


def test_header_macros_equal_the_python_rules(rules_dump):
    from visitron_amd import ops

    lines = [l.split() for l in subprocess.check_output([rules_dump]).decode().splitlines()]
    assert lines[0] == ["emb", str(ops.SITE_EMB), "img", str(ops.SITE_IMG)] and (ops.SITE_EMB, ops.SITE_IMG) == (0xE0, 0xE1)
    sites = {int(l[1]): tuple(map(int, l[2:])) for l in lines if l[0] == "site"}
    assert sites == {l: (ops.site_attn(l), ops.site_selfout(l), ops.site_out(l)) for l in LAYERS}
    assert sites[11] == (88, 89, 90)
    keep = {tuple(map(int, l[1:4])): int(l[4]) for l in lines if l[0] == "keep"}
    assert keep == {(B, nh, S): ops.keep_words(B, nh, S) for B, nh, S in SHAPES} and len(keep) == 20
    assert keep[(3, 12, 767)] == 3 * 12 * 24 * 768
    kinds = {tuple(map(int, l[1:6])): int(l[6]) for l in lines if l[0] == "kind"}
    assert kinds == {k: ops.tune_kind(k[0], residual=bool(k[1]), pre_act=bool(k[2]), out_f32=bool(k[3]), ln_mode=k[4]) for k in KINDS}
    assert len(kinds) == 96
    # ACT_MUL's factor operand counts as a residual whether or not the caller says so, in both languages
    assert kinds[(ops.ACT_MUL, 0, 0, 0, 0)] == kinds[(ops.ACT_MUL, 1, 0, 0, 0)] == 3 + 16 == ops.tune_kind(ops.ACT_MUL)
    assert kinds[(ops.ACT_GELU, 0, 0, 0, 0)] == 1 and kinds[(ops.ACT_GELU, 1, 0, 0, 0)] == 1 + 16
