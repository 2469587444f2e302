"""ctypes binding of ``libvisitron_hip.so`` (the C ABI in ``include/visitron_hip.h``).

There is NO fallback: if the shared library is missing this module raises, and every
op in ``visitron_amd.ops`` refuses tensors that are not on a HIP device.
"""
import ctypes
import os
import re

from . import switches

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = switches.text("VT_HIP_LIB")   # A/B builds of the kernels (tools/): same ABI, other path
if LIB_PATH is None:
    LIB_PATH = os.path.join(_HERE, "lib", "libvisitron_hip.so")

# ---- the binding is read from the header: one declaration per entry point, struct and constant, in include/visitron_hip.h ----
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "visitron_hip.h")

# C struct -> name of the ctypes.Structure mirroring it (module attributes, set below)
_STRUCTS = {"vt_layer_weights": "LayerWeights", "vt_layer_acts": "LayerActs", "vt_layer_weights_ln": "LayerWeightsLn",
            "vt_layer_weights_t": "LayerWeightsT", "vt_layer_grads": "LayerGrads", "vt_bwd_workspace": "BwdWorkspace",
            "vt_wgrad_problem": "WgradProblem"}
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "uint32_t": ctypes.c_uint32, "float": ctypes.c_float, "vt_stream_t": ctypes.c_void_p}
_POINTEES = ("void", "float", "int", "int32_t", "int64_t", "uint8_t", "uint16_t", "uint32_t", "uint64_t")  # data: c_void_p
_classes = {}   # C struct name -> Structure class, filled by _parse_header
# `#define VT_NAME <integer>` / `(-<integer>)` is a constant; any other #define must be one of these: the include guard, the
# function-like macros (Python keeps its own ops.keep_words / site_* / tune_kind) and the two unsigned site numbers beside them
_MACROS = ("VISITRON_HIP_H", "VT_KEEP_WORDS_RECT", "VT_KEEP_WORDS","VT_SITE_ATTN", "VT_SITE_SELFOUT", "VT_SITE_OUT", "VT_SITE_EMB", "VT_SITE_IMG", "VT_TUNE_KIND")
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+(?:\s*,\s*\w+)*)")   # [const] base [*...] name[, name]


def _ctype(base, stars, what):
    """The closed type rule; anything outside it raises with the declaration's text."""
    stars = stars.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base in _classes:
        return ctypes.POINTER(_classes[base])
    if stars == 1 and base == "unsigned":
        return ctypes.POINTER(ctypes.c_uint)
    if stars >= 1 and base in _POINTEES:
        return ctypes.c_void_p
    raise ImportError("visitron_amd: no ctypes rule for `%s` in %s" % (" ".join(what.split()), _HEADER))


def _parse_header():
    """include/visitron_hip.h -> _classes (the seven Structure classes), {name: (restype, argtypes)} and {VT_NAME: integer}."""
    if not os.path.exists(_HEADER):
        raise ImportError("visitron_amd: %s not found: the ctypes binding is derived from it" % _HEADER)
    src = open(_HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"#ifdef __cplusplus.*?#endif", " ", src, flags=re.S)   # the extern "C" braces
    constants = {}
    for define in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(.*?)[ \t]*$", src, flags=re.M):
        c = re.fullmatch(r"(VT_\w+)[ \t]+(\d+|\(-\d+\))", define)
        if c and c.group(1) not in constants:
            constants[c.group(1)] = int(c.group(2).strip("()"))
        elif c or not re.match(r"(%s)\b" % "|".join(_MACROS), define):
            raise ImportError("visitron_amd: cannot read `#define %s` in %s" % (define, _HEADER))
    src = re.sub(r"^[ \t]*#.*$", " ", src, flags=re.M)

    def struct(m):
        if m.group(1) != m.group(3) or m.group(1) not in _STRUCTS:
            raise ImportError("visitron_amd: struct %s of %s has no ctypes mirror" % (m.group(1), _HEADER))
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            f = _DECL.fullmatch(decl)
            if not f or ("," in f.group(3) and f.group(2)):
                raise ImportError("visitron_amd: cannot read field `%s` of %s in %s" % (decl, m.group(1), _HEADER))
            fields += [(n.strip(), _ctype(f.group(1), f.group(2), decl)) for n in f.group(3).split(",")]
        _classes[m.group(1)] = type(_STRUCTS[m.group(1)], (ctypes.Structure,), {"_fields_": fields})
        return " "

    src = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, src, flags=re.S)
    if len(_classes) != len(_STRUCTS):
        raise ImportError("visitron_amd: %s does not define %s" % (_HEADER, ", ".join(sorted(set(_STRUCTS) - set(_classes)))))
    signatures = {}
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        if stmt == "typedef void* vt_stream_t":
            continue
        p = re.fullmatch(r"(const\s+char\s*\*|\w+)\s*(vt_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not p or p.group(2) in signatures:
            raise ImportError("visitron_amd: cannot read `%s` in %s" % (" ".join(stmt.split()), _HEADER))
        ret, name, params = p.groups()
        if ret.startswith("const"):
            restype = ctypes.c_char_p
        else:
            restype = None if ret == "void" else _ctype(ret, "", stmt)
        argtypes = []
        if params.strip() != "void":
            for param in params.split(","):
                a = _DECL.fullmatch(param.strip())
                if not a or "," in a.group(3):
                    raise ImportError("visitron_amd: cannot read `%s` in %s" % (" ".join(stmt.split()), _HEADER))
                argtypes.append(_ctype(a.group(1), a.group(2), stmt))
        signatures[name] = (restype, argtypes)
    return signatures, constants


# name -> (restype, argtypes) of every entry point the header declares; VT_NAME -> value of every integer constant
SIGNATURES, CONSTANTS = _parse_header()
VT_OK, VT_ERR_BAD_SHAPE, VT_ERR_BAD_ALIGN, VT_ERR_NULL, VT_ERR_UNSUPPORTED, VT_ERR_HIP = (
    CONSTANTS[c] for c in ("VT_OK", "VT_ERR_BAD_SHAPE", "VT_ERR_BAD_ALIGN", "VT_ERR_NULL", "VT_ERR_UNSUPPORTED", "VT_ERR_HIP"))
# LayerWeights, LayerActs, LayerWeightsLn, LayerWeightsT, LayerGrads, BwdWorkspace, WgradProblem
globals().update({_STRUCTS[c]: cls for c, cls in _classes.items()})

_lib = None


def load():
    """Load the library once; raise with build instructions if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "visitron_amd: %s not found. Build it first: `make -C visitron_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback." % LIB_PATH
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().vt_error_string(int(rc)).decode()
        raise RuntimeError("visitron_hip %s failed: %s (code %d)" % (what, msg, rc))
