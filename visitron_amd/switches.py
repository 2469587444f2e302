"""The environment switches of the package: ``csrc/switches.def`` holds THE list (name, rule, default, reader, one line of
description), the library builds its own table from the same file (``csrc/switches.hpp``), and every read of the environment
in ``visitron_amd/*.py`` is a call of ``on``, ``integer`` or ``text`` below.  The environment is read when the call is made;
a name that is not in the list raises ``KeyError``.
"""
import os
import re

_DEF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "switches.def")
_LINE = re.compile(r'VT_SWITCH\((VT_[A-Z0-9_]+), (NOT0|IS1|INT|NONEMPTY|TEXT), (NONE|"[^"]*"), (PY|LIB|BOTH)\)\s*//\s*(\S.*)')


def _parse_switches(src):
    """The text of csrc/switches.def -> {name: {"rule", "default" (str or None), "reader", "doc"}}; a line is a comment or one entry."""
    table = {}
    for line in src.splitlines():
        line = line.strip()
        if not line or line.startswith("//"):
            continue
        m = _LINE.fullmatch(line)
        if not m or m.group(1) in table:
            raise ImportError("visitron_amd: cannot read `%s` in %s" % (line, _DEF))
        name, rule, default, reader, doc = m.groups()
        if default == "NONE" and rule in ("NOT0", "IS1", "INT"):
            raise ImportError("visitron_amd: rule %s needs a default: `%s` in %s" % (rule, line, _DEF))
        table[name] = {"rule": rule, "default": None if default == "NONE" else default[1:-1], "reader": reader, "doc": doc}
    return table


if not os.path.exists(_DEF):
    raise ImportError("visitron_amd: %s not found: the environment switches are read from it" % _DEF)
SWITCHES = _parse_switches(open(_DEF).read())


def text(name, environ=None):
    """The variable's string; the default (None where the list gives none) when it is unset."""
    return (os.environ if environ is None else environ).get(name, SWITCHES[name]["default"])


def on(name, environ=None):
    """NOT0: anything but "0" is on.  IS1: only "1" is on.  NONEMPTY: set to anything."""
    rule, v = SWITCHES[name]["rule"], text(name, environ)
    if rule not in ("NOT0", "IS1", "NONEMPTY"):
        raise TypeError("%s is %s, not an on / off switch" % (name, rule))
    return v != "0" if rule == "NOT0" else v == "1" if rule == "IS1" else bool(v)


def integer(name, environ=None):
    """INT: int() of the variable's string; garbage raises ValueError."""
    if SWITCHES[name]["rule"] != "INT":
        raise TypeError("%s is %s, not a number" % (name, SWITCHES[name]["rule"]))
    return int(text(name, environ))
