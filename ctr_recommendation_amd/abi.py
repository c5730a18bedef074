"""include/fibinet.h read as data: the prototypes of the entry points and the integer constants.

The header is the only statement of the C ABI.  The native sources include it, so the compiler
checks every definition against it; the Python side reads it here -- _lib.SIGNATURES (the ctypes
argument types) and the FBN_* constants are derived from it at import, nothing is typed twice.
"""
from __future__ import annotations

import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fibinet.h")


def _code(src: str) -> str:
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def _type(text: str) -> str:
    """A type as one spelling: single spaces, every '*' attached ("const float*", "float* const*")."""
    return " ".join(text.replace("*", " * ").split()).replace(" *", "*")


def declarations(src: str):
    """[(name, return type, [parameter type, ...])] of the fbn_* entry points, sorted by name."""
    src = "\n".join(ln for ln in _code(src).splitlines() if not ln.lstrip().startswith("#"))
    out = []
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(fbn_\w+)\s*\(([^()]*)\)\s*;", src):
        name, params = m.group(2), " ".join(m.group(3).split())
        args = []
        if params and params != "void":
            for p in params.split(","):
                pm = re.match(r"^(.*?)([A-Za-z_]\w*)$", p.strip())
                if pm is None or not pm.group(1).strip():       # every parameter is "<type> <name>"
                    raise ValueError(f"{name}: cannot parse parameter {p.strip()!r}")
                args.append(_type(pm.group(1)))
        out.append((name, _type(m.group(1)), args))
    if len({n for n, _, _ in out}) != len(out):
        raise ValueError("duplicate declarations in fibinet.h")
    return sorted(out)


def constants(src: str) -> dict:
    """{name: value} of every ``#define FBN_X <integer literal>``."""
    return {m.group(1): int(m.group(2), 0)
            for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(FBN_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[ \t]*$",
                                 _code(src), flags=re.M)}


def read_header():
    """(declarations, constants) of include/fibinet.h."""
    src = open(HEADER).read()
    return declarations(src), constants(src)
