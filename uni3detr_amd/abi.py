"""The C ABI of libu3d_hip.so, read from include/u3d_hip.h: the one description native.py binds from.

Standard library only.  The header is regular; whatever this reader cannot digest is an error, never a
guess - reformat an awkward declaration in the header rather than teach the reader more C.
  prototypes  name -> (restype, [argtypes]) in ctypes terms: int32_t / int64_t / float / u3d_stream by value, every parameter with
              `*` or `[` a c_void_p, `const char*` returned as c_char_p
  constants   every `#define U3D_X <integer>` and every enumerator of every `enum { ... }`
  structs     name -> [(field, kind, array length or None)], kind one of int32_t / int64_t / float / pointer
"""
import collections
import ctypes as C
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "u3d_hip.h")
BY_VALUE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "u3d_stream": C.c_void_p}
FIELD = {"int32_t": (C.c_int32, "<i4"), "int64_t": (C.c_int64, "<i8"), "float": (C.c_float, "<f4"), "pointer": (C.c_void_p, "<u8")}
Abi = collections.namedtuple("Abi", "prototypes constants structs")
_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"


class AbiError(ValueError):
    pass


def _param(name, text):
    if "*" in text or "[" in text:
        return C.c_void_p
    words = [w for w in text.split() if w != "const"]
    if not 1 <= len(words) <= 2 or words[0] not in BY_VALUE:
        raise AbiError(f"{name}: parameter `{text.strip()}` is passed by value with a type outside {sorted(BY_VALUE)}")
    return BY_VALUE[words[0]]


def _fields(struct, body, constants):
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)", decl, re.S)
        kind = "pointer" if m and m.group(2) else m.group(1) if m else None
        names = [d.strip() for d in m.group(3).split(",")] if m else []
        if kind not in FIELD or (kind == "pointer" and len(names) > 1):
            raise AbiError(f"struct {struct}: cannot read the field declaration `{decl}`")
        for d in names:
            dm = re.fullmatch(r"(\w+)(?:\s*\[\s*(\w+)\s*\])?", d)
            if not dm:
                raise AbiError(f"struct {struct}: cannot read the declarator `{d}`")
            n = dm.group(2)
            if n is not None and not n.isdigit() and n not in constants:
                raise AbiError(f"struct {struct}: the array length of `{d}` is neither a number nor a known constant")
            out.append((dm.group(1), kind, None if n is None else int(n) if n.isdigit() else constants[n]))
    return out


def parse(text):
    """-> Abi(prototypes, constants, structs) of a header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(" + _INT + r")[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    for body in re.findall(r"\benum\s*\w*\s*\{([^}]*)\}", text):
        value = -1
        for entry in filter(None, (e.strip() for e in body.split(","))):
            m = re.fullmatch(r"(\w+)(?:\s*=\s*(" + _INT + r"))?", entry)
            if not m:
                raise AbiError(f"cannot read the enumerator `{entry}`")
            value = value + 1 if m.group(2) is None else int(m.group(2), 0)
            constants[m.group(1)] = value
    structs = {name: _fields(name, body, constants)
               for body, name in re.findall(r"\btypedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", text)}
    prototypes = {}
    for ret, name, params in re.findall(r"^[ \t]*([\w \t*]+?)[ \t]*\b(u3d_[a-z0-9_]+)\(([^()]*)\)\s*;", text, re.M):
        if name in prototypes:
            raise AbiError(f"{name} is declared twice")
        ret = " ".join(ret.replace("*", " * ").split())
        if ret != "const char *" and ret not in BY_VALUE:
            raise AbiError(f"{name}: return type `{ret}` is outside {sorted(BY_VALUE)} and const char*")
        args = [] if params.strip() == "void" else [_param(name, p) for p in params.split(",")]
        prototypes[name] = (C.c_char_p if ret == "const char *" else BY_VALUE[ret], args)
    calls = len(re.findall(r"u3d_[a-z0-9_]+\(", text))
    if calls != len(prototypes):
        raise AbiError(f"{calls} occurrences of `u3d_...(` but {len(prototypes)} prototypes read: a declaration is in a form this "
                       "reader does not take (see the module docstring)")
    return Abi(prototypes, constants, structs)


@functools.lru_cache(maxsize=None)
def load():
    """The ABI of include/u3d_hip.h, parsed once per process."""
    if not os.path.exists(HEADER):
        raise FileNotFoundError(f"{HEADER} is missing: the ctypes binding is derived from it")
    with open(HEADER) as f:
        return parse(f.read())


def structure(fields, name):
    """A ctypes.Structure subclass called `name` with the layout of a parsed struct."""
    return type(name, (C.Structure,), {"_fields_": [(f, FIELD[k][0] if n is None else FIELD[k][0] * n) for f, k, n in fields]})


def numpy_dtype(fields):
    """The numpy structured dtype of a parsed struct (natural alignment: the padding a C compiler inserts)."""
    import numpy as np
    return np.dtype([(f, FIELD[k][1]) if n is None else (f, FIELD[k][1], (n,)) for f, k, n in fields], align=True)
