"""The C ABI as the binding sees it, read from include/fastvocoder_hip.h: the header is the one place that declares an
entry's parameters and a constant's value.  prototypes() gives name -> (restype, [argtypes]) for every fv_* function,
constants() name -> int for every `#define FV_NAME <integer literal>`.

Scalars map by the table below and anything else raises: a width is never guessed.  `const char*` is c_char_p, every other
pointer (at any depth, arrays included) c_void_p: the header cannot tell host memory from device or mapped memory, so the
wrappers of _native build their host arrays with explicit element types and the binding checks none of them."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fastvocoder_hip.h")

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "float": ctypes.c_float,
           "double": ctypes.c_double, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}

_INT = r"-?(?:0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)"
_DEFINE = re.compile(rf"^[ \t]*#[ \t]*define[ \t]+(FV_\w+)[ \t]+(?:\(({_INT})\)|({_INT}))[ \t]*$", re.M)
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(fv_\w+)\s*\(([^()]*)\)\s*;")
_PARAMETER = re.compile(r"(.*?)\w+\s*(\[[^\]]*\])?", re.S)        # a type, the parameter's name, array bounds


class NativeError(RuntimeError):
    pass


def _ctype(text, name):
    """The ctypes type of a C type written without a declarator."""
    words = text.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if words == ["const", "char", "*"] else ctypes.c_void_p
    scalar = " ".join(w for w in words if w != "const")
    if scalar not in SCALARS:
        raise NativeError(f"{name}: the binding has no ctypes type for the C type '{' '.join(words)}' (fastvocoder_amd/_abi.py)")
    return SCALARS[scalar]


def parse(text):
    """(prototypes, constants) of a header's text."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {m[1]: int(m[2] or m[3], 0) for m in _DEFINE.finditer(text)}
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\s+\w*\s*\{.*?\}[^;]*;", " ", text, flags=re.S)
    prototypes = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        args = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            m = _PARAMETER.fullmatch(p.strip())
            if not m:
                raise NativeError(f"{name}: cannot read the parameter '{p.strip()}'")
            args.append(_ctype(m[1] + ("*" if m[2] else ""), name))
        prototypes[name] = (None if ret.split() == ["void"] else _ctype(ret, name), args)
    missed = set(re.findall(r"\b(fv_\w+)\s*\(", text)) - set(prototypes)
    if missed:
        raise NativeError(f"cannot read the declaration of {sorted(missed)}")
    return prototypes, constants


_parsed = None


def _header():
    global _parsed
    if _parsed is None:
        if not os.path.exists(HEADER):
            raise NativeError(f"{HEADER} is missing: the binding reads every entry's signature and the FV_* constants from it")
        with open(HEADER) as f:
            _parsed = parse(f.read())
    return _parsed


def prototypes():
    return _header()[0]


def constants():
    return _header()[1]
