"""ctypes binding of libseer_hip.so, derived from include/seer_hip.h: the header is the one declaration of the C ABI.

`parse_header` reads the header's text once, at import, and yields what this module exports: `SIGNATURES` (entry point ->
(argtypes, restype)), one `ctypes.Structure` class per struct (`GemmDesc`, `AttnDesc`, ...: `CLASS_NAMES`) and every integer
`#define SEER_*` as a module attribute; `ABI_VERSION` is the header's `SEER_ABI_VERSION`.

Type rule:
  - a scalar maps by name: int, int32_t, int64_t, uint32_t, uint64_t, float, double (uint8_t too: it occurs as a pointee only);
  - `const char*` as a return type is c_char_p;
  - a pointer (or an array parameter, `int32_t out[5]`) is c_void_p -- device memory or a stream -- unless the header marks the
    parameter `/* host */`: a host pointer to a struct is POINTER(its class), to a scalar POINTER(its ctype);
  - a struct field is its scalar, c_void_p for any pointer, or an earlier struct by value.
The parser refuses what it does not understand (SeerHipError with the line and the text): a declaration is never skipped.

The library is the product: there is NO fallback.  If it is missing, `load()` raises with the build command;
if a call returns a negative code, `check()` raises `SeerHipError` with the entry point's name.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

_PKG = Path(__file__).resolve().parent
_LIB_PATH = _PKG / "lib" / "libseer_hip.so"
_HEADER = _PKG.parent / "include" / "seer_hip.h"
_lib = None


class SeerHipError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double}
CLASS_NAMES = {"seer_gemm_desc": "GemmDesc", "seer_attn_desc": "AttnDesc", "seer_attn_bwd_desc": "AttnBwdDesc",
               "seer_rowchain_desc": "RowChainDesc", "seer_tn_item": "TnItem", "seer_colfinal_item": "ColfinalItem",
               "seer_transpose_item": "TransposeItem"}

_HOST = "__host__"
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(SEER_\w+)[ \t]+(\S.*?)[ \t]*$", re.M)
_INTEGER = re.compile(r"\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))[uUlL]*\s*\)?")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)
_FIELD = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)")
_FUNCTION = re.compile(r"(const\s+char\s*\*|\w+)\s*\b(seer_\w+)\s*\(([^()]*)\)")
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*\w+\s*(\[\d*\])?")


def _blank(m) -> str:
    return "\n" * m.group().count("\n")            # what is cut out keeps its line breaks: errors name the header's line


def _refuse(what: str, text: str, pos: int, stmt: str):
    at = pos + len(stmt) - len(stmt.lstrip())
    raise SeerHipError(f"seer_hip.h line {text.count(chr(10), 0, at) + 1}: {what}: {' '.join(stmt.split())!r}")


def _statements(text: str, start: int = 0):
    """(offset, statement) for every non-empty `;`-terminated piece of text"""
    for m in re.finditer(r"[^;]+", text):
        if m.group().strip():
            yield start + m.start(), m.group()


def parse_header(text: str, class_names=None):
    """header text -> (constants, structs, signatures): {SEER_* name: int}, {C struct name: ctypes.Structure class} and
    {entry point: (argtypes list, restype)}, by the type rule of the module docstring.  class_names: C struct name -> the class's
    Python name (None: the C name).  Pure: reads nothing but `text`."""
    text = re.sub(r"/\*\s*host\s*\*/", f" {_HOST} ", text)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", _blank, text, flags=re.S)

    constants = {}
    for m in _DEFINE.finditer(text):
        val = _INTEGER.fullmatch(m.group(2))
        if val is None:
            _refuse("not an integer constant", text, m.start(), m.group())
        constants[m.group(1)] = int(val.group(1), 0)
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)

    structs = {}
    for m in _STRUCT.finditer(text):
        cname = m.group(1)
        if m.group(3) != cname or cname in structs or (class_names is not None and cname not in class_names):
            _refuse("struct tag and typedef differ, a second definition, or a struct without a class name", text, m.start(), m.group())
        fields = []
        for pos, stmt in _statements(m.group(2), m.start(2)):
            f = _FIELD.fullmatch(stmt.strip())
            base = f.group(1) if f else None
            if base in _SCALARS or base in structs or (base == "void" and f.group(2)):
                ctype = C.c_void_p if f.group(2) else _SCALARS.get(base) or structs[base]
            else:
                _refuse("struct field of unknown type", text, pos, stmt)
            fields += [(name.strip(), ctype) for name in f.group(3).split(",")]
        structs[cname] = type(class_names[cname] if class_names else cname, (C.Structure,), {"_fields_": fields})
    text = _STRUCT.sub(_blank, text)

    def param(p: str, pos: int, stmt: str):
        host = _HOST in p
        m = _PARAM.fullmatch(p.replace(_HOST, " ").strip())
        base = m.group(1) if m else None
        if base not in _SCALARS and not (m and (m.group(2) or m.group(3)) and (base == "void" or base in structs)):
            _refuse(f"parameter {' '.join(p.split())!r} of unknown scalar type", text, pos, stmt)
        if not (m.group(2) or m.group(3)):
            return _SCALARS[base]
        return C.POINTER(structs.get(base) or _SCALARS[base]) if host and base != "void" else C.c_void_p

    signatures = {}
    for pos, stmt in _statements(text):
        if stmt.strip() == "}" and not text[pos + len(stmt):].strip():
            continue                                # the brace that closes extern "C"
        m = _FUNCTION.fullmatch(stmt.strip())
        if m is None or m.group(2) in signatures:
            _refuse("not a declaration of an entry point (or its second declaration)", text, pos, stmt)
        ret = "".join(m.group(1).split())
        if ret not in _SCALARS and ret != "constchar*":
            _refuse(f"return type {m.group(1)!r} is an unknown scalar type", text, pos, stmt)
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        signatures[m.group(2)] = ([param(p, pos, stmt) for p in params], _SCALARS.get(ret, C.c_char_p))
    # every `seer_...(` outside comments is one of the declarations above: none was skipped
    for m in re.finditer(r"\b(seer_\w+)\s*\(", text):
        if m.group(1) not in signatures:
            _refuse("did not parse as a declaration", text, m.start(), m.group())
    return constants, structs, signatures


_constants, _structs, SIGNATURES = parse_header(_HEADER.read_text(), CLASS_NAMES)
globals().update(_constants)                                     # SEER_EPI_GEGLU, SEER_TILE_WS, ...
globals().update({cls.__name__: cls for cls in _structs.values()})  # GemmDesc, AttnDesc, ...: CLASS_NAMES
ABI_VERSION = _constants["SEER_ABI_VERSION"]


def lib_path() -> Path:
    return Path(os.environ.get("SEER_HIP_LIB", _LIB_PATH))


def bind(cdll, names=None):
    """set argtypes and restype from SIGNATURES on a loaded library: on the entry points in `names` (AttributeError if the library
    lacks one), or -- names=None -- on every declared entry point the library exports (a partial build, an older library)"""
    for name in (SIGNATURES if names is None else names):
        if names is None and not hasattr(cdll, name):
            continue
        fn = getattr(cdll, name)
        fn.argtypes, fn.restype = SIGNATURES[name]
    return cdll


def load():
    """dlopen libseer_hip.so and bind every entry point; raises if the library is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not path.exists():
        raise SeerHipError(
            f"{path} not found: the HIP extension is the only compute path of seervideoldm_amd. "
            "Build it with `python -m seervideoldm_amd.build` (hipcc, --offload-arch=gfx950).")
    lib = bind(C.CDLL(str(path)), list(SIGNATURES))   # AttributeError if the .so lacks a declared symbol
    ver = lib.seer_abi_version()
    if ver != ABI_VERSION:
        raise SeerHipError(f"libseer_hip.so ABI {ver} != binding ABI {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().seer_strerror(code).decode()
        raise SeerHipError(f"{what} failed: {msg} ({code})")
