"""ctypes binding of libsfmi.so — the C-ABI drop-in boundary (include/sfmi.h).

The product path has NO fallback: if the library is missing or a symbol is
absent, import-time / call-time errors are raised loudly.

The header is the one statement of the ABI: the sources are compiled against it, and every
restype / argtypes here is read from it at import.  Nothing is restated by hand.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsfmi.so")
HEADER = os.path.join(_HERE, "..", "include", "sfmi.h")     # where build.py points -I

_lib = None
f32 = C.c_float
_SCALARS = {"int": C.c_int, "long long": C.c_longlong, "size_t": C.c_size_t, "float": f32, "double": C.c_double,
            "unsigned": C.c_uint, "unsigned long long": C.c_ulonglong}


class SfmiError(RuntimeError):
    pass


def _ctype(text, fn, named):
    """ctypes type of one parameter (`named`: its last word is the parameter's name) or of the return type of `fn`, as the header spells
    it.  const char* is a C string, any other pointer is an address, scalars are the seven of _SCALARS; anything else is an error."""
    words = text.replace("*", " * ").split()
    if "*" in words:
        return C.c_char_p if words[:3] == ["const", "char", "*"] and words.count("*") == 1 else C.c_void_p
    t = _SCALARS.get(" ".join(w for w in (words[:-1] if named else words) if w != "const"))
    if t is None:
        raise SfmiError(f"sfmi.h: {fn}: no ctypes type for {'parameter' if named else 'return type'} `{text.strip()}`")
    return t


def parse_header(text):
    """C header text -> ({name: (restype, argtypes)} of every `ret name(params);`, {NAME: value} of every `#define SFMI_NAME integer`).
    Strict: after comments and preprocessor lines nothing but such declarations may remain, and every type must map (see _ctype)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    codes = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(SFMI_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?)\b(\w+) ?\((.*)\)", stmt)
        if not m:
            raise SfmiError(f"sfmi.h: `{stmt}` is not a function declaration")
        ret, fn, params = m.groups()
        protos[fn] = (_ctype(ret, fn, False), [] if params.strip() == "void" else [_ctype(p, fn, True) for p in params.split(",")])
    return protos, codes


def load_header():
    if not os.path.exists(HEADER):
        raise SfmiError(f"{HEADER} not found: the binding is derived from it and REQUIRED (there is no hand-written table to fall back to)")
    with open(HEADER) as f:
        return parse_header(f.read())


# name -> (restype, argtypes), and the SFMI_* return codes: read once from include/sfmi.h
PROTOTYPES, CODES = load_header()
SFMI_OK, SFMI_EINVAL = CODES["SFMI_OK"], CODES["SFMI_EINVAL"]
_CODE_NAMES = {v: k for k, v in CODES.items()}


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SfmiError(
                f"{LIB_PATH} not found: the HIP extension is REQUIRED (no CPU/eager fallback). "
                "Build it with `python -m shapeformer_amd.build`.")
        # torch's bundled HIP runtime (same SONAME libamdhip64.so.7) must be the one in the process BEFORE
        # libsfmi.so is loaded, otherwise two runtimes coexist and our launches see "no device" (hipError 100).
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError as e:
                raise SfmiError(f"libsfmi.so does not export {name}; rebuild it") from e
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str):
    """Raise on a non-zero return of an entry point, naming the code as sfmi.h does: an SFMI_E* name, or hipError_t for a positive one."""
    if rc != 0:
        raise SfmiError(f"{what} failed with code {rc} ({_CODE_NAMES.get(rc, 'hipError_t' if rc > 0 else 'unknown')})")


def ptr(t):
    """Device (or host) pointer of a torch tensor / numpy array, or None."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


_raw_stream = None


def stream_ptr():
    """hipStream_t of torch's current stream on the current device.  Called once per kernel launch (~900 times per training step):
    torch.cuda.current_stream() builds a Stream object per call; the raw-stream binding the compiler back ends use returns the
    same handle as a plain int."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        get, dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
        if get is not None and dev is not None:
            _raw_stream = lambda: get(dev())
        else:
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream
    return _raw_stream()
