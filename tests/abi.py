"""The C headers under include/ as the host tests read them: one parser for the declarations, one for the constants, the rule that matches
a line of the binding table (real3dportrait_amd/_lib.py SIGNATURES) to a declared parameter type, and the refusal check the argument-error
tests of the audio and fit units share.  Imported by tests/test_abi.py and the per-unit host tests the way tests/sr_formats.py is; it holds
no tests and never loads the library itself."""
import ctypes
import os
import re

from conftest import ROOT

# the header, then the five companion headers it includes, in the order it includes them: the functions each declares itself
HEADERS = {"r3d_hip.h": 74, "r3d_hip_clip.h": 3, "r3d_hip_video.h": 2, "r3d_hip_source.h": 6, "r3d_hip_audio.h": 3, "r3d_hip_fit.h": 4}


def header_source(header):
    """include/<header> without its comments."""
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def header_declarations(header="r3d_hip.h"):
    """{name: (return type, [parameter type, ...])} of every function include/<header> declares itself (not the headers it includes):
    comments stripped, `const` dropped, no blanks around a star ("const float* const* ext_bounds" -> "float**",
    "unsigned long long* cycles" -> "unsigned long long*")."""
    norm = lambda t: re.sub(r"\s*\*\s*", "*", " ".join(re.sub(r"\bconst\b", " ", t).split()))
    decls = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?)\s*\b(r3d_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_source(header), flags=re.M):
        assert name not in decls, name
        types = []
        for p in (params.split(",") if params.strip() not in ("", "void") else []):
            m = re.match(r"^(.*?)(\w+)$", " ".join(p.split()))          # everything up to the parameter's name
            assert m and m.group(1).strip(), (name, p)
            types.append(norm(m.group(1)))
        decls[name] = (norm(ret), types)
    return decls


def header_constants(header):
    """{name: int} of every `#define R3D_X <integer>` (the integer bare, negative or in parentheses) and every enumerator `R3D_X = <integer>`
    include/<header> holds itself; its include guard, which has no value, is not among them."""
    src = header_source(header)
    integer = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))"
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(R3D_\w+)[ \t]+\(?[ \t]*%s[ \t]*\)?[ \t]*$" % integer, src, flags=re.M)
    found += re.findall(r"^[ \t]*(R3D_\w+)[ \t]*=[ \t]*%s[ \t]*,?[ \t]*$" % integer, src, flags=re.M)
    consts = {}
    for name, value in found:
        assert name not in consts, name
        consts[name] = int(value, 0)
    assert "R3D_" + header[4:-2].upper() + "_H" not in consts
    return consts


C_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
             "uint64_t": ctypes.c_uint64, "unsigned long long": ctypes.c_ulonglong}
C_RETURNS = dict(C_SCALARS, **{"char*": ctypes.c_char_p})
# what a bare c_void_p in the table (a host pointer the package never looks into) may stand for: an opaque handle or the 128-byte id (void*),
# the array of chain ops, an array of device addresses; a host pointer to a scalar or a handle is a ctypes.POINTER of exactly that type
UNTYPED_HOST = {"void*", "r3d_chain_op*", "float**"}


def entry_matches(entry, ctype, _lib):
    """Does one table entry stand for the header's parameter type `ctype`, exactly?"""
    if ctype == "r3d_stream_t":
        return isinstance(entry, _lib.Stream)
    if isinstance(entry, _lib.DevPtr):
        return ctype == entry.elem + "*" and entry.elem in _lib.DevPtr.DTYPES
    if isinstance(entry, _lib.Stream):
        return False
    if ctype in C_SCALARS:
        return entry is C_SCALARS[ctype]
    if entry is ctypes.c_void_p:
        return ctype in UNTYPED_HOST
    if ctype == "void**":
        return entry is ctypes.POINTER(ctypes.c_void_p)
    return ctype.endswith("*") and ctype[:-1] in C_SCALARS and entry is ctypes.POINTER(C_SCALARS[ctype[:-1]])


def refusals(lib, prefix):
    """refused(fn, base, quote, rc=-1, **over) for the entry points `prefix` + fn of `lib`: the call with base's values in their order,
    `over` in the place of some and a NULL stream returns rc, and r3d_last_error() holds the entry point's tag ("a2m_conv1d:" for prefix
    "r3d_a2m_", fn "conv1d") and the quote."""
    def refused(fn, base, quote, rc=-1, **over):
        assert set(over) <= set(base), (fn, over)          # an override the entry point has no argument for would leave a valid call
        got = getattr(lib, prefix + fn)(*dict(base, **over).values(), None)
        msg = lib.r3d_last_error()
        assert got == rc and (prefix[4:] + fn).encode() + b":" in msg and quote in msg, (fn, over, got, msg)
    return refused
