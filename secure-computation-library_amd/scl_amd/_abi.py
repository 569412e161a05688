"""scl_amd._abi -- how the package binds a library of csrc/: the one loader and the one reader of a boundary header's prototypes,
for the engine (scl_amd itself) and the extension libraries beside it (mpc, prep, hm, ip, vf, rb, fx, cmp).  Imports nothing of scl_amd."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))

_SCALARS = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "unsigned": C.c_uint, "float": C.c_float}
_RETS = {"int": C.c_int, "void": None, "size_t": C.c_size_t, "const char*": C.c_char_p}


def load(name: str):
    """(library, path) of lib<name>.so beside the package"""
    so = os.path.join(_HERE, f"lib{name}.so")
    if not os.path.exists(so):
        raise ImportError(
            f"{so} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C secure-computation-library_amd/csrc)")
    return C.CDLL(so), so


def find_header(header_name: str):
    """the repository's header, or the copy the csrc Makefile leaves next to the .so (a package moved without the tree); None"""
    candidates = [os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", header_name), os.path.join(_HERE, header_name)]
    return next((c for c in candidates if os.path.exists(c)), None)


def declare(lib, so_path: str, header_name: str, prefix: str, version_macro: str, who: str, version_optional: bool = False) -> int:
    """argtypes / restype of every entry point `prefix`* from the prototypes of include/`header_name` (the boundary's one source
    of truth): a forgotten c_size_t wrap or a swapped argument is then a ctypes.ArgumentError, not a wild pointer.  Every pointer
    parameter is c_void_p (accepts ints, data_ptr() wrappers, bytes, byref() and None).  The boundary's version is compared
    BEFORE any other symbol is looked up: a library built from an older header fails HERE, with a message that says so, not at
    the lookup of a symbol it does not have.  Returns the number of prototypes."""
    hdr = find_header(header_name)
    if hdr is None:
        raise ImportError(f"{who}: include/{header_name} not found beside the package")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    want = re.search(r"#define\s+" + version_macro + r"\s+(\d+)", src)
    version = getattr(lib, prefix + "abi_version")
    version.restype = C.c_int
    version.argtypes = []
    have = version()
    if (not want and not version_optional) or (want and have != int(want.group(1))):
        raise ImportError(f"{who}: {so_path} implements ABI version {have}, {hdr} declares {want.group(1) if want else '?'}: "
                          "rebuild the extension (make -C secure-computation-library_amd/csrc)")
    n = 0
    for m in re.finditer(r"\b(int|void|size_t|const char\s*\*)\s*(" + prefix + r"\w+)\s*\(([^;{]*?)\)\s*;", src):
        ret, name, params = m.group(1).replace(" ", "").replace("constchar*", "const char*"), m.group(2), m.group(3)
        fn = getattr(lib, name)
        fn.restype = _RETS[ret]
        argt = []
        for prm in [x.strip() for x in params.split(",")]:
            if prm in ("void", ""):
                continue
            if "*" in prm or "[" in prm:
                argt.append(C.c_void_p)
            else:
                base = re.sub(r"\bconst\b", "", prm).split()
                if base[0] not in _SCALARS:
                    raise ImportError(f"{who}: {name}: parameter type {base[0]!r} in {hdr} has no ctypes mapping here")
                argt.append(_SCALARS[base[0]])
        fn.argtypes = argt
        n += 1
    return n
