"""What the tests of the random-bit extension (libscl_hip_rb.so, include/scl_hip_rb.h) share: the description of the library for
the boundary checks of abi_support, the Python model of the square root and of the bit finish -- Python integers, `pow` where
p = 3 mod 4 and its own Tonelli-Shanks otherwise --, the way between integers and the engine's limbs, and the recipe that builds
tests/cxx/_build/test_rb_api (build() calls it, so that the binary travels with the tree).  Standard library and numpy only at
import: build() imports this module.  Every assert carries the values it compared: this is no test module."""
import os
import subprocess

import numpy as np

import abi_support
import cxx_support

RB = abi_support.Library("scl_rb_", "scl_hip_rb.h", "libscl_hip_rb.so", "exports_rb.map", "scl_amd.rb", "SCL_RB_ABI_VERSION")
SYMBOLS = ["scl_rb_abi_version", "scl_rb_bits_finish", "scl_rb_last_error", "scl_rb_sqrt"]
ODD_ROOT, INVERSE = 1, 2
OK_STATUS, ZERO, NONRESIDUE = 0, 1, 2

# the engine's tags (include/scl_hip.h)
M61, M127, MONT128, GF2_128, SECP_SCALAR, SECP_FIELD = 0, 1, 2, 3, 4, 5
MONT_P0, MONT_P1 = 2 ** 128 - 159, 2 ** 127 - 1
SECP_Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SECP_P = 2 ** 256 - 2 ** 32 - 977
PRIME_FIELDS = [M61, M127, MONT128, SECP_SCALAR, SECP_FIELD]
NAMES = {M61: "m61", M127: "m127", MONT128: "mont128", SECP_SCALAR: "secp_scalar", SECP_FIELD: "secp_field"}


def prime(f, mont_p=MONT_P0):
    return {M61: 2 ** 61 - 1, M127: 2 ** 127 - 1, MONT128: mont_p, SECP_SCALAR: SECP_Q, SECP_FIELD: SECP_P}[f]


def limbs(f):
    return {M61: 1, M127: 2, MONT128: 2, GF2_128: 2, SECP_SCALAR: 4, SECP_FIELD: 4}[f]


def radix(f):
    """the Montgomery radix of the field's stored form (1: plain residues)"""
    return {M61: 1, M127: 1, MONT128: 2 ** 128, SECP_SCALAR: 2 ** 256, SECP_FIELD: 2 ** 256}[f]


# ---- the model -------------------------------------------------------------------------------------------------------------------
def split(p):
    """p - 1 = 2^s q, q odd -> (s, q)"""
    s, q = 0, p - 1
    while q % 2 == 0:
        s, q = s + 1, q // 2
    return s, q


def is_residue(p, a):
    """Euler's criterion for a != 0"""
    return pow(a, (p - 1) // 2, p) == 1


def tonelli_shanks(p, a):
    """a root of the residue a, the textbook way (the variable-time form: the exponent of b is searched)"""
    s, q = split(p)
    z = 2
    while is_residue(p, z):
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


def model_sqrt(p, a, flags=0):
    """-> (value written, status): the even root (ODD_ROOT: the odd one), its inverse with INVERSE; 0 for zero and non-residues"""
    if a == 0:
        return 0, ZERO
    if not is_residue(p, a):
        return 0, NONRESIDUE
    x = pow(a, (p + 1) // 4, p) if p % 4 == 3 else tonelli_shanks(p, a)
    assert x * x % p == a, (p, a, x)
    if (x & 1) != (1 if flags & ODD_ROOT else 0):
        x = p - x
    return (pow(x, -1, p) if flags & INVERSE else x), OK_STATUS


def model_bits(p, u, r):
    """u [N], r [rows][N] as integers -> (b [rows][N], status [N]): b = (r / root(u) + 1) / 2, zero where the status is set"""
    half = pow(2, -1, p)
    cols = [model_sqrt(p, v, INVERSE) for v in u]
    return [[(half * v * row[s] + half) % p if st == OK_STATUS else 0 for s, (v, st) in enumerate(cols)] for row in r], [st for _, st in cols]


# ---- integers <-> the engine's limbs ------------------------------------------------------------------------------------------------
def to_limbs(f, values, mont_p=MONT_P0):
    """integers below p -> [len][L] uint64, in the field's stored form"""
    p, R, L = prime(f, mont_p), radix(f), limbs(f)
    return np.array([[(v * R % p >> (64 * i)) & (2 ** 64 - 1) for i in range(L)] for v in values], dtype=np.uint64).reshape(len(values), L)


def from_limbs(f, arr, mont_p=MONT_P0):
    """[..][L] uint64 -> the integers, flat"""
    p, L = prime(f, mont_p), limbs(f)
    rinv = pow(radix(f), -1, p)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % p for row in np.asarray(arr, dtype=np.uint64).reshape(-1, L)]


def seeded(p, n, seed):
    """n integers below p, about half of them residues: numpy's generator on `seed`"""
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)]


# ---- the boundary: abi_support's dependency check counts the siblings among its own five; this library is not one of them -----------
def check_engine_is_only_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and against no other extension library; every undefined scl_*
    symbol is a prototype of scl_hip.h"""
    dyn = subprocess.run(["readelf", "-d", RB.path("so")], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip.so" in dyn and "$ORIGIN" in dyn, dyn
    assert not any(x.so in dyn for x in abi_support.EXTENSIONS), dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", RB.path("so")], capture_output=True, text=True, check=True).stdout
    used = sorted({ln.split()[-1].split("@")[0] for ln in und.splitlines() if "scl_" in ln})
    assert used and set(used) <= set(abi_support.declared_symbols(abi_support.ENGINE)), used


# ---- the mirror's test program -------------------------------------------------------------------------------------------------------
def rb_api_binary():
    """tests/cxx/test_rb_api.cc against the mirror, libscl_hip_rb.so and the engine -> tests/cxx/_build/test_rb_api; rebuilt when
    stale (the recipe and the staleness rule of cxx_support.mirror_binary, whose table is closed)"""
    src, exe = os.path.join(cxx_support.CXX, "test_rb_api.cc"), os.path.join(cxx_support.BUILD, "test_rb_api")
    if not os.path.exists(exe) or os.path.getmtime(exe) < cxx_support.newest_input(src):
        os.makedirs(cxx_support.BUILD, exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{cxx_support.ROOT}/include", "-o", exe, src,
                            f"-L{cxx_support.LIBDIR}", "-lscl_hip_rb", "-lscl_hip", f"-Wl,-rpath,{cxx_support.LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe
