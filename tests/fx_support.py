"""What the tests of the fixed-point extension (libscl_hip_fx.so, include/scl_hip_fx.h) share: the description of the library for
the boundary checks of abi_support, the Python model of the three calls -- Python integers: compose, the mask, the finish, and the
exact form of what a probabilistic truncation yields --, the way between integers and the engine's limbs, and the recipe that
builds tests/cxx/_build/test_fx_api (build() calls it, so that the binary travels with the tree).  Standard library and numpy only
at import: build() imports this module.  Every assert carries the values it compared: this is no test module."""
import os
import subprocess

import numpy as np

import abi_support
import cxx_support

FX = abi_support.Library("scl_fx_", "scl_hip_fx.h", "libscl_hip_fx.so", "exports_fx.map", "scl_amd.fx", "SCL_FX_ABI_VERSION")
SYMBOLS = ["scl_fx_abi_version", "scl_fx_compose", "scl_fx_last_error", "scl_fx_max_bits", "scl_fx_trunc_finish", "scl_fx_trunc_mask"]
OK_STATUS, RANGE = 0, 1

# the engine's tags (include/scl_hip.h)
M61, M127, MONT128, GF2_128, SECP_SCALAR, SECP_FIELD = 0, 1, 2, 3, 4, 5
MONT_P0, MONT_P1 = 2 ** 128 - 159, 2 ** 127 - 1
SECP_Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SECP_P = 2 ** 256 - 2 ** 32 - 977
PRIME_FIELDS = [M61, M127, MONT128, SECP_SCALAR, SECP_FIELD]
NAMES = {M61: "m61", M127: "m127", MONT128: "mont128", SECP_SCALAR: "secp_scalar", SECP_FIELD: "secp_field"}
# (name, tag, the Mont128 modulus or None): Mont128 at both moduli of rb_support
CASES = [("m61", M61, None), ("m127", M127, None), ("mont128_p0", MONT128, MONT_P0), ("mont128_p1", MONT128, MONT_P1),
         ("secp_scalar", SECP_SCALAR, None), ("secp_field", SECP_FIELD, None)]


def prime(f, mont_p=None):
    return {M61: 2 ** 61 - 1, M127: 2 ** 127 - 1, MONT128: mont_p or MONT_P0, SECP_SCALAR: SECP_Q, SECP_FIELD: SECP_P}[f]


def limbs(f):
    return {M61: 1, M127: 2, MONT128: 2, GF2_128: 2, SECP_SCALAR: 4, SECP_FIELD: 4}[f]


def radix(f):
    """the Montgomery radix of the field's stored form (1: plain residues)"""
    return {M61: 1, M127: 1, MONT128: 2 ** 128, SECP_SCALAR: 2 ** 256, SECP_FIELD: 2 ** 256}[f]


def max_bits(p):
    """|p| - 2, the largest B: 2^(B+1) < p"""
    return p.bit_length() - 2


# ---- the model -------------------------------------------------------------------------------------------------------------------
def model_compose(p, planes):
    """planes [B][..] of integers below p (any nesting below the plane axis, here flat lists) -> sum 2^i planes[i] mod p, flat"""
    return [sum(pl[s] << i for i, pl in enumerate(planes)) % p for s in range(len(planes[0]))]


def model_mask(p, x, planes, k, shift):
    """x [N], planes [B][N] -> (c, rlow) [N] each: c = x + 2^(k-1) + r, rlow = r' mod p"""
    r, rlow = model_compose(p, planes), model_compose(p, planes[:shift])
    return [(v + (1 << (k - 1)) + rr) % p for v, rr in zip(x, r)], rlow


def model_finish(p, c, x, rlow, shift, B):
    """c [N] opened, x, rlow [rows][N] -> (y [rows][N], status [N]): c' = c mod 2^shift as an integer, y = (x + rlow - c') 2^-shift;
    status 1 and a column of zeros where c >= 2^(B+1)"""
    inv = pow(1 << shift, -1, p)
    status = [RANGE if v >> (B + 1) else OK_STATUS for v in c]
    return [[0 if st else (xv + lv - (cv & ((1 << shift) - 1))) * inv % p for xv, lv, cv, st in zip(xr, lr, c, status)]
            for xr, lr in zip(x, rlow)], status


def model_open(p, lam, shares):
    """sum_j lam[j] shares[j][s] mod p"""
    return [sum(l * row[s] for l, row in zip(lam, shares)) % p for s in range(len(shares[0]))]


def lagrange_at_zero(p, m):
    """the basis of the nodes 1..m at 0"""
    out = []
    for j in range(1, m + 1):
        num = den = 1
        for i in range(1, m + 1):
            if i != j:
                num, den = num * (-i) % p, den * (j - i) % p
        out.append(num * pow(den, -1, p) % p)
    return out


def exact_trunc(p, x, bits, k, shift):
    """what the truncation of the signed k-bit integer x (as an element: x mod p) yields with the opened bits `bits` (integers
    0 / 1, at least `shift` of them): floor((x + 2^(k-1)) / 2^shift) + carry - 2^(k-1-shift) mod p, the carry that of
    (x + 2^(k-1)) mod 2^shift + r'"""
    xs = x if x < p // 2 else x - p                                # the signed value
    assert -(1 << (k - 1)) <= xs < (1 << (k - 1)), (xs, k)
    rlow = sum(b << i for i, b in enumerate(bits[:shift]))
    u = xs + (1 << (k - 1))
    carry = 1 if (u & ((1 << shift) - 1)) + rlow >= (1 << shift) else 0
    y = (u >> shift) + carry - (1 << (k - 1 - shift))
    assert y in (xs >> shift, (xs >> shift) + 1), (xs, shift, y)
    return y % p


# ---- integers <-> the engine's limbs ------------------------------------------------------------------------------------------------
def to_limbs(f, values, mont_p=None):
    """integers below p -> [len][L] uint64, in the field's stored form"""
    p, R, L = prime(f, mont_p), radix(f), limbs(f)
    return np.array([[(v * R % p >> (64 * i)) & (2 ** 64 - 1) for i in range(L)] for v in values], dtype=np.uint64).reshape(len(values), L)


def from_limbs(f, arr, mont_p=None):
    """[..][L] uint64 -> the integers, flat"""
    p, L = prime(f, mont_p), limbs(f)
    rinv = pow(radix(f), -1, p)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % p for row in np.asarray(arr, dtype=np.uint64).reshape(-1, L)]


# ---- the same on whole arrays: numpy object arrays of Python integers, any shape ---------------------------------------------------
def ints_of(f, arr, mont_p=None):
    """[..][L] uint64 -> an object array [..] of the integers the limbs stand for"""
    p, L = prime(f, mont_p), limbs(f)
    a = np.asarray(arr, dtype=np.uint64)
    v = sum(a[..., i].astype(object) << (64 * i) for i in range(L))
    return v * pow(radix(f), -1, p) % p if radix(f) != 1 else v


def limbs_of(f, values, mont_p=None):
    """an object array [..] of integers below p -> [..][L] uint64, in the field's stored form"""
    p, R, L = prime(f, mont_p), radix(f), limbs(f)
    v = np.asarray(values, dtype=object)
    v = v * R % p if R != 1 else v
    return np.stack([((v >> (64 * i)) & (2 ** 64 - 1)).astype(np.uint64) for i in range(L)], axis=-1)


def uniform(p, shape, seed):
    """an object array of integers below 2^(|p| - 1) < p: every bit below the top one seeded (shares of bits look like these)"""
    bits = p.bit_length() - 1
    L = -(-bits // 64)
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 64, size=tuple(shape) + (L,), dtype=np.uint64)
    v = sum(w[..., i].astype(object) << (64 * i) for i in range(L))
    return v & ((1 << bits) - 1)


def a_compose(p, planes):
    """planes [B][..] -> sum 2^i planes[i] mod p"""
    return sum(pl << i for i, pl in enumerate(planes)) % p


def a_mask(p, x, planes, k, shift):
    """-> (c, rlow), the shapes of x"""
    return (x + (1 << (k - 1)) + a_compose(p, planes)) % p, a_compose(p, planes[:shift])


def a_finish(p, c, x, rlow, shift, B):
    """c [N] opened, x, rlow [rows][N] -> (y [rows][N], status [N] uint8)"""
    bad = (c >> (B + 1)) != 0
    y = (x + rlow - (c & ((1 << shift) - 1))) * pow(1 << shift, -1, p) % p
    y[:, bad.astype(bool)] = 0
    return y, bad.astype(np.uint8)


def a_share(p, secrets, t, n, seed):
    """[N] -> [n][N]: degree-t sharings at the nodes 1..n, the coefficients seeded"""
    co = [np.asarray(secrets, dtype=object) % p] + [uniform(p, np.shape(secrets), seed + e) for e in range(1, t + 1)]
    return np.stack([sum(c * pow(i, e, p) for e, c in enumerate(co)) % p for i in range(1, n + 1)])


def seeded(p, n, seed):
    """n integers below p: numpy's generator on `seed`"""
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % p for _ in range(n)]


def seeded_bits(n, seed):
    rng = np.random.default_rng(seed)
    return [int(b) for b in rng.integers(0, 2, n)]


def share_poly(p, secret, t, n, seed):
    """the shares at the nodes 1..n of a degree-t polynomial with the constant term `secret`, its other coefficients seeded"""
    co = [secret % p] + seeded(p, t, seed)
    return [sum(c * pow(i, e, p) for e, c in enumerate(co)) % p for i in range(1, n + 1)]


def shapes(p):
    """(B, k, shift) of a field: the smallest, the largest, a wide kappa, one mid case, and shift on both sides of every limb
    boundary below |p| - 2"""
    top = max_bits(p)
    out = [(2, 2, 1), (top, top, top - 1), (top, 2, 1), (top // 2 + 7, top // 2 + 2, top // 4 + 1)]
    for edge in (64, 128, 192):
        if edge + 1 < top:
            out += [(top, top - 1, s) for s in (edge - 1, edge, edge + 1)]
    return out


# ---- the boundary: abi_support's dependency check counts the siblings among its own five; this library is not one of them -----------
def check_engine_is_only_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and against no other extension library; every undefined scl_*
    symbol is a prototype of scl_hip.h"""
    dyn = subprocess.run(["readelf", "-d", FX.path("so")], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip.so" in dyn and "$ORIGIN" in dyn, dyn
    assert not any(x.so in dyn for x in abi_support.EXTENSIONS) and "libscl_hip_rb.so" not in dyn, dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", FX.path("so")], capture_output=True, text=True, check=True).stdout
    used = sorted({ln.split()[-1].split("@")[0] for ln in und.splitlines() if "scl_" in ln})
    assert used and set(used) <= set(abi_support.declared_symbols(abi_support.ENGINE)), used


# ---- the mirror's test program -------------------------------------------------------------------------------------------------------
def fx_api_binary():
    """tests/cxx/test_fx_api.cc against the mirror, libscl_hip_fx.so and the engine -> tests/cxx/_build/test_fx_api; rebuilt when
    stale (the recipe and the staleness rule of cxx_support.mirror_binary, whose table is closed)"""
    src, exe = os.path.join(cxx_support.CXX, "test_fx_api.cc"), os.path.join(cxx_support.BUILD, "test_fx_api")
    if not os.path.exists(exe) or os.path.getmtime(exe) < cxx_support.newest_input(src):
        os.makedirs(cxx_support.BUILD, exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{cxx_support.ROOT}/include", "-o", exe, src,
                            f"-L{cxx_support.LIBDIR}", "-lscl_hip_fx", "-lscl_hip", f"-Wl,-rpath,{cxx_support.LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe
