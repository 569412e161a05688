"""What the tests of the comparison extension (libscl_hip_cmp.so, include/scl_hip_cmp.h) share: the description of the library for the
boundary checks of abi_support, the Python-integer model of the three calls and of the tree on clear values, and the recipe that
builds tests/cxx/_build/test_cmp_api (build() calls it, so that the binary travels with the tree).  Integers, limbs, sharings and
the field cases are those of fx_support.  Standard library and numpy only at import: build() imports this module.  Every assert
carries the values it compared: this is no test module."""
import os
import subprocess

import numpy as np

import abi_support
import cxx_support
import fx_support as FXS

CMP = abi_support.Library("scl_cmp_", "scl_hip_cmp.h", "libscl_hip_cmp.so", "exports_cmp.map", "scl_amd.cmp", "SCL_CMP_ABI_VERSION")
SYMBOLS = ["scl_cmp_abi_version", "scl_cmp_finish", "scl_cmp_first_mask", "scl_cmp_last_error", "scl_cmp_level_mask", "scl_cmp_levels", "scl_cmp_planes"]
LT_ONLY = 1
MOD, TRUNC, LTZ = 0, 1, 2
# every tree shape with a lone node at some level appears among these, and both sides of every limb boundary
WIDTHS = list(range(1, 18)) + [59, 63, 64, 65, 125, 127, 128, 129, 254]


# ---- the counts, by the loop that defines them ------------------------------------------------------------------------------------
def level_counts(w):
    """the node count each level starts from: w, ceil(w / 2), ... down to 2 (or [w] for w <= 2: at least one level)"""
    out, cnt = [w], w
    while (cnt + 1) // 2 > 1:
        cnt = (cnt + 1) // 2
        out.append(cnt)
    return out


def model_levels(w):
    return len(level_counts(w))


def model_planes(w):
    """2 ceil(cnt / 2) planes per level, 1 for the last"""
    counts = level_counts(w)
    return sum(2 * ((c + 1) // 2) for c in counts[:-1]) + 1


# ---- the three calls on object arrays of Python integers ----------------------------------------------------------------------------
def a_open_col(c, w, B):
    """c [N] opened -> (cmod [N], status [N] uint8): status 1 and cmod 0 where c >= 2^(B+1)"""
    bad = (c >> (B + 1)) != 0
    cmod = c & ((1 << w) - 1)
    cmod[bad.astype(bool)] = 0
    return cmod, bad.astype(np.uint8)


def _combine(p, lt_hi, eq_hi, lt_lo, eq_lo):
    return (lt_hi + eq_hi * lt_lo) % p, eq_hi * eq_lo % p


def _pairs(p, lts, eqs, r2, lt_only):
    """nodes (lts[i], eqs[i]), each [rows][N] -> the node array d [P][rows][N]: pairs combined, a lone last node with the identity,
    + r2"""
    out = []
    for j in range((len(lts) + 1) // 2):
        lo, hi = 2 * j, 2 * j + 1
        lt, eq = _combine(p, lts[hi], eqs[hi], lts[lo], eqs[lo]) if hi < len(lts) else (lts[lo] % p, eqs[lo] % p)
        out += [lt] if lt_only else [lt, eq]
    assert len(out) == len(r2), (len(out), len(r2))
    return np.stack([(o + r) % p for o, r in zip(out, r2)])


def a_first(p, cmod, bits, r2, w, lt_only=False):
    """cmod [N] (integers below 2^w), bits [>= w][rows][N], r2 [P][rows][N] -> d [P][rows][N]: the leaves lt_i = (1 - c_i) b_i,
    eq_i = c_i ? b_i : 1 - b_i, combined in pairs"""
    lts, eqs = [], []
    for i in range(w):
        ci = ((cmod >> i) & 1).astype(bool)[None, :]
        lts.append(np.where(ci, 0, bits[i]))
        eqs.append(np.where(ci, bits[i], (1 - bits[i]) % p))
    return _pairs(p, lts, eqs, r2, lt_only)


def a_level(p, nodes, r2, lt_only=False):
    """nodes [2 cnt][rows][N], r2 [P][rows][N] -> d [P][rows][N]"""
    return _pairs(p, list(nodes[0::2]), list(nodes[1::2]), r2, lt_only)


def a_finish(p, lt, cmod, status, rlow, x, w, what):
    """lt, rlow, x [rows][N], cmod, status [N] -> [rows][N]; a column whose status is set is 0"""
    a = (cmod[None, :] - rlow + (lt << w)) % p
    if what == MOD:
        y = a
    else:
        y = (x - a) * pow(1 << w, -1, p) % p
        if what == LTZ:
            y = -y % p
    y[:, np.asarray(status).astype(bool)] = 0
    return y


# ---- the tree and the pipelines on clear values: the yardstick, itself pinned on the CPU (tests/test_cmp_host.py) ---------------
def model_bit_lt(p, cmod, bits, w):
    """cmod [N] integers below 2^w, bits [w][N] of 0 / 1 -> [N] of 0 / 1: the tree of the three calls with r2 = 0, one row"""
    counts = level_counts(w)
    zeros = lambda P: np.zeros((P, 1, len(cmod)), dtype=object)
    last = len(counts) == 1
    nodes = a_first(p, cmod, np.asarray(bits, dtype=object)[:, None, :], zeros(1 if last else 2 * ((w + 1) // 2)), w, last)
    for lv, cnt in enumerate(counts[1:], start=1):
        last = lv == len(counts) - 1
        assert len(nodes) == 2 * cnt, (len(nodes), cnt)
        nodes = a_level(p, nodes, zeros(1 if last else 2 * ((cnt + 1) // 2)), last)
    assert nodes.shape == (1, 1, len(cmod)), nodes.shape
    return nodes[0, 0]


def model_pipeline(p, x, bits, k, w, what):
    """x [N] elements that stand for signed k-bit integers, bits [B][N] of 0 / 1 -> (the result [N] as elements, cmod, rlow): the
    protocol on clear values -- mask, open, less-than, finish"""
    B = len(bits)
    planes = np.asarray(bits, dtype=object)
    c, rlow = FXS.a_mask(p, x, planes, k, w)
    cmod, status = a_open_col(c, w, B)
    assert not status.any(), (k, w, B)
    lt = model_bit_lt(p, cmod, planes[:w], w)
    return a_finish(p, lt[None, :], cmod, status, rlow[None, :], x[None, :], w, what)[0], cmod, rlow


def signed(p, v):
    return v if v <= p // 2 else v - p


def corner_bits(w, B, kind, seed):
    """B bits (0 / 1) whose lowest w hit a corner of the comparison: 'zero' r' = 0, 'ones' r' = 2^w - 1, 'any' seeded; the bits from
    w up are seeded.  (c' = (x + 2^(k-1) + r) mod 2^w = (x + r') mod 2^w for w <= k - 1, so c' == r' is x mod 2^w == 0 under any
    bits: the caller's x = 0 and x = -2^(k-1) are that corner.)"""
    bits = FXS.seeded_bits(B, seed)
    if kind == "zero":
        bits[:w] = [0] * w
    elif kind == "ones":
        bits[:w] = [1] * w
    return bits


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def check_engine_is_only_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and against no other extension library; every undefined scl_*
    symbol is a prototype of scl_hip.h"""
    dyn = subprocess.run(["readelf", "-d", CMP.path("so")], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip.so" in dyn and "$ORIGIN" in dyn, dyn
    assert not any(x.so in dyn for x in abi_support.EXTENSIONS) and "libscl_hip_rb.so" not in dyn and "libscl_hip_fx.so" not in dyn, dyn
    und = subprocess.run(["nm", "-D", "--undefined-only", CMP.path("so")], capture_output=True, text=True, check=True).stdout
    used = sorted({ln.split()[-1].split("@")[0] for ln in und.splitlines() if "scl_" in ln})
    assert used and set(used) <= set(abi_support.declared_symbols(abi_support.ENGINE)), used


# ---- the mirror's test program -------------------------------------------------------------------------------------------------------
def cmp_api_binary():
    """tests/cxx/test_cmp_api.cc against the mirror, libscl_hip_cmp.so, libscl_hip_fx.so and the engine -> tests/cxx/_build/test_cmp_api;
    rebuilt when stale (the recipe and the staleness rule of cxx_support.mirror_binary, whose table is closed)"""
    src, exe = os.path.join(cxx_support.CXX, "test_cmp_api.cc"), os.path.join(cxx_support.BUILD, "test_cmp_api")
    if not os.path.exists(exe) or os.path.getmtime(exe) < cxx_support.newest_input(src):
        os.makedirs(cxx_support.BUILD, exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{cxx_support.ROOT}/include", "-o", exe, src,
                            f"-L{cxx_support.LIBDIR}", "-lscl_hip_cmp", "-lscl_hip", f"-Wl,-rpath,{cxx_support.LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe
