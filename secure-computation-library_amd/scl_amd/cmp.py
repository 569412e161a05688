"""scl_amd.cmp -- Python harness over libscl_hip_cmp.so, exact comparison and truncation of Shamir sharings (include/scl_hip_cmp.h).

The bitwise less-than of an opened value against shared bits, by a tree of Damgard-Nielsen multiplications, and the three results
that are linear on top of it: x mod 2^w, the exact floor(x / 2^w) and [x < 0].  `first_mask` is the first level of the tree fused
with the opening of c, `level_mask` a later level, `finish` the local last step; `bit_lt` is the whole tree and `mod2m`, `trunc`,
`ltz` and `lt` the local pipelines for all simulated parties on one device, over scl_amd.fx (the mask) and scl_amd.hm (each level's
opening).  Plumbing only, like scl_amd itself: torch device buffers and the current HIP stream go to the C ABI; there is no CPU or
torch fallback.  Tensors are those of scl_amd.fx: int64 limbs, SoA rows `[rows][N][L]`, bit planes `[B][rows][N][L]`; a node array
is `[P][rows][N][L]`, plane 2j the lt and plane 2j + 1 the eq of node j, planes and rows any pitch apart -- a matrix
`[rows][P N][L]`, what one scl_amd.hm.mul_finish over P N columns yields, is `a.view(rows, P, N, L).transpose(0, 1)` without a copy.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_cmp.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_cmp")

LT_ONLY = 1
MOD, TRUNC, LTZ = 0, 1, 2
STATUS_OK, STATUS_RANGE = 0, 1


# argtypes / restype of every entry point from the prototypes of include/scl_hip_cmp.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_cmp.h", "scl_cmp_", "SCL_CMP_ABI_VERSION", "scl_amd.cmp")


_chk = _scl._checker(lib.scl_cmp_last_error)
_z = C.c_size_t


def levels(w: int) -> int:
    """max(1, ceil(log2 w)): the levels of the tree, one round each (scl_cmp_levels)"""
    return int(lib.scl_cmp_levels(w))


def planes(w: int) -> int:
    """the double-sharing planes of N a comparison of w bits consumes over all levels (scl_cmp_planes); 119 for w = 59"""
    return int(lib.scl_cmp_planes(w))


def _node_planes(field, t: torch.Tensor, count, rows, N, like, what: str):
    """(pointer, plane stride, row stride) of `count` planes [count][rows][N][L] (or [count][N][L]: one row); count None: any, the library
    decides"""
    from scl_amd.fx import _planes
    p, ps, rs, have = _planes(field, t, rows, N, like, what)
    if count is not None and have != count:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{what}: {have} planes, expected {count}")
    return p, ps, rs


def first_mask(field, csh, bits, r2, w: int, B: int, lam=None, flags: int = 0, out=None, cmod=None, status=None):
    """(d, cmod, status): the first level of the tree, fused with the opening of c (scl_cmp_first_mask).  csh [m][N][L], the
    m <= 64 shares of c (or [N][L]: c already opened), lam their Lagrange basis (default: nodes 1..m at 0; for an opened c: one);
    bits [>= w][rows][N][L], of which the planes 0 .. w - 1 are read; r2 and d node arrays [P][rows][N][L], P = 2 ceil(w / 2), or
    1 under LT_ONLY (w <= 2).  cmod [N][L] = c mod 2^w; one status byte per column: 1 where c >= 2^(B+1)."""
    from scl_amd import hm
    L = _scl.limbs(field)
    D = _scl._rows3(field, csh, "first_mask csh")
    m, N, _ = D.shape
    if bits.dim() == 3:
        bits = bits.unsqueeze(1)
    rows = bits.shape[1] if bits.dim() == 4 else 0
    P = None if w < 1 else 1 if flags & LT_ONLY else 2 * ((w + 1) // 2)  # (w == 0: the library says so)
    if bits.dim() == 4 and bits.shape[0] < w:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"first_mask bits: {bits.shape[0]} planes, w = {w} are read")
    pb, bps, brs = _node_planes(field, bits, None, rows, N, D, "first_mask bits")
    if r2.dim() == 3:
        r2 = r2.unsqueeze(1)
    pr, rps, rrs = _node_planes(field, r2, P, rows, N, D, "first_mask r2")
    d = torch.empty(P or 1, rows, N, L, dtype=torch.int64, device=D.device) if out is None else (out.unsqueeze(1) if out.dim() == 3 else out)
    pd, dps, drs = _node_planes(field, d, P, rows, N, D, "first_mask out")
    if lam is None:
        lam = hm.element(field, 1)[None] if csh.dim() == 2 else _scl.lagrange_basis(field, m)
    lam = _scl._host(lam).reshape(m, L)
    cm = torch.empty(N, L, dtype=torch.int64, device=D.device) if cmod is None else cmod
    _scl._want(cm, (N, L), "first_mask cmod", D)
    if not cm.is_contiguous():
        raise _scl.SclError(_scl.ERR_BAD_ARG, "first_mask cmod: must be contiguous")
    st = _scl._status(N, D, status, "first_mask")
    pc, sc = _scl._dev_rows(D)
    _chk(lib.scl_cmp_first_mask(field, pd, _z(dps), _z(drs), C.c_void_p(cm.data_ptr()), C.c_void_p(st.data_ptr()), pc, _z(sc), _scl._hp(lam), _z(m),
                                pb, _z(bps), _z(brs), pr, _z(rps), _z(rrs), _z(w), _z(B), _z(rows), _z(N), C.c_uint(flags), _scl._stream()))
    return (out if out is not None else d), cm, st


def level_mask(field, nodes, r2, flags: int = 0, out=None):
    """d: a later level (scl_cmp_level_mask).  nodes [2 cnt][rows][N][L], cnt >= 2 nodes; r2 and d node arrays of ceil(cnt / 2)
    nodes, [P][rows][N][L] with P = 2 ceil(cnt / 2), or 1 under LT_ONLY (cnt == 2)."""
    L = _scl.limbs(field)
    if nodes.dim() == 3:
        nodes = nodes.unsqueeze(1)
    if nodes.dim() != 4 or nodes.shape[0] % 2:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"level_mask nodes: shape {tuple(nodes.shape)}, expected [2 cnt][rows][N][{L}]")
    cnt, rows, N = nodes.shape[0] // 2, nodes.shape[1], nodes.shape[2]
    P = None if cnt < 2 else 1 if flags & LT_ONLY else 2 * ((cnt + 1) // 2)  # (cnt < 2: the library says so)
    pn, nps, nrs = _node_planes(field, nodes, 2 * cnt, rows, N, None, "level_mask nodes")
    if r2.dim() == 3:
        r2 = r2.unsqueeze(1)
    pr, rps, rrs = _node_planes(field, r2, P, rows, N, nodes, "level_mask r2")
    d = torch.empty(P or 1, rows, N, L, dtype=torch.int64, device=nodes.device) if out is None else (out.unsqueeze(1) if out.dim() == 3 else out)
    pd, dps, drs = _node_planes(field, d, P, rows, N, nodes, "level_mask out")
    _chk(lib.scl_cmp_level_mask(field, pd, _z(dps), _z(drs), pn, _z(nps), _z(nrs), pr, _z(rps), _z(rrs), _z(cnt), _z(rows), _z(N), C.c_uint(flags),
                                _scl._stream()))
    return out if out is not None else d


def finish(field, lt, cmod, status, rlow, x, w: int, what: int, out=None):
    """a = cmod - rlow + 2^w lt; MOD: a, TRUNC: (x - a) 2^-w, LTZ: -(x - a) 2^-w, for every row of lt, rlow, x [rows][N][L] (or
    [N][L]) in one launch (scl_cmp_finish).  A column whose status is set is 0 in every row.  x may be None for MOD; `out` may be
    x, rlow or lt (in place)."""
    L = _scl.limbs(field)
    T, R = _scl._rows3(field, lt, "finish lt"), _scl._rows3(field, rlow, "finish rlow")
    rows, N, _ = T.shape
    _scl._want(R, (rows, N, L), "finish rlow", T)
    _scl._want(cmod, (N, L), "finish cmod", T)
    if not cmod.is_contiguous():
        raise _scl.SclError(_scl.ERR_BAD_ARG, "finish cmod: must be contiguous")
    st = _scl._status(N, T, status, "finish")
    if x is None:
        px, sx = None, N
    else:
        X = _scl._rows3(field, x, "finish x")
        _scl._want(X, (rows, N, L), "finish x", T)
        px, sx = _scl._dev_rows(X)
    y = torch.empty(rows, N, L, dtype=torch.int64, device=T.device) if out is None else _scl._rows3(field, out, "finish out")
    _scl._want(y, (rows, N, L), "finish out", T)
    (py, sy), (pt, stt), (pr, sr) = _scl._dev_rows(y), _scl._dev_rows(T), _scl._dev_rows(R)
    _chk(lib.scl_cmp_finish(field, py, _z(sy), pt, _z(stt), C.c_void_p(cmod.data_ptr()), C.c_void_p(st.data_ptr()), pr, _z(sr), px, _z(sx), _z(w),
                            C.c_int(what), _z(rows), _z(N), _scl._stream()))
    if out is not None:
        return out
    return y[0] if lt.dim() == 2 else y


def bit_lt(field, csh, bits, R_lo, R_hi, w: int, B: int, lam_t=None, lam_2t=None):
    """The whole tree for all n simulated parties on one device -> (lt [n][N][L], cmod [N][L], status [N]): shares of [c' < r'],
    c' = c mod 2^w of the c that csh [m][N][L] opens under lam_t (default: nodes 1..m at 0), r' = sum_{i<w} 2^i bits[i].

    bits [>= w][n][N][L]; (R_lo, R_hi) [n][>= planes(w) N][L] double sharings, consumed from column 0; lam_2t opens a degree-2t
    sharing from the first len(lam_2t) parties (default: all n).  The steps: first_mask, then for every level hm.mul_finish over
    the whole node array in one call and -- but for the last -- level_mask."""
    from scl_amd import hm
    L = _scl.limbs(field)
    n, N = bits.shape[1], bits.shape[2]
    need = planes(w) * N
    if R_lo.shape[1] < need or R_hi.shape[1] < need or R_lo.shape[0] != n or R_hi.shape[0] != n:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"bit_lt: {need} double sharings for {n} parties needed (planes(w) N), R_lo {tuple(R_lo.shape)}, R_hi {tuple(R_hi.shape)}")
    m2 = n if lam_2t is None else len(lam_2t)
    as_planes = lambda a, P: a.view(n, P, N, L).transpose(0, 1)
    cnt, off, nodes, cmod, status = w, 0, None, None, None
    for level in range(levels(w)):
        out_nodes = (cnt + 1) // 2
        flags = LT_ONLY if out_nodes == 1 else 0
        P = 1 if flags else 2 * out_nodes
        d = torch.empty(n, P * N, L, dtype=torch.int64, device=bits.device)
        r2 = as_planes(R_hi[:, off:off + P * N], P)
        if level == 0:
            _, cmod, status = first_mask(field, csh, bits, r2, w, B, lam=lam_t, flags=flags, out=as_planes(d, P))
        else:
            level_mask(field, as_planes(nodes, 2 * cnt), r2, flags=flags, out=as_planes(d, P))
        nodes = hm.mul_finish(field, d[:m2], R_lo[:, off:off + P * N], lam=lam_2t)
        cnt, off = out_nodes, off + P * N
    return nodes, cmod, status


def _pipeline(field, x, bits, R_lo, R_hi, k: int, w: int, what: int, lam_t, lam_2t):
    from scl_amd import fx
    B = bits.shape[0]
    c, rlow = fx.trunc_mask(field, x, bits, k, w)
    m = x.shape[0] if lam_t is None else len(lam_t)
    lt, cmod, status = bit_lt(field, c[:m], bits, R_lo, R_hi, w, B, lam_t=lam_t, lam_2t=lam_2t)
    return finish(field, lt, cmod, status, rlow, x, w, what, out=rlow), status


def mod2m(field, x, bits, R_lo, R_hi, k: int, w: int, lam_t=None, lam_2t=None):
    """(y, status): shares of x mod 2^w, exactly.  x [n][N][L]: the parties' degree-t shares of N signed k-bit values; bits
    [B][n][N][L], B >= k shared random bits per value; (R_lo, R_hi) [n][>= planes(w) N][L]; lam_t opens a degree-t sharing from
    the first len(lam_t) parties, lam_2t a degree-2t sharing (defaults: all n).  fx.trunc_mask, bit_lt, finish."""
    return _pipeline(field, x, bits, R_lo, R_hi, k, w, MOD, lam_t, lam_2t)


def trunc(field, x, bits, R_lo, R_hi, k: int, w: int, lam_t=None, lam_2t=None):
    """(y, status): shares of floor(x / 2^w), exactly -- never plus one.  Operands as mod2m."""
    return _pipeline(field, x, bits, R_lo, R_hi, k, w, TRUNC, lam_t, lam_2t)


def ltz(field, x, bits, R_lo, R_hi, k: int, lam_t=None, lam_2t=None):
    """(y, status): shares of [x < 0], 1 or 0, for signed k-bit values: the exact truncation by w = k - 1 bits, negated.
    Operands as mod2m; planes(k - 1) N double sharings."""
    return _pipeline(field, x, bits, R_lo, R_hi, k, k - 1, LTZ, lam_t, lam_2t)


def lt(field, x, y, bits, R_lo, R_hi, k: int, lam_t=None, lam_2t=None):
    """(z, status): shares of [x < y] for signed k-bit values x, y [n][N][L]: ltz of x - y, a signed (k + 1)-bit value, so bits
    holds B >= k + 1 planes and planes(k) N double sharings are consumed."""
    return ltz(field, _scl.ew(field, _scl.SUB, x, y), bits, R_lo, R_hi, k + 1, lam_t=lam_t, lam_2t=lam_2t)
