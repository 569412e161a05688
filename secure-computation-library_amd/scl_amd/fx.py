"""scl_amd.fx -- Python harness over libscl_hip_fx.so, fixed-point arithmetic over Shamir sharings (include/scl_hip_fx.h).

A fixed-point product [x][y] carries 2f fractional bits; the probabilistic truncation of Catrina and de Hoogh drops f of them with
one mask, one opening and one local finish, and consumes B = k + kappa shared random bits (scl_amd.rb) per value.  `compose` is the
bounded random value sum 2^i [b_i] that masks are made of, `trunc_mask` the mask [c] = [x] + 2^(k-1) + [r] with [r'] beside it,
`trunc_finish` the opening, c mod 2^shift as an integer and [y] = ([x] + [r'] - c') 2^-shift in one launch, `trunc_pr` the whole
local pipeline for all simulated parties on one device and `mul_trunc` the fixed-point product over scl_amd.hm.  Plumbing only,
like scl_amd itself: torch device buffers and the current HIP stream go to the C ABI; there is no CPU or torch fallback.  Tensors
are those of scl_amd: int64 limbs, SoA rows `[rows][N][L]`; bit planes are `[B][rows][N][L]`, planes and rows any pitch apart -- the
output b [rows][B N][L] of one `scl_amd.rb.random_bits` call is `b.view(rows, B, N, L).transpose(0, 1)`, without a copy; a status is
one uint8 per column.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_fx.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_fx")

STATUS_OK, STATUS_RANGE = 0, 1


# argtypes / restype of every entry point from the prototypes of include/scl_hip_fx.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_fx.h", "scl_fx_", "SCL_FX_ABI_VERSION", "scl_amd.fx")


_chk = _scl._checker(lib.scl_fx_last_error)


def max_bits(field) -> int:
    """|p| - 2, the largest bit count B (scl_fx_max_bits); 0 for a tag the library refuses"""
    return int(lib.scl_fx_max_bits(field))


def _planes(field, bits: torch.Tensor, rows, N, like, what: str):
    """(pointer, plane stride, row stride, B) of bit planes [B][rows][N][L] (or [B][N][L]: one row)"""
    L = _scl.limbs(field)
    if bits.dtype != torch.int64:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: dtype {bits.dtype}, expected int64 limbs")
    if bits.dim() == 3:
        bits = bits.unsqueeze(1)
    if bits.dim() != 4 or bits.shape[3] != L or (rows is not None and tuple(bits.shape[1:3]) != (rows, N)):
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{what}: shape {tuple(bits.shape)}, expected [B][{rows}][{N}][{L}]")
    if not bits.is_cuda or (like is not None and bits.device != like.device):
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: on {bits.device}, expected the operands' GPU")
    B, R, n, _ = bits.shape
    if n and ((L > 1 and bits.stride(3) != 1) or (n > 1 and bits.stride(2) != L) or (B > 1 and (bits.stride(0) % L or bits.stride(0) < n * L)) or
              (R > 1 and (bits.stride(1) % L or bits.stride(1) < n * L))):
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: the rows of a plane must be dense (plane and row pitches are allowed)")
    return C.c_void_p(bits.data_ptr()), (bits.stride(0) // L if B > 1 else max(n, 1)), (bits.stride(1) // L if R > 1 else max(n, 1)), B


def compose(field, bits, out=None):
    """out[r][s] = sum_i 2^i bits[i][r][s] (scl_fx_compose): bits [B][rows][N][L] (or [B][N][L]: one row) -> [rows][N][L] (or
    [N][L])."""
    L = _scl.limbs(field)
    one_row = bits.dim() == 3
    pb, ps, rs, B = _planes(field, bits, None, None, None, "compose bits")
    rows, N = (1, bits.shape[1]) if one_row else (bits.shape[1], bits.shape[2])
    o = torch.empty(rows, N, L, dtype=torch.int64, device=bits.device) if out is None else _scl._rows3(field, out, "compose out")
    _scl._want(o, (rows, N, L), "compose out", bits)
    po, so = _scl._dev_rows(o)
    _chk(lib.scl_fx_compose(field, po, C.c_size_t(so), pb, C.c_size_t(ps), C.c_size_t(rs), C.c_size_t(B), C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out
    return o[0] if one_row else o


def trunc_mask(field, x, bits, k: int, shift: int, out=None, rlow=None):
    """(c, rlow): c = x + 2^(k-1) + r and rlow = r', r = sum_{i<B} 2^i bits[i], r' its lowest `shift` planes, in one launch
    (scl_fx_trunc_mask).  x [rows][N][L] (or [N][L]: one row), bits [B][rows][N][L] (or [B][N][L]); `out` may be x (in place)."""
    X = _scl._rows3(field, x, "trunc_mask x")
    rows, N, L = X.shape
    pb, ps, rs, B = _planes(field, bits, rows, N, X, "trunc_mask bits")
    c = torch.empty(rows, N, L, dtype=torch.int64, device=X.device) if out is None else _scl._rows3(field, out, "trunc_mask out")
    lo = torch.empty(rows, N, L, dtype=torch.int64, device=X.device) if rlow is None else _scl._rows3(field, rlow, "trunc_mask rlow")
    _scl._want(c, (rows, N, L), "trunc_mask out", X)
    _scl._want(lo, (rows, N, L), "trunc_mask rlow", X)
    (pc, sc), (pl, sl), (px, sx) = _scl._dev_rows(c), _scl._dev_rows(lo), _scl._dev_rows(X)
    _chk(lib.scl_fx_trunc_mask(field, pc, C.c_size_t(sc), pl, C.c_size_t(sl), px, C.c_size_t(sx), pb, C.c_size_t(ps), C.c_size_t(rs), C.c_size_t(k),
                               C.c_size_t(shift), C.c_size_t(B), C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    one = x.dim() == 2
    return (out if out is not None else (c[0] if one else c)), (rlow if rlow is not None else (lo[0] if one else lo))


def trunc_finish(field, csh, x, rlow, shift: int, B: int, lam=None, out=None, status=None):
    """(y, status): c opened from csh [m][N][L], the m <= 64 shares of c (or [N][L]: c already opened), lam their Lagrange basis
    (default: nodes 1..m at 0; for an opened c: one); c' = c mod 2^shift and y = (x + rlow - c') 2^-shift for every row of
    x, rlow [rows][N][L] (or [N][L]) in one launch (scl_fx_trunc_finish).  One status byte per column: 1 where c >= 2^(B+1), and
    that column is 0 in every row.  `out` may be x or rlow (in place)."""
    from scl_amd import hm
    L = _scl.limbs(field)
    D, X, R = _scl._rows3(field, csh, "trunc_finish csh"), _scl._rows3(field, x, "trunc_finish x"), _scl._rows3(field, rlow, "trunc_finish rlow")
    m, N, _ = D.shape
    rows = X.shape[0]
    _scl._want(X, (rows, N, L), "trunc_finish x", D)
    _scl._want(R, (rows, N, L), "trunc_finish rlow", D)
    if lam is None:
        lam = hm.element(field, 1)[None] if csh.dim() == 2 else _scl.lagrange_basis(field, m)
    lam = _scl._host(lam).reshape(m, L)
    y = torch.empty(rows, N, L, dtype=torch.int64, device=D.device) if out is None else _scl._rows3(field, out, "trunc_finish out")
    _scl._want(y, (rows, N, L), "trunc_finish out", D)
    st = _scl._status(N, D, status, "trunc_finish")
    (py, sy), (pd, sd), (px, sx), (pr, sr) = _scl._dev_rows(y), _scl._dev_rows(D), _scl._dev_rows(X), _scl._dev_rows(R)
    _chk(lib.scl_fx_trunc_finish(field, py, C.c_size_t(sy), C.c_void_p(st.data_ptr()), pd, C.c_size_t(sd), _scl._hp(lam), C.c_size_t(m), px, C.c_size_t(sx),
                                 pr, C.c_size_t(sr), C.c_size_t(shift), C.c_size_t(B), C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out, st
    return (y[0] if x.dim() == 2 else y), st


def trunc_pr(field, x, bits, k: int, shift: int, lam=None):
    """The local pipeline of a probabilistic truncation for all n simulated parties on one device -> (y, status).

    x [n][N][L]: the parties' degree-t shares of N signed k-bit values; bits [B][n][N][L]: their shares of B >= k random bits per
    value.  lam: the basis over the first len(lam) parties that opens a degree-t sharing (default: all n).  The steps: trunc_mask,
    then trunc_finish on the first len(lam) rows of c.  y [n][N][L] are shares of floor(x / 2^shift) or that plus one; status [N]
    flags the columns whose opened c was out of range."""
    B = bits.shape[0]
    c, rlow = trunc_mask(field, x, bits, k, shift)
    m = x.shape[0] if lam is None else len(lam)
    return trunc_finish(field, c[:m], x, rlow, shift, B, lam=lam, out=rlow)


def mul_trunc(field, x, y, R_lo, R_hi, bits, k: int, shift: int, lam_2t=None, lam_t=None):
    """The fixed-point product -> (z, status): hm.mul_mask(x, y, R_hi), hm.mul_finish -- [x y]_t, 2 shift fractional bits --, then
    trunc_pr drops `shift` of them.  x, y [n][N][L] fixed-point encodings whose product is a signed k-bit value; (R_lo, R_hi) one
    double sharing per column; bits [B][n][N][L]; lam_2t opens a degree-2t sharing from the n shares, lam_t a degree-t sharing
    from the first len(lam_t) (defaults: the nodes 1..n at 0)."""
    from scl_amd import hm
    d = hm.mul_mask(field, x, y, R_hi)
    z = hm.mul_finish(field, d, R_lo, lam=lam_2t)
    return trunc_pr(field, z, bits, k, shift, lam=lam_t)
