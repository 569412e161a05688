"""scl_amd.rb -- Python harness over libscl_hip_rb.so, random shared bits (include/scl_hip_rb.h).

Comparison, truncation, bit decomposition and fixed-point arithmetic over Shamir sharings consume shared random bits.  The
honest-majority construction: take a random [r]_t, square it, open u = r^2, and set [b]_t = ([r]_t / sqrt(u) + 1) / 2.  `sqrt` is
the batched modular square root with a status byte per element, `bits_finish` the fused last step for every party's row at once,
`random_bits` the whole local pipeline for all simulated parties on one device, over scl_amd.hm.  Plumbing only, like scl_amd
itself: torch device buffers and the current HIP stream go to the C ABI; there is no CPU or torch fallback.  Tensors are those of
scl_amd: int64 limbs, SoA rows `[rows][N][limb]`; a status is one uint8 per element or column.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_rb.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_rb")

ODD_ROOT = 1     # SCL_RB_ODD_ROOT: the root with an odd integer value instead of the even one
INVERSE = 2      # SCL_RB_INVERSE: 1/root instead of root
STATUS_OK, STATUS_ZERO, STATUS_NONRESIDUE = 0, 1, 2


# argtypes / restype of every entry point from the prototypes of include/scl_hip_rb.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_rb.h", "scl_rb_", "SCL_RB_ABI_VERSION", "scl_amd.rb")


_chk = _scl._checker(lib.scl_rb_last_error)


def sqrt(field, a, flags: int = 0, out=None, status=None):
    """(root, status) of a [N][L] (scl_rb_sqrt): the root whose integer value is even (ODD_ROOT: the odd one; INVERSE: its
    inverse) and one status byte per element -- 0 ok, 1 the input was zero (root 0), 2 a non-residue (0 is written).  `out` may
    be `a` (in place)."""
    L = _scl.limbs(field)
    N = a.shape[0]
    _scl._want(a, (N, L), "sqrt a")
    out = torch.empty_like(a) if out is None else _scl._want(out, (N, L), "sqrt out", a)
    st = _scl._status(N, a, status, "sqrt")
    _chk(lib.scl_rb_sqrt(field, _scl._dev(out), C.c_void_p(st.data_ptr()), _scl._dev(a), C.c_size_t(N), C.c_uint(flags), _scl._stream()))
    return out, st


def bits_finish(field, u, r, out=None, status=None):
    """(b, status): b[i][s] = (r[i][s] / root(u[s]) + 1) / 2 for every row of r [rows][N][L] (or [N][L]: one row), u [N][L] the
    opened squares (scl_rb_bits_finish).  One status byte per column; a column whose status is not 0 is 0 in every row.  `out`
    may be `r` (in place)."""
    L = _scl.limbs(field)
    R = r.unsqueeze(0) if r.dim() == 2 else r
    if R.dim() != 3 or R.dtype != torch.int64:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"bits_finish r: shape {tuple(r.shape)}, expected [rows][N][{L}] or [N][{L}] int64 limbs")
    rows, N, _ = R.shape
    _scl._want(R, (rows, N, L), "bits_finish r")
    _scl._want(u, (N, L), "bits_finish u", R)
    if out is None:
        B = torch.empty(rows, N, L, dtype=torch.int64, device=R.device)
    else:
        B = _scl._want(out.unsqueeze(0) if out.dim() == 2 else out, (rows, N, L), "bits_finish out", R)
    st = _scl._status(N, R, status, "bits_finish")
    (pb, sb), (pr, sr) = _scl._dev_rows(B), _scl._dev_rows(R)
    _chk(lib.scl_rb_bits_finish(field, pb, C.c_size_t(sb), C.c_void_p(st.data_ptr()), _scl._dev(u), pr, C.c_size_t(sr), C.c_size_t(rows),
                                C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out, st
    return (B[0] if r.dim() == 2 else B), st


def random_bits(field, r, R_lo, R_hi, lam_2t=None, lam_t=None):
    """The local pipeline of a batch of random shared bits for all n simulated parties on one device -> (b, status).

    r [n][N][L]: the parties' degree-t shares of N random values; (R_lo, R_hi) [n][N][L]: one double sharing per column, degrees
    t and 2t (scl_amd.hm.double_share and apply_matrix deal both).  lam_2t: the Lagrange basis that opens a degree-2t sharing from
    the n shares (default: the nodes 1..n at 0); lam_t: the basis over the first len(lam_t) parties that opens a degree-t sharing
    (default: all n).  The steps: hm.mul_mask(r, r, R_hi), hm.mul_finish -- [r^2]_t --, shamir_recover -- u = r^2 in the open --,
    bits_finish.  b [n][N][L] are the parties' degree-t shares of N bits; status [N] flags the columns to discard (r = 0)."""
    from scl_amd import hm
    n = r.shape[0]
    d = hm.mul_mask(field, r, r, R_hi)
    sq = hm.mul_finish(field, d, R_lo, lam=lam_2t)
    m = n if lam_t is None else len(lam_t)
    u = _scl.shamir_recover(field, sq[:m], lam=lam_t)
    return bits_finish(field, u, r)
