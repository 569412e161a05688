"""scl_amd.mpc -- Python harness over libscl_hip_mpc.so, the protocol extension beside the engine (include/scl_hip_mpc.h).

Beaver multiplication of shared vectors (the reference's BeaverMul, test/scl/protocol/beaver.h:31-70): `beaver_mask` before the
open step, `beaver_finish` after it, one kernel launch each.  Plumbing only, like scl_amd itself: torch device buffers and the
current HIP stream go to the C ABI; there is no CPU or torch fallback.  Tensors are those of scl_amd: int64 limbs, trailing
dimension `limbs(field)`, a share matrix SoA `[party][secret][limb]` whose rows may sit a pitch apart.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_mpc.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_mpc")


# argtypes / restype of every entry point from the prototypes of include/scl_hip_mpc.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_mpc.h", "scl_mpc_", "SCL_MPC_ABI_VERSION", "scl_amd.mpc")


_chk = _scl._checker(lib.scl_mpc_last_error)


def _same_rows(field, named):
    """device pointers of operands that share one shape and one row stride"""
    first_name, first = named[0]
    ptrs, stride = [], None
    for name, t in named:
        if tuple(t.shape) != tuple(first.shape):
            raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{name}: shape {tuple(t.shape)}, {first_name} has {tuple(first.shape)}")
        if t.device != first.device:
            raise _scl.SclError(_scl.ERR_BAD_ARG, f"{name}: on {t.device}, {first_name} on {first.device}")
        p, s = _scl._dev_rows(t)
        if stride is not None and s != stride:
            raise _scl.SclError(_scl.ERR_BAD_ARG, f"{name}: row stride {s}, {first_name} has {stride} (operands share op_stride)")
        stride = s
        ptrs.append(p)
    return ptrs, stride


def beaver_mask(field, x, y, a, b, out=None):
    """[e] = [x] - [a] and [d] = [y] - [b] in one launch (scl_mpc_beaver_mask).  Operands [rows][N][L] (or [N][L]: one row);
    returns (e_rows, d_rows), the two halves of ONE tensor [2 rows][N][L] -- `out`, if given -- each shaped like the operands:
    with one row the tensor is the reference's packet, e then d; with rows = n the halves go to shamir_recover /
    additive_recover as they lie."""
    vec = x.dim() == 2
    ops = [(n, _scl._rows3(field, t, "beaver_mask " + n)) for n, t in (("x", x), ("y", y), ("a", a), ("b", b))]
    rows, N, L = ops[0][1].shape
    ptrs, stride = _same_rows(field, ops)
    if out is None:
        out = torch.empty(2 * rows, N, L, dtype=torch.int64, device=x.device)
    else:
        _scl._want(out, (2 * rows, N, L), "beaver_mask out", x)
    po, so = _scl._dev_rows(out)
    _chk(lib.scl_mpc_beaver_mask(field, po, C.c_size_t(so), *ptrs, C.c_size_t(stride), C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    return (out[0], out[1]) if vec else (out[:rows], out[rows:])


def beaver_finish(field, e, d, a, b, c, ed_rows, out=None):
    """[z] = e [b] + d [a] + [c], plus e d in the first `ed_rows` rows (scl_mpc_beaver_finish).  e, d: the opened values [N][L];
    a, b, c: [rows][N][L] (or [N][L]: one row).  Shamir: ed_rows = rows; additive: 1 where row 0 is party 0, else 0.  `out` may be
    a, b or c (in place)."""
    vec = a.dim() == 2
    ops = [(n, _scl._rows3(field, t, "beaver_finish " + n)) for n, t in (("a", a), ("b", b), ("c", c))]
    rows, N, L = ops[0][1].shape
    _scl._want(e, (N, L), "beaver_finish e", a)
    _scl._want(d, (N, L), "beaver_finish d", a)
    ptrs, stride = _same_rows(field, ops)
    if out is None:
        z = torch.empty(rows, N, L, dtype=torch.int64, device=a.device)
    else:
        z = _scl._rows3(field, out, "beaver_finish out")
        _scl._want(z, (rows, N, L), "beaver_finish out", a)
    pz, sz = _scl._dev_rows(z)
    _chk(lib.scl_mpc_beaver_finish(field, pz, C.c_size_t(sz), _scl._dev(e), _scl._dev(d), *ptrs, C.c_size_t(stride), C.c_size_t(rows),
                                   C.c_size_t(int(ed_rows)), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out
    return z[0] if vec else z
