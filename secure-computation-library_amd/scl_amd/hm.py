"""scl_amd.hm -- Python harness over libscl_hip_hm.so, honest-majority multiplication beside the engine (include/scl_hip_hm.h).

Damgard-Nielsen multiplication for Shamir sharings among n > 2t parties, without a dealer: `double_share` deals one party's
double sharings ([r]_t, [r]_2t) in the reference's PRG order, `apply_matrix` applies a small matrix -- the hyper-invertible
matrix of `hyper_invertible` -- across the sharings a party received (the extraction), `mul_mask` and `mul_finish` are the two
local steps of a product on either side of the open.  Plumbing only, like scl_amd itself: torch device buffers and the current
HIP stream go to the C ABI; there is no CPU or torch fallback.  Tensors are those of scl_amd: int64 limbs, a share matrix SoA
`[party][secret][limb]`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import scl_amd as _scl  # the engine first: libscl_hip_hm.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_hm")

TWO_PASS = 1                # flags bit 0 of double_share


# argtypes / restype of every entry point from the prototypes of include/scl_hip_hm.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_hm.h", "scl_hm_", "SCL_HM_ABI_VERSION", "scl_amd.hm")


_chk = _scl._checker(lib.scl_hm_last_error)


def double_blocks(field, n: int, t: int) -> int:
    """AES blocks one double sharing consumes (B of include/scl_hip_hm.h).  Raises for arguments the deal call refuses."""
    B = lib.scl_hm_double_blocks(field, n, t)
    if B == 0:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"double_blocks: field {field:#x}, n = {n}, t = {t} is not a case the dealer accepts")
    return B


def double_scratch_bytes(field, N: int, n: int, t: int, flags: int = 0) -> int:
    """bytes of scratch double_share needs for this case: 0 where the fused kernel deals it"""
    return lib.scl_hm_double_scratch_bytes(field, N, n, t, flags)


def double_share(field, N: int, t: int, n: int, seed: bytes, counter0: int = 0, out=None, scratch=None, flags: int = 0, device="cuda"):
    """N double sharings of one dealer at the nodes 1..n (scl_hm_double_share_prg): returns (lo, hi), each [n][N][L] -- the
    degree-t and the degree-2t shares of the same N secrets.  `out`: two such tensors of one row stride.  Where the case takes the
    two-pass path (double_scratch_bytes > 0) the scratch is `scratch` -- an int64 tensor of at least that many bytes -- or
    allocated here; pass one when the call is captured into a graph."""
    L = _scl.limbs(field)
    if out is None:
        both = torch.empty(2, n, N, L, dtype=torch.int64, device=device)
        out = (both[0], both[1])
    if len(out) != 2:
        raise _scl.SclError(_scl.ERR_BAD_ARG, "double_share: out is the two matrices (lo, hi)")
    for name, m in zip(("lo", "hi"), out):
        _scl._want(m, (n, N, L), f"double_share out {name}", out[0])
    (plo, stride), (phi, s2) = _scl._dev_rows(out[0]), _scl._dev_rows(out[1])
    if s2 != stride:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"double_share out hi: row stride {s2}, lo has {stride} (the matrices share one stride)")
    need = double_scratch_bytes(field, N, n, t, flags)
    sp = None
    if need:
        if scratch is None:
            scratch = torch.empty(need // 8, dtype=torch.int64, device=out[0].device)
        if scratch.dtype != torch.int64 or scratch.numel() * 8 < need or scratch.device != out[0].device:
            raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"double_share: scratch must be an int64 tensor of at least {need} bytes on {out[0].device}")
        sp = _scl._dev(scratch)
    _chk(lib.scl_hm_double_share_prg(field, plo, phi, C.c_size_t(stride), C.c_size_t(N), C.c_size_t(t), C.c_size_t(n), seed,
                                     C.c_size_t(len(seed)), C.c_uint64(counter0), sp, C.c_uint(flags), _scl._stream()))
    return tuple(out)


def _modulus(field):
    """(p, R): the prime and the Montgomery radix of the field's canonical form (R = 1: plain residues); None for GF(2^128)"""
    if field == _scl.M61:
        return 2 ** 61 - 1, 1
    if field == _scl.M127:
        return 2 ** 127 - 1, 1
    if field == _scl.MONT128:
        return _scl.mont128_prime(), 2 ** 128
    if field == _scl.SECP256K1_SCALAR:
        return 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141, 2 ** 256
    if field == _scl.SECP256K1_FIELD:
        return 2 ** 256 - 2 ** 32 - 977, 2 ** 256
    if field == _scl.GF2_128:
        return None
    raise _scl.SclError(_scl.ERR_BAD_ARG, "unknown field tag")


def element(field, value: int) -> np.ndarray:
    """the integer `value` (negative values too) as one canonical element [L]; over GF(2^128) the bit pattern of `value`"""
    L, pr = _scl.limbs(field), _modulus(field)
    v = value % (1 << 128) if pr is None else (value % pr[0]) * pr[1] % pr[0]
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(L)], dtype=np.uint64)


def hyper_invertible(field, rows: int, cols: int, points=None) -> np.ndarray:
    """Matrix::hyperInvertible(rows, cols) (matrix.h:462-475) on the host, [rows][cols][L]: row i is the Lagrange basis of the
    nodes 1..cols at the point -i.  `points`: other evaluation points, as integers (see `element`).  Over GF(2^128) -i = i
    collides with the nodes; there the default points are the bit patterns cols + 1 + i -- this project's choice."""
    if points is None:
        points = [cols + 1 + i for i in range(rows)] if field == _scl.GF2_128 else [-i for i in range(rows)]
    if len(points) != rows:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"hyper_invertible: {len(points)} points for {rows} rows")
    L = _scl.limbs(field)
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols, L), dtype=np.uint64)
    return np.stack([_scl.lagrange_basis(field, cols, None, element(field, int(x))) for x in points])


def _batched(field, t: torch.Tensor, what: str):
    """(pointer, row stride, batch stride, batch, rows, N) of [rows][N][L] or [batch][rows][N][L]; any view whose columns are
    dense: a transposed [dealer][party] pair of leading axes is what the extraction reads"""
    L = _scl.limbs(field)
    if t.dtype != torch.int64 or not t.is_cuda:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: expected int64 limbs on the GPU")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[3] != L:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{what}: shape {tuple(t.shape)}, expected [rows][N][{L}] or [batch][rows][N][{L}]")
    batch, rows, N, _ = t.shape
    if N and ((L > 1 and t.stride(3) != 1) or (N > 1 and t.stride(2) != L) or t.stride(0) % L or t.stride(1) % L or
              (rows > 1 and t.stride(1) < N * L)):
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: rows must be dense (row and batch pitches are allowed)")
    return C.c_void_p(t.data_ptr()), (t.stride(1) // L if rows > 1 else max(N, 1)), (t.stride(0) // L if batch > 1 else 0), batch, rows, N


def apply_matrix(field, M, x, out=None):
    """out[b][k] = sum_i M[k][i] x[b][i] (scl_hm_apply): M [m][n][L] on the device (upload it once), x [n][N][L] or
    [batch][n][N][L]; returns [m][N][L] or [batch][m][N][L].  With dealers' matrices stacked as deals [dealer][party][N][L],
    `apply_matrix(field, M, deals.transpose(0, 1))` extracts for every party in one launch."""
    L = _scl.limbs(field)
    if M.dim() != 3 or M.shape[2] != L or M.dtype != torch.int64:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"apply_matrix M: shape {tuple(M.shape)}, expected [m][n][{L}] int64 limbs")
    m, n = M.shape[0], M.shape[1]
    pm, ldm = _scl._dev_rows(M)
    pi, si, bi, batch, rows, N = _batched(field, x, "apply_matrix x")
    if rows != n:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"apply_matrix: M has {n} columns, x {rows} rows")
    if out is None:
        out = torch.empty((batch, m, N, L) if x.dim() == 4 else (m, N, L), dtype=torch.int64, device=x.device)
    po, so, bo, ob, orows, oN = _batched(field, out, "apply_matrix out")
    if (ob, orows, oN) != (batch, m, N) or out.device != x.device or M.device != x.device:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"apply_matrix out: shape {tuple(out.shape)} on {out.device}, expected batch {batch}, {m} rows, N = {N} on {x.device}")
    _chk(lib.scl_hm_apply(field, po, C.c_size_t(so), C.c_size_t(bo), pi, C.c_size_t(si), C.c_size_t(bi), pm, C.c_size_t(ldm),
                          C.c_size_t(m), C.c_size_t(n), C.c_size_t(batch), C.c_size_t(N), _scl._stream()))
    return out


def mul_mask(field, x, y, r2, out=None):
    """[d]_2t = [x]_t [y]_t + [R]_2t, one product and one reduction per element (scl_hm_mul_mask).  Operands [rows][N][L] (or
    [N][L]: one row) of one row stride; `out` may be r2 (in place)."""
    ops = [(nm, _scl._rows3(field, t, "mul_mask " + nm)) for nm, t in (("x", x), ("y", y), ("r2", r2))]
    rows, N, L = ops[0][1].shape
    ptrs, stride = [], None
    for nm, t in ops:
        _scl._want(t, (rows, N, L), "mul_mask " + nm, ops[0][1])
        p, s = _scl._dev_rows(t)
        if stride is not None and s != stride:
            raise _scl.SclError(_scl.ERR_BAD_ARG, f"mul_mask {nm}: row stride {s}, x has {stride} (operands share op_stride)")
        stride = s
        ptrs.append(p)
    d = torch.empty(rows, N, L, dtype=torch.int64, device=x.device) if out is None else _scl._rows3(field, out, "mul_mask out")
    _scl._want(d, (rows, N, L), "mul_mask out", ops[0][1])
    pd, sd = _scl._dev_rows(d)
    _chk(lib.scl_hm_mul_mask(field, pd, C.c_size_t(sd), *ptrs, C.c_size_t(stride), C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out
    return d[0] if x.dim() == 2 else d


def mul_finish(field, dsh, r, lam=None, out=None):
    """[z]_t = open(d) - [R]_t in one launch (scl_hm_mul_finish): dsh [m][N][L] the m <= 64 shares of d (or [N][L]: d already
    opened), lam their Lagrange basis (default: nodes 1..m at 0; for an opened d: one), r [rows][N][L] (or [N][L]: one row).
    `out` may be r (in place)."""
    L = _scl.limbs(field)
    D, R = _scl._rows3(field, dsh, "mul_finish dsh"), _scl._rows3(field, r, "mul_finish r")
    m, N, _ = D.shape
    rows = R.shape[0]
    _scl._want(R, (rows, N, L), "mul_finish r", D)
    if lam is None:
        lam = element(field, 1)[None] if dsh.dim() == 2 else _scl.lagrange_basis(field, m)
    lam = _scl._host(lam).reshape(m, L)
    z = torch.empty(rows, N, L, dtype=torch.int64, device=D.device) if out is None else _scl._rows3(field, out, "mul_finish out")
    _scl._want(z, (rows, N, L), "mul_finish out", D)
    (pz, sz), (pd, sd), (pr, sr) = _scl._dev_rows(z), _scl._dev_rows(D), _scl._dev_rows(R)
    _chk(lib.scl_hm_mul_finish(field, pz, C.c_size_t(sz), pd, C.c_size_t(sd), _scl._hp(lam), C.c_size_t(m), pr, C.c_size_t(sr),
                               C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out
    return z[0] if r.dim() == 2 else z
