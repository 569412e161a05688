"""scl_amd.ip -- Python harness over libscl_hip_ip.so, inner and matrix products of Shamir sharings at one opening each
(include/scl_hip_ip.h).

The Damgard-Nielsen multiplication of scl_amd.hm opens one value per product; a whole sum of products costs the same single
opening: [d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t.  `dot_mask` is that local step for inner products, `matmul_mask` for a batch
of small matrix products, both over many independent instances (one per column).  The open-and-subtract that follows is
`scl_amd.hm.mul_finish`.  Plumbing only, like scl_amd itself: torch device buffers and the current HIP stream go to the C ABI;
there is no CPU or torch fallback.  Tensors are those of scl_amd: int64 limbs, SoA rows `[...][N][limb]`.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_ip.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_ip")


# argtypes / restype of every entry point from the prototypes of include/scl_hip_ip.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_ip.h", "scl_ip_", "SCL_IP_ABI_VERSION", "scl_amd.ip")


_chk = _scl._checker(lib.scl_ip_last_error)


def matmul_tile(field):
    """(TI, TL): the output tile a lane of matmul_mask owns for this field (scl_ip_matmul_tile)"""
    ti, tl = C.c_int(0), C.c_int(0)
    lib.scl_ip_matmul_tile(field, C.byref(ti), C.byref(tl))
    if ti.value == 0:
        raise _scl.SclError(_scl.ERR_BAD_ARG, "unknown field tag")
    return ti.value, tl.value


def _view(field, t: torch.Tensor, lead: int, what: str, shape=None):
    """an operand [d_0]..[d_{lead-1}][N][L] whose columns are dense -> (pointer, the lead strides in elements); the stride of an
    axis of extent 1 is reported as 0 (it addresses nothing)"""
    L = _scl.limbs(field)
    if t.dtype != torch.int64 or not t.is_cuda:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: expected int64 limbs on the GPU")
    if t.dim() != lead + 2 or t.shape[-1] != L or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{what}: shape {tuple(t.shape)}, expected "
                            f"{tuple(shape) if shape is not None else '%d leading axes, then [N][%d]' % (lead, L)}")
    N = t.shape[-2]
    if t.numel() and ((L > 1 and t.stride(-1) != 1) or (N > 1 and t.stride(-2) != L) or any(t.stride(i) % L for i in range(lead))):
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: columns must be dense (row, term and batch pitches are allowed)")
    return C.c_void_p(t.data_ptr()), [t.stride(i) // L if t.shape[i] > 1 else 0 for i in range(lead)]


def dot_mask(field, x, y, r2=None, out=None):
    """[d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t, one launch and one reduction per F::ACC_TERMS terms (scl_ip_dot_mask).  x and y
    are [terms][rows][N][L] (or [terms][N][L]: one row), possibly strided views -- any term pitch, x may be y (sums of squares);
    r2 [rows][N][L] (or [N][L]) or None: a plain sum of products.  x, y and r2 share one row pitch; `out` may be r2 (in place).
    The open-and-subtract that follows is scl_amd.hm.mul_finish(field, d, R_t)."""
    L = _scl.limbs(field)
    single = x.dim() == 3
    X, Y = (x.unsqueeze(1), y.unsqueeze(1)) if single else (x, y)
    if X.dim() != 4:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"dot_mask x: shape {tuple(x.shape)}, expected [terms][rows][N][{L}] or [terms][N][{L}]")
    terms, rows, N, _ = X.shape
    px, (xts, xrs) = _view(field, X, 2, "dot_mask x")
    py, (yts, yrs) = _view(field, Y, 2, "dot_mask y", X.shape)
    ops = [("x", xrs), ("y", yrs)]
    pr = None
    if r2 is not None:
        R = r2.unsqueeze(0) if r2.dim() == 2 else r2
        pr, (rrs,) = _view(field, R, 1, "dot_mask r2", (rows, N, L))
        ops.append(("r2", rrs))
    if out is None:
        d = torch.empty(rows, N, L, dtype=torch.int64, device=x.device)
    else:
        d = out.unsqueeze(0) if out.dim() == 2 else out
    pd, (drs,) = _view(field, d, 1, "dot_mask out", (rows, N, L))
    for nm, t in (("y", y), ("r2", r2), ("out", d)):
        if t is not None and t.device != x.device:
            raise _scl.SclError(_scl.ERR_BAD_ARG, f"dot_mask {nm}: on {t.device}, expected {x.device}")
    if rows > 1 and any(s != xrs for _, s in ops):
        raise _scl.SclError(_scl.ERR_BAD_ARG, "dot_mask: row strides " + ", ".join(f"{nm} {s}" for nm, s in ops) + " (x, y and r2 share op_stride)")
    # one row has no row stride: N stands in.  More rows pass the tensors' own strides, whatever they are -- a row stride below
    # N (an expanded operand has 0) is the library's to refuse, never to be rounded up here
    op_stride, d_stride = (xrs, drs) if rows > 1 else (max(N, 1), max(N, 1))
    _chk(lib.scl_ip_dot_mask(field, pd, C.c_size_t(d_stride), px, C.c_size_t(xts), py, C.c_size_t(yts), pr, C.c_size_t(op_stride),
                             C.c_size_t(terms), C.c_size_t(rows), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out
    return d[0] if single else d


def _matrix(field, t, what, shape):
    """[batch][p][q][N][L] -> (pointer, entry stride, batch stride): entry (i, j) at (i q + j) * stride, so the p axis must step
    by q entries"""
    ptr, (bs, ps, qs) = _view(field, t, 3, what, shape)
    p, q, N = shape[1], shape[2], shape[3]
    es = qs if q > 1 else (ps if p > 1 else max(N, 1))
    if p > 1 and q > 1 and ps != q * qs:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: the matrices must be row-major (row pitch {ps}, expected {q} entries of pitch {qs})")
    return ptr, es, bs


def matmul_mask(field, X, Y, r2=None, out=None):
    """[D]_2t = [X]_t [Y]_t + [R]_2t for a batch of small matrix products over N independent instances (scl_ip_matmul_mask):
    X [batch][a][K][N][L] (or [a][K][N][L]), Y [batch][K][b][N][L], r2 and the result [batch][a][b][N][L]; r2 None: no addend;
    `out` may be r2 (in place).  Row-major matrices with any entry and batch pitch.  A lane keeps a tile of outputs
    (matmul_tile) in accumulators and reads each operand once per tile.
    The open-and-subtract that follows is scl_amd.hm.mul_finish over the output viewed as a b N columns -- d.reshape(a * b * N, L)
    per party, the parties as rows -- which is a view where the entry pitch equals N."""
    L = _scl.limbs(field)
    single = X.dim() == 4
    if single:
        X, Y = X.unsqueeze(0), Y.unsqueeze(0)
        r2 = None if r2 is None else r2.unsqueeze(0)
        D = None if out is None else out.unsqueeze(0)
    else:
        D = out
    if X.dim() != 5 or Y.dim() != 5:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"matmul_mask: shapes {tuple(X.shape)}, {tuple(Y.shape)}, expected [batch][a][K][N][{L}] and [batch][K][b][N][{L}]")
    batch, a, K, N, _ = X.shape
    b = Y.shape[2]
    px, xs, xbs = _matrix(field, X, "matmul_mask X", (batch, a, K, N, L))
    py, ys, ybs = _matrix(field, Y, "matmul_mask Y", (batch, K, b, N, L))
    pr, rs, rbs = (None, 0, 0) if r2 is None else _matrix(field, r2, "matmul_mask r2", (batch, a, b, N, L))
    if D is None:
        D = torch.empty(batch, a, b, N, L, dtype=torch.int64, device=X.device)
    pd, ds, dbs = _matrix(field, D, "matmul_mask out", (batch, a, b, N, L))
    for nm, t in (("Y", Y), ("r2", r2), ("out", D)):
        if t is not None and t.device != X.device:
            raise _scl.SclError(_scl.ERR_BAD_ARG, f"matmul_mask {nm}: on {t.device}, expected {X.device}")
    _chk(lib.scl_ip_matmul_mask(field, pd, C.c_size_t(ds), C.c_size_t(dbs), px, C.c_size_t(xs), C.c_size_t(xbs), py, C.c_size_t(ys),
                                C.c_size_t(ybs), pr, C.c_size_t(rs), C.c_size_t(rbs), C.c_size_t(a), C.c_size_t(K), C.c_size_t(b),
                                C.c_size_t(batch), C.c_size_t(N), _scl._stream()))
    if out is not None:
        return out
    return D[0] if single else D
