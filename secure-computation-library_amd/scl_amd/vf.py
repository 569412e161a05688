"""scl_amd.vf -- Python harness over libscl_hip_vf.so, batch verification: random linear combinations of sharings along N
(include/scl_hip_vf.h).

The multiplication stack of scl_amd.mpc / prep / hm / ip is passively secure.  To detect a cheating party one checks that N
dealt sharings have the right degree, that N double sharings share one value at both degrees, that N products are right: draw a
public coin, fold the N instances into one with a random linear combination, check that one.  `combine_prg` is the fold with
the coin drawn from the AES-CTR PRG on the device, `combine` the fold with coefficients that come from elsewhere, and
`check_degree` the check of the folded sharing (scl_hip_shamir_recover_detect).  Plumbing only, like scl_amd itself: torch
device buffers and the current HIP stream go to the C ABI; there is no CPU or torch fallback.  Tensors are those of scl_amd:
int64 limbs, SoA rows `[rows][N][limb]`.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_vf.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_vf")

PRG = 1          # SCL_VF_PRG
REPS_MAX = 4


# argtypes / restype of every entry point from the prototypes of include/scl_hip_vf.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_vf.h", "scl_vf_", "SCL_VF_ABI_VERSION", "scl_amd.vf")


_chk = _scl._checker(lib.scl_vf_last_error)


def coin_blocks(field, N: int) -> int:
    """ceil(N * byteSize / 16): the AES blocks one Vector::random(N, prg) consumes (scl_vf_coin_blocks)"""
    if not 0 <= field <= 5:     # the six fields (scl_hip.h); a ring has no Shamir sharing to verify
        raise _scl.SclError(_scl.ERR_BAD_ARG, "unknown field tag")
    return lib.scl_vf_coin_blocks(field, C.c_size_t(N))


def scratch_bytes(field, rows: int, reps: int, N: int, flags: int = 0) -> int:
    return lib.scl_vf_scratch_bytes(field, C.c_size_t(rows), C.c_size_t(reps), C.c_size_t(N), flags)


def launch_shape(field, reps: int, prg: bool):
    """(R, cols_per_trip, max_groups, fused): the launch geometry of scl_vf_launch_shape"""
    r, f = C.c_int(0), C.c_int(0)
    c, g = C.c_size_t(0), C.c_size_t(0)
    lib.scl_vf_launch_shape(field, C.c_size_t(reps), int(bool(prg)), C.byref(r), C.byref(c), C.byref(g), C.byref(f))
    if r.value == 0:
        raise _scl.SclError(_scl.ERR_BAD_ARG, "unknown field tag, or reps outside 1..4")
    return r.value, c.value, g.value, bool(f.value)


def _rows(field, t: torch.Tensor, what: str, shape=None):
    """[rows][N][L] with dense columns -> (pointer, the row stride in elements: the tensor's own; N where one row has none)"""
    L = _scl.limbs(field)
    if t.dtype != torch.int64 or not t.is_cuda:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: expected int64 limbs on the GPU")
    if t.dim() != 3 or t.shape[-1] != L or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{what}: shape {tuple(t.shape)}, expected "
                            f"{tuple(shape) if shape is not None else '[rows][N][%d]' % L}")
    rows, N = t.shape[0], t.shape[1]
    if t.numel() and ((L > 1 and t.stride(2) != 1) or (N > 1 and t.stride(1) != L) or (rows > 1 and t.stride(0) % L)):
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: columns must be dense (a row pitch is allowed)")
    return C.c_void_p(t.data_ptr()), (t.stride(0) // L if rows > 1 else max(N, 1))


def _operands(field, who, x, y, reps, out):
    L = _scl.limbs(field)
    if not 1 <= reps <= REPS_MAX:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{who}: reps must be at least 1 and at most 4")
    px, xs = _rows(field, x, f"{who} x")
    rows, N = x.shape[0], x.shape[1]
    py, ys = (None, xs) if y is None else _rows(field, y, f"{who} y", x.shape)
    if y is not None and y.device != x.device:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{who} y: on {y.device}, expected {x.device}")
    if rows > 1 and ys != xs:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{who}: row strides x {xs}, y {ys} (x and y share op_stride)")
    if out is None:
        out = torch.empty(rows, reps, L, dtype=torch.int64, device=x.device)
    po, os_ = _rows(field, out, f"{who} out", (rows, reps, L))
    if out.device != x.device:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{who} out: on {out.device}, expected {x.device}")
    return px, py, xs, rows, N, out, po, (os_ if rows > 1 else max(reps, 1))


def _scratch(field, who, rows, reps, N, flags, scratch, device):
    """the call's scratch: `scratch` -- an int64 tensor of at least scratch_bytes on the operands' device; pass one when the call
    is captured into a graph -- or allocated here"""
    need = scratch_bytes(field, rows, reps, N, flags)
    if rows and not need:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{who}: rows * reps * N overflows")
    if scratch is None:
        scratch = torch.empty(max(need, 16) // 8, dtype=torch.int64, device=device)
    if scratch.dtype != torch.int64 or scratch.numel() * 8 < need or scratch.device != device or not scratch.is_contiguous():
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"{who}: scratch must be a contiguous int64 tensor of at least {need} bytes on {device}")
    return scratch, scratch.numel() * 8


def combine_prg(field, x, y=None, *, seed: bytes, counter0: int = 0, reps: int = 1, out=None, scratch=None):
    """out[r][j] = sum_s rho_j[s] x[r][s] (y[r][s]) for j < reps, rho_j the j-th consecutive Vector::random(N) of a util::PRG
    on `seed` whose block counter stands at counter0 (scl_vf_combine_prg).  x, y [rows][N][L], possibly pitched views that share
    one row pitch; y None: the plain form; x may be y.  -> [rows][reps][L], the share matrix check_degree takes."""
    px, py, xs, rows, N, out, po, os_ = _operands(field, "combine_prg", x, y, reps, out)
    if not isinstance(seed, (bytes, bytearray)):
        raise _scl.SclError(_scl.ERR_BAD_ARG, "combine_prg: seed must be bytes")
    if not 0 <= counter0 < 1 << 64:
        raise _scl.SclError(_scl.ERR_BAD_ARG, "combine_prg: counter0 is not a 64-bit block counter")
    scratch, need = _scratch(field, "combine_prg", rows, reps, N, PRG, scratch, x.device)
    _chk(lib.scl_vf_combine_prg(field, po, C.c_size_t(os_), px, py, C.c_size_t(xs), C.c_size_t(rows), C.c_size_t(N), C.c_size_t(reps),
                                bytes(seed), C.c_size_t(len(seed)), C.c_uint64(counter0), C.c_void_p(scratch.data_ptr()), C.c_size_t(need),
                                _scl._stream()))
    return out


def combine(field, x, rho, y=None, *, out=None, scratch=None):
    """The same value with rho [reps][N][L] read from memory (scl_vf_combine): coefficients that come from elsewhere."""
    if rho.dim() != 3:
        raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"combine rho: shape {tuple(rho.shape)}, expected [reps][N][{_scl.limbs(field)}]")
    reps = rho.shape[0]
    px, py, xs, rows, N, out, po, os_ = _operands(field, "combine", x, y, reps, out)
    pr, rs = _rows(field, rho, "combine rho", (reps, N, _scl.limbs(field)))
    if rho.device != x.device:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"combine rho: on {rho.device}, expected {x.device}")
    scratch, need = _scratch(field, "combine", rows, reps, N, 0, scratch, x.device)
    _chk(lib.scl_vf_combine(field, po, C.c_size_t(os_), px, py, C.c_size_t(xs), pr, C.c_size_t(rs), C.c_size_t(rows), C.c_size_t(N),
                            C.c_size_t(reps), C.c_void_p(scratch.data_ptr()), C.c_size_t(need), _scl._stream()))
    return out


def check_degree(field, combined, t: int, d: int | None = None):
    """The folded sharing `combined` [n][reps][L] against degree d (default t): scl_hip_shamir_recover_detect over its reps
    columns.  -> the opened values [reps][L]; a share off the polynomial raises the engine's error for "error detected during
    recovery"."""
    out, status, bad = _scl.shamir_recover_detect(field, combined.contiguous(), t, d)
    if bad:
        raise _scl.SclError(_scl.ERR_ERROR_DETECTED, f"check_degree: {bad} of {combined.shape[1]} combinations are off the polynomial")
    return out
