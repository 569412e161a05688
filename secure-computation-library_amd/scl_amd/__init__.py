"""scl_amd -- Python harness over libscl_hip.so, the MI355X-native finite-field /
secret-sharing engine behind SCL's API (include/scl_hip.h is the boundary).

This module is plumbing: it hands torch device buffers (`data_ptr()`) and the
current HIP stream to the C ABI.  All arithmetic runs in the HIP kernels of
csrc/; there is no CPU or torch fallback -- if the extension is missing the
import fails, and if no GPU is present every batch call raises SclError.

Conventions: an element tensor has dtype int64 (the bits of the uint64 limbs)
and trailing dimension `limbs(field)`; a share matrix is SoA `[party][secret][limb]`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch  # imported BEFORE the extension so both share torch's libamdhip64 (same SONAME)

from scl_amd import _abi

lib, _SO = _abi.load("scl_hip")

M61, M127, MONT128, GF2_128, SECP256K1_SCALAR, SECP256K1_FIELD = 0, 1, 2, 3, 4, 5


def Z2K(bits: int) -> int:
    """tag of the ring scl::math::Z2k<bits> (include/scl/math/z2k.h), 1 <= bits <= 128; see SCL_Z2K in scl_hip.h"""
    if not 1 <= bits <= 128:
        raise ValueError("Z2k bit size must be in 1..128")
    return 0x100 + bits


def byte_size(field) -> int:
    """T::byteSize(): the stride of read / Vector::random -- (K-1)/8 + 1 for Z2k<K>, 8 * limbs for the fields"""
    return (field - 0x100 - 1) // 8 + 1 if 0x100 < field <= 0x100 + 128 else 8 * limbs(field)

ADD, SUB, MUL, NEG, INV, DIV = range(6)
OK, ERR_SIZE_MISMATCH, ERR_ZERO_INVERSE, ERR_BAD_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_ERROR_DETECTED, \
    ERR_NOT_ENOUGH_SHARES, ERR_MATMUL_DIMS, ERR_VANDERMONDE_XS, ERR_INVALID_RANGE = range(11)



def _declare_prototypes():
    """argtypes / restype of every entry point, read from the prototypes of include/scl_hip.h (_abi.declare).  Two things are
    the engine's own: without a header the import goes on with a warning, and a header without a version macro is accepted."""
    if _abi.find_header("scl_hip.h") is None:
        import warnings
        # no header to read: result types only (status ints, the two size_t / string getters); arguments unchecked
        warnings.warn("scl_amd: include/scl_hip.h not found beside the package; ctypes argument checking is off")
        for name, ret in (("scl_hip_last_error", C.c_char_p), ("scl_hip_status_message", C.c_char_p),
                          ("scl_hip_field_name", C.c_char_p), ("scl_hip_wire_size", C.c_size_t),
                          ("scl_hip_wire_size_matrix", C.c_size_t), ("scl_hip_frame_size", C.c_size_t)):
            if hasattr(lib, name):
                getattr(lib, name).restype = ret
        return 0
    return _abi.declare(lib, _SO, "scl_hip.h", "scl_hip_", "SCL_HIP_ABI_VERSION", "scl_amd", version_optional=True)


_NPROTO = _declare_prototypes()

_u64p = C.POINTER(C.c_uint64)


class SclError(RuntimeError):
    """status + the message the reference would put in its C++ exception"""

    def __init__(self, status: int, detail: str):
        self.status = status
        self.reference_message = lib.scl_hip_status_message(status).decode()
        super().__init__(f"[{status}] {self.reference_message}" + (f" ({detail})" if detail and detail != self.reference_message else ""))


def _checker(last_error_fn):
    """the status check of one library: raises SclError with the diagnostic of that library's own slot (an extension library
    beside the engine keeps its own: `_chk = _scl._checker(lib.scl_X_last_error)`)"""
    def chk(status: int):
        if status != OK:
            raise SclError(status, last_error_fn().decode())
    return chk


_chk = _checker(lib.scl_hip_last_error)


def limbs(field: int) -> int:
    n = lib.scl_hip_limbs(field)
    if n < 0:
        raise SclError(ERR_BAD_ARG, "unknown field tag")
    return n


def field_name(field: int) -> str:
    return lib.scl_hip_field_name(field).decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t: torch.Tensor):
    if not t.is_cuda:
        raise SclError(ERR_BAD_ARG, "tensor is not on the GPU")
    if not t.is_contiguous():
        raise SclError(ERR_BAD_ARG, "tensor is not contiguous")
    return C.c_void_p(t.data_ptr())


def _want(t: torch.Tensor, shape, what: str, like: torch.Tensor | None = None):
    """out= / operand checks before a raw pointer crosses the boundary: exact shape, int64 limbs, contiguous, on the
    same device as `like` -- a short buffer would otherwise be a silent out-of-bounds HBM access"""
    if t.dtype != torch.int64:
        raise SclError(ERR_BAD_ARG, f"{what}: dtype {t.dtype}, expected int64 limbs")
    if tuple(t.shape) != tuple(shape):
        raise SclError(ERR_SIZE_MISMATCH, f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if like is not None and t.device != like.device:
        raise SclError(ERR_BAD_ARG, f"{what}: on {t.device}, expected {like.device}")
    return t


def _dev_rows(t: torch.Tensor):
    """(device pointer, row stride in elements) of a share matrix [rows][N][L] whose rows are dense but may sit a pitch
    apart -- a window of a larger matrix (a chunk, a shard), the C ABI's `stride >= N`"""
    if not t.is_cuda:
        raise SclError(ERR_BAD_ARG, "tensor is not on the GPU")
    rows, N, L = t.shape
    # (the stride of a dimension of extent 1 means nothing: a [rows][1][L] view of a transposed array carries any value there)
    if N and ((L > 1 and t.stride(2) != 1) or (N > 1 and t.stride(1) != L) or
              (rows > 1 and (t.stride(0) % L or t.stride(0) < N * L))):
        raise SclError(ERR_BAD_ARG, "share matrix rows must be dense (a row pitch is allowed)")
    return C.c_void_p(t.data_ptr()), (t.stride(0) // L if rows > 1 else max(N, 1))


def _rows3(field, t: torch.Tensor, what: str):
    """an operand as [rows][N][L]: a vector [N][L] is one row"""
    L = limbs(field)
    if t.dtype != torch.int64:
        raise SclError(ERR_BAD_ARG, f"{what}: dtype {t.dtype}, expected int64 limbs")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[2] != L:
        raise SclError(ERR_SIZE_MISMATCH, f"{what}: shape {tuple(t.shape)}, expected [rows][N][{L}] or [N][{L}]")
    return t


def _status(N: int, like: torch.Tensor, status, what: str):
    """the status bytes of a call, one per column: the caller's buffer checked, or a new one beside `like`"""
    if status is None:
        return torch.empty(N, dtype=torch.uint8, device=like.device)
    if status.dtype != torch.uint8 or tuple(status.shape) != (N,) or status.device != like.device or not status.is_contiguous():
        raise SclError(ERR_SIZE_MISMATCH, f"{what}: status must be a contiguous uint8 tensor of {N} bytes on {like.device}")
    return status


def _host(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


def _hp(a: np.ndarray):
    return a.ctypes.data_as(_u64p)


def to_device(a, device="cuda") -> torch.Tensor:
    """numpy uint64 (..., limbs) -> int64 device tensor"""
    return torch.from_numpy(_host(a).view(np.int64)).to(device)


def to_host(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint64)


def empty(field: int, *shape, device="cuda") -> torch.Tensor:
    return torch.empty(*shape, limbs(field), dtype=torch.int64, device=device)


def set_tuning(key: str, value: int):
    _chk(lib.scl_hip_set_tuning(key.encode(), C.c_long(value)))


def set_mont128_prime(p: int):
    """Modulus of the MONT128 field for the calling thread AND the process-wide default (scl_hip.h).  A thread that never
    calls this -- a ThreadPoolExecutor worker, say -- LATCHES the default at its first Mont128 call and keeps it; when the
    default changes afterwards that worker's next Mont128 call raises SclError (ERR_BAD_ARG) instead of computing on over
    the old modulus in silence: the worker then calls set_mont128_prime (its own modulus) or mont128_relatch (the current
    default).  A thread that has called this keeps its own modulus whatever the others do."""
    a = np.array([p & (2 ** 64 - 1), p >> 64], dtype=np.uint64)
    _chk(lib.scl_hip_mont128_set_prime(_hp(a)))


def mont128_relatch():
    """the calling thread takes the current process-wide MONT128 modulus (see set_mont128_prime)"""
    _chk(lib.scl_hip_mont128_relatch())


def mont128_prime() -> int:
    a = np.zeros(2, dtype=np.uint64)
    _chk(lib.scl_hip_mont128_get_prime(_hp(a)))
    return int(a[0]) | (int(a[1]) << 64)


# ---- element-wise: scl::math::Vector<FF> ------------------------------------------------------------
def ew(field, op, a, b=None, out=None):
    L = limbs(field)
    if b is not None and b.shape != a.shape:
        raise SclError(ERR_SIZE_MISMATCH, "")  # Vector::ensureCompatible
    if out is None:
        out = torch.empty_like(a)
    n = a.numel() // L
    _chk(lib.scl_hip_ew(field, op, _dev(out), _dev(a), _dev(b) if b is not None else None, C.c_size_t(n), _stream()))
    return out


def ew_status_buffer(device="cuda") -> torch.Tensor:
    """one cleared 32-bit device word for ew_status (scl_hip_ew_status's status_dev)"""
    return torch.zeros(1, dtype=torch.int32, device=device)


def ew_status(field, op, a, b, status, out=None):
    """scl_hip_ew_status: the element-wise call without a host synchronisation -- a zero (even, in a ring) operand of INV / DIV
    ORs 1 into the device word `status` (an int32 tensor of one element, never cleared by the call) instead of raising; read it
    with status.item() when the caller synchronises anyway.  Capturable into a hipGraph."""
    L = limbs(field)
    if b is not None and b.shape != a.shape:
        raise SclError(ERR_SIZE_MISMATCH, "")
    if out is None:
        out = torch.empty_like(a)
    if status is not None and (status.dtype != torch.int32 or status.numel() != 1 or not status.is_cuda):
        raise SclError(ERR_BAD_ARG, "status: one int32 element on the GPU")
    n = a.numel() // L
    _chk(lib.scl_hip_ew_status(field, op, _dev(out), _dev(a), _dev(b) if b is not None else None, C.c_size_t(n),
                               C.c_void_p(status.data_ptr()) if status is not None else None, _stream()))
    return out


def scalar_mul(field, a, scalar, out=None):
    L = limbs(field)
    if out is None:
        out = torch.empty_like(a)
    s = _host(scalar).reshape(L)
    _chk(lib.scl_hip_scalar_mul(field, _dev(out), _dev(a), _hp(s), C.c_size_t(a.numel() // L), _stream()))
    return out


def vsum(field, a) -> np.ndarray:
    L = limbs(field)
    out = np.zeros(L, dtype=np.uint64)
    _chk(lib.scl_hip_sum(field, _hp(out), _dev(a), C.c_size_t(a.numel() // L), _stream()))
    return out


def dot(field, a, b) -> np.ndarray:
    L = limbs(field)
    if b.shape != a.shape:
        raise SclError(ERR_SIZE_MISMATCH, "")
    out = np.zeros(L, dtype=np.uint64)
    _chk(lib.scl_hip_dot(field, _hp(out), _dev(a), _dev(b), C.c_size_t(a.numel() // L), _stream()))
    return out


def equals(field, a, b) -> bool:
    if a.shape != b.shape:
        return False  # Vector::equals (vector.h:559-561)
    eq = C.c_int(0)
    _chk(lib.scl_hip_equals(field, C.byref(eq), _dev(a), _dev(b), C.c_size_t(a.numel() // limbs(field)), _stream()))
    return bool(eq.value)


# ---- randomness: scl::util::PRG ------------------------------------------------------------------------
def prg_blocks(nblocks: int, seed: bytes, counter0: int = 0, device="cuda", out=None) -> torch.Tensor:
    """PRG::next: blocks counter0 .. counter0 + nblocks - 1 of the stream as bytes; `out` (uint8, >= 16 nblocks bytes) is reused"""
    if out is None:
        out = torch.empty(max(nblocks, 1) * 16, dtype=torch.uint8, device=device)
    elif out.dtype != torch.uint8 or out.numel() < nblocks * 16:
        raise SclError(ERR_BAD_ARG, "prg_blocks out: uint8 tensor of at least 16 * nblocks bytes")
    _chk(lib.scl_hip_prg_blocks(_dev(out), C.c_size_t(nblocks), seed, C.c_size_t(len(seed)), C.c_uint64(counter0),
                                _stream()))
    return out[: nblocks * 16]


def from_bytes(field, raw: torch.Tensor) -> torch.Tensor:
    n = raw.numel() // byte_size(field)
    out = empty(field, n, device=raw.device)
    _chk(lib.scl_hip_from_bytes(field, _dev(out), _dev(raw), C.c_size_t(n), _stream()))
    return out


def vector_random(field, n: int, seed: bytes, counter0: int = 0, device="cuda", out=None) -> torch.Tensor:
    if out is None:
        out = empty(field, n, device=device)
    else:
        _want(out, (n, limbs(field)), "vector_random out")
    _chk(lib.scl_hip_vector_random(field, _dev(out), C.c_size_t(n), seed, C.c_size_t(len(seed)),
                                   C.c_uint64(counter0), _stream()))
    return out


# ---- Shamir: scl::ss -----------------------------------------------------------------------------------------
def lagrange_basis(field, m: int, alphas=None, x=None) -> np.ndarray:
    L = limbs(field)
    out = np.zeros((m, L), dtype=np.uint64)
    al = _host(alphas).reshape(m, L) if alphas is not None else None
    xx = _host(x).reshape(L) if x is not None else None
    _chk(lib.scl_hip_lagrange_basis(field, _hp(out), _hp(al) if al is not None else None, C.c_size_t(m),
                                    _hp(xx) if xx is not None else None))
    return out


def shamir_share(field, secrets, coeffs, n: int, alphas=None, out=None):
    """secrets [N][L]; coeffs [t][N][L] (c_1..c_t) -> shares [n][N][L]"""
    L = limbs(field)
    N = secrets.shape[0]
    _want(secrets, (N, L), "shamir_share secrets")
    t = 0 if coeffs is None else coeffs.shape[0]
    if coeffs is not None:
        _want(coeffs, (t, N, L), "shamir_share coeffs", secrets)
    if out is None:
        out = empty(field, n, N, device=secrets.device)
    else:
        _want(out, (n, N, L), "shamir_share out", secrets)
    al = _host(alphas).reshape(n, L) if alphas is not None else None
    _chk(lib.scl_hip_shamir_share(field, _dev(out), C.c_size_t(N), _dev(secrets),
                                  _dev(coeffs) if t else None, C.c_size_t(N), C.c_size_t(N), C.c_size_t(t),
                                  C.c_size_t(n), _hp(al) if al is not None else None, _stream()))
    return out


def blocks_per_secret(field, t: int) -> int:
    """AES blocks one shamirSecretShare call consumes: ceil((t+1)*byteSize/16)"""
    return ((t + 1) * 8 * limbs(field) + 15) // 16


def shamir_share_prg(field, secrets, t: int, n: int, seed: bytes, first_secret: int = 0, out=None, counter0=None):
    """first_secret: index of secrets[0] in a longer single-PRG run (counter0 = first_secret * B);
    counter0 overrides it with an explicit PRG block counter"""
    N = secrets.shape[0]
    _want(secrets, (N, limbs(field)), "shamir_share_prg secrets")
    if counter0 is None:
        counter0 = first_secret * blocks_per_secret(field, t)
    if out is None:
        out = empty(field, n, N, device=secrets.device)
    else:
        _want(out, (n, N, limbs(field)), "shamir_share_prg out", secrets)
    _chk(lib.scl_hip_shamir_share_prg(field, _dev(out), C.c_size_t(N), _dev(secrets), C.c_size_t(N), C.c_size_t(t),
                                      C.c_size_t(n), seed, C.c_size_t(len(seed)), C.c_uint64(counter0),
                                      _stream()))
    return out


def shamir_recover(field, shares, lam=None, out=None):
    """shares [m][N][L] -> out [N][L]; lam defaults to the basis for nodes 1..m at x=0"""
    L = limbs(field)
    m, N = shares.shape[0], shares.shape[1]
    _want(shares, (m, N, L), "shamir_recover shares")
    if lam is None:
        lam = lagrange_basis(field, m)
    lam = _host(lam).reshape(m, L)
    if out is None:
        out = empty(field, N, device=shares.device)
    else:
        _want(out, (N, L), "shamir_recover out", shares)
    sp, stride = _dev_rows(shares)
    _chk(lib.scl_hip_shamir_recover(field, _dev(out), sp, C.c_size_t(stride), _hp(lam), C.c_size_t(m),
                                    C.c_size_t(N), _stream()))
    return out


def shamir_recover_detect(field, shares, t: int, d: int | None = None, alphas=None, x=None):
    """-> (out [N][L], status uint8 [N], num_bad); raises nothing for detected errors (see status)"""
    L = limbs(field)
    m, N = shares.shape[0], shares.shape[1]
    d = t if d is None else d
    out = empty(field, N, device=shares.device)
    status = torch.empty(max(N, 1), dtype=torch.uint8, device=shares.device)
    al = _host(alphas).reshape(m, L) if alphas is not None else None
    xx = _host(x).reshape(L) if x is not None else None
    bad = C.c_size_t(0)
    st = lib.scl_hip_shamir_recover_detect(field, _dev(out), _dev(status), _dev(shares), C.c_size_t(N), C.c_size_t(m),
                                           C.c_size_t(N), C.c_size_t(t), C.c_size_t(d),
                                           _hp(al) if al is not None else None, _hp(xx) if xx is not None else None,
                                           C.byref(bad), _stream())
    if st not in (OK, ERR_ERROR_DETECTED):
        _chk(st)
    return out, status[:N], bad.value


def shamir_share_prg_packed(field, secrets, t: int, n: int, seed: bytes, counter0: int = 0):
    """shamirSecretShare over Array<FF, W>: secrets [W][N][L] -> shares [W][n][N][L] (component-major SoA)"""
    W, N = secrets.shape[0], secrets.shape[1]
    out = empty(field, W, n, N, device=secrets.device)
    _chk(lib.scl_hip_shamir_share_prg_packed(field, _dev(out), C.c_size_t(N), _dev(secrets), C.c_size_t(N), C.c_size_t(N),
                                             C.c_size_t(t), C.c_size_t(n), C.c_size_t(W), seed, C.c_size_t(len(seed)),
                                             C.c_uint64(counter0), _stream()))
    return out


def shamir_recover_correct(field, shares, alphas=None):
    """Batched shamirRecoverC (Berlekamp-Welch).  shares [m][N][L] -> dict(f [3t+1][N][L], err [t+1][N][L],
    status uint8 [N], nerr int32 [N], queued, failed); the secrets are f[0]."""
    L = limbs(field)
    m, N = shares.shape[0], shares.shape[1]
    t = (m - 1) // 3
    n = 3 * t + 1
    f = empty(field, n, N, device=shares.device)
    e = empty(field, t + 1, N, device=shares.device)
    status = torch.empty(max(N, 1), dtype=torch.uint8, device=shares.device)
    nerr = torch.empty(max(N, 1), dtype=torch.int32, device=shares.device)
    al = _host(alphas).reshape(-1, L) if alphas is not None else None
    queued, failed = C.c_size_t(0), C.c_size_t(0)
    _chk(lib.scl_hip_shamir_recover_correct(field, _dev(f), C.c_size_t(N), _dev(e), C.c_size_t(N), _dev(status), _dev(nerr),
                                            _dev(shares), C.c_size_t(N), C.c_size_t(m), C.c_size_t(N),
                                            _hp(al) if al is not None else None, C.byref(queued), C.byref(failed),
                                            _stream()))
    return {"f": f, "err": e, "status": status[:N], "nerr": nerr[:N], "queued": queued.value, "failed": failed.value}


# ---- additive ----------------------------------------------------------------------------------------------------
def additive_share(field, secrets, rnd, n: int, out=None):
    N, L = secrets.shape[0], limbs(field)
    _want(secrets, (N, L), "additive_share secrets")
    if rnd is not None:
        _want(rnd, (n - 1, N, L), "additive_share rnd", secrets)
    if out is None:
        out = empty(field, n, N, device=secrets.device)
    else:
        _want(out, (n, N, L), "additive_share out", secrets)
    _chk(lib.scl_hip_additive_share(field, _dev(out), C.c_size_t(N), _dev(secrets),
                                    _dev(rnd) if rnd is not None else None, C.c_size_t(N), C.c_size_t(N),
                                    C.c_size_t(n), _stream()))
    return out


def additive_share_prg(field, secrets, n: int, seed: bytes, first_secret: int = 0, out=None, counter0=None):
    N = secrets.shape[0]
    _want(secrets, (N, limbs(field)), "additive_share_prg secrets")
    if counter0 is None:
        counter0 = first_secret * (n - 1) * ((8 * limbs(field) + 15) // 16)  # FF::random burns whole blocks
    if out is None:
        out = empty(field, n, N, device=secrets.device)
    else:
        _want(out, (n, N, limbs(field)), "additive_share_prg out", secrets)
    _chk(lib.scl_hip_additive_share_prg(field, _dev(out), C.c_size_t(N), _dev(secrets), C.c_size_t(N), C.c_size_t(n),
                                        seed, C.c_size_t(len(seed)), C.c_uint64(counter0), _stream()))
    return out


def additive_recover(field, shares, out=None):
    n, N = shares.shape[0], shares.shape[1]
    _want(shares, (n, N, limbs(field)), "additive_recover shares")
    if out is None:
        out = empty(field, N, device=shares.device)
    else:
        _want(out, (N, limbs(field)), "additive_recover out", shares)
    _chk(lib.scl_hip_additive_recover(field, _dev(out), _dev(shares), C.c_size_t(N), C.c_size_t(n), C.c_size_t(N),
                                      _stream()))
    return out


# ---- matrices ---------------------------------------------------------------------------------------------------------
def vandermonde(field, n: int, m: int, xs=None, device="cuda"):
    L = limbs(field)
    out = empty(field, n, m, device=device)
    x = _host(xs).reshape(n, L) if xs is not None else None
    _chk(lib.scl_hip_vandermonde(field, _dev(out), C.c_size_t(n), C.c_size_t(m), _hp(x) if x is not None else None,
                                 _stream()))
    return out


def matmul(field, A, B, out=None):
    M, K = A.shape[0], A.shape[1]
    if B.shape[0] != K:
        raise SclError(ERR_MATMUL_DIMS, "")
    N = B.shape[1]
    if out is None:
        out = empty(field, M, N, device=A.device)
    _chk(lib.scl_hip_matmul(field, _dev(out), C.c_size_t(N), _dev(A), C.c_size_t(K), _dev(B), C.c_size_t(N),
                            C.c_size_t(M), C.c_size_t(K), C.c_size_t(N), _stream()))
    return out


# ---- layout -----------------------------------------------------------------------------------------------------------
def aos_to_soa(field, aos):
    N, n = aos.shape[0], aos.shape[1]
    out = empty(field, n, N, device=aos.device)
    _chk(lib.scl_hip_aos_to_soa(field, _dev(out), C.c_size_t(N), _dev(aos), C.c_size_t(N), C.c_size_t(n), _stream()))
    return out


def soa_to_aos(field, soa):
    n, N = soa.shape[0], soa.shape[1]
    out = empty(field, N, n, device=soa.device)
    _chk(lib.scl_hip_soa_to_aos(field, _dev(out), _dev(soa), C.c_size_t(N), C.c_size_t(N), C.c_size_t(n), _stream()))
    return out


# ---- wire image: seri::Serializer<Vector<FF>> -------------------------------------------------------------------------
def wire_pack(field, a: torch.Tensor) -> torch.Tensor:
    """elements [n][L] -> uint8 device buffer: u32 count || n * byteSize bytes (FF::write images)"""
    L = limbs(field)
    n = a.numel() // L
    lib.scl_hip_wire_size.restype = C.c_size_t
    out = torch.empty(lib.scl_hip_wire_size(field, C.c_size_t(n)), dtype=torch.uint8, device=a.device)
    _chk(lib.scl_hip_wire_pack(field, _dev(out), _dev(a) if n else None, C.c_size_t(n), _stream()))
    return out


def wire_unpack(field, raw: torch.Tensor, capacity: int | None = None) -> torch.Tensor:
    L = limbs(field)
    cap = (raw.numel() - 4) // (8 * L) if capacity is None else capacity
    out = empty(field, max(cap, 1), device=raw.device)
    n = C.c_size_t(0)
    _chk(lib.scl_hip_wire_unpack(field, _dev(out), C.c_size_t(cap), _dev(raw), C.c_size_t(raw.numel()), C.byref(n),
                                 _stream()))
    return out[: n.value]


def wire_pack_matrix(field, m: torch.Tensor) -> torch.Tensor:
    """row-major matrix [rows][cols][L] -> uint8 device buffer: u32 rows || u32 cols || vector image (matrix.h:910-963)"""
    rows, cols = (m.shape[0], m.shape[1]) if m.numel() else (0, 0)
    lib.scl_hip_wire_size_matrix.restype = C.c_size_t
    out = torch.empty(lib.scl_hip_wire_size_matrix(field, C.c_size_t(rows), C.c_size_t(cols)), dtype=torch.uint8,
                      device=m.device)
    _chk(lib.scl_hip_wire_pack_matrix(field, _dev(out), _dev(m) if m.numel() else None, C.c_size_t(cols), C.c_size_t(rows),
                                      C.c_size_t(cols), _stream()))
    return out


def wire_unpack_matrix(field, raw: torch.Tensor, capacity=None) -> torch.Tensor:
    """inverse of wire_pack_matrix; capacity = (rows, cols) of the destination (default: sized from the image)"""
    L = limbs(field)
    if capacity is None:
        hdr = raw[:12].cpu().numpy().view("<u4")
        capacity = (int(hdr[0]), int(hdr[1]))
    cr, cc = capacity
    out = empty(field, max(cr, 1), max(cc, 1), device=raw.device)
    r, c = C.c_size_t(0), C.c_size_t(0)
    _chk(lib.scl_hip_wire_unpack_matrix(field, _dev(out), C.c_size_t(max(cc, 1)), C.c_size_t(cr), _dev(raw),
                                        C.c_size_t(raw.numel()), C.byref(r), C.byref(c), _stream()))
    return out[: r.value, : c.value]


def frame_pack(field, a: torch.Tensor, as_matrix: bool = False) -> torch.Tensor:
    """TcpChannel frame (u32 packet size || packet) of a Packet holding this Vector [n][L] / Matrix [rows][cols][L]"""
    L = limbs(field)
    lib.scl_hip_wire_size.restype = lib.scl_hip_wire_size_matrix.restype = lib.scl_hip_frame_size.restype = C.c_size_t
    if as_matrix:
        rows, cols = (a.shape[0], a.shape[1]) if a.numel() else (0, 0)
        image = lib.scl_hip_wire_size_matrix(field, C.c_size_t(rows), C.c_size_t(cols))
        out = torch.empty(lib.scl_hip_frame_size(C.c_size_t(image)), dtype=torch.uint8, device=a.device)
        _chk(lib.scl_hip_frame_pack_matrix(field, _dev(out), _dev(a) if a.numel() else None, C.c_size_t(cols),
                                           C.c_size_t(rows), C.c_size_t(cols), _stream()))
        return out
    n = a.numel() // L
    image = lib.scl_hip_wire_size(field, C.c_size_t(n))
    out = torch.empty(lib.scl_hip_frame_size(C.c_size_t(image)), dtype=torch.uint8, device=a.device)
    _chk(lib.scl_hip_frame_pack(field, _dev(out), _dev(a) if n else None, C.c_size_t(n), _stream()))
    return out


def frame_unpack(field, raw: torch.Tensor) -> torch.Tensor:
    L = limbs(field)
    cap = max(0, (raw.numel() - 8) // (8 * L))
    out = empty(field, max(cap, 1), device=raw.device)
    n = C.c_size_t(0)
    _chk(lib.scl_hip_frame_unpack(field, _dev(out), C.c_size_t(cap), _dev(raw), C.c_size_t(raw.numel()), C.byref(n),
                                  _stream()))
    return out[: n.value]


# ---- commitments: scl::util::Sha256, scl::util::MerkleTree<Sha256, FF> -------------------------------------------------------
def _digests(*shape, device="cuda") -> torch.Tensor:
    return torch.empty(*shape, 32, dtype=torch.uint8, device=device)


def _index(idx, device):
    """None, or a device tensor of 64-bit indices"""
    if idx is None:
        return None
    t = torch.as_tensor(idx, dtype=torch.int64, device=device)
    return t if t.is_contiguous() else t.contiguous()


def sha256(msgs: torch.Tensor, msg_len: int | None = None) -> torch.Tensor:
    """uint8 [count][stride] device buffer -> [count][32] digests of the first msg_len (default: stride) bytes of each row"""
    if msgs.dtype != torch.uint8 or msgs.dim() != 2:
        raise SclError(ERR_BAD_ARG, "sha256: a uint8 [count][stride] tensor is expected")
    count, stride = msgs.shape
    msg_len = stride if msg_len is None else msg_len
    if msg_len > stride:
        raise SclError(ERR_SIZE_MISMATCH, "sha256: msg_len exceeds the row length")
    out = _digests(count, device=msgs.device)
    _chk(lib.scl_hip_sha256(_dev(out), _dev(msgs) if msgs.numel() else None, C.c_size_t(msg_len), C.c_size_t(stride),
                            C.c_size_t(count), _stream()))
    return out


def merkle_depth(L: int) -> int:
    return lib.scl_hip_merkle_depth(C.c_size_t(L))


def merkle_level_size(L: int, level: int) -> int:
    return lib.scl_hip_merkle_level_size(C.c_size_t(L), C.c_size_t(level))


def merkle_tree_bytes(L: int, T: int = 1) -> int:
    return lib.scl_hip_merkle_tree_bytes(C.c_size_t(L), C.c_size_t(T))


def merkle_leaves(field, a: torch.Tensor, out=None) -> torch.Tensor:
    """elements [L][limbs] (one tree) or a share matrix [n][N][limbs] (N trees of n leaves; rows may sit a pitch apart)
    -> leaf digests [L][32] / [n][N][32], the leaf level of merkle_build's layout"""
    if a.dim() == 2:
        a = a.unsqueeze(0)
        shape = (a.shape[1],)
    else:
        shape = (a.shape[0], a.shape[1])
    ptr, stride = _dev_rows(a)
    rows, cols = a.shape[0], a.shape[1]
    if out is None:
        out = _digests(*shape, device=a.device)
    elif out.dtype != torch.uint8 or out.numel() != rows * cols * 32:
        raise SclError(ERR_SIZE_MISMATCH, "merkle_leaves: out must hold rows * cols digests")
    _chk(lib.scl_hip_merkle_leaves(field, _dev(out), ptr, C.c_size_t(stride), C.c_size_t(rows), C.c_size_t(cols), _stream()))
    return out


def _leaf_shape(leaf_digests: torch.Tensor):
    """(L, T) of leaf digests [L][32] or [L][T][32]"""
    if leaf_digests.dtype != torch.uint8 or leaf_digests.shape[-1] != 32 or leaf_digests.dim() not in (2, 3):
        raise SclError(ERR_BAD_ARG, "leaf digests: uint8 [L][32] or [L][T][32] expected")
    return leaf_digests.shape[0], (leaf_digests.shape[1] if leaf_digests.dim() == 3 else 1)


def merkle_build(leaf_digests: torch.Tensor) -> torch.Tensor:
    """all levels of T trees of L leaves as one uint8 buffer (scl_hip.h: leaf-major, tree-minor, roots last)"""
    L, T = _leaf_shape(leaf_digests)
    tree = torch.empty(merkle_tree_bytes(L, T), dtype=torch.uint8, device=leaf_digests.device)
    _chk(lib.scl_hip_merkle_build(_dev(tree), _dev(leaf_digests), C.c_size_t(L), C.c_size_t(T), _stream()))
    return tree


def merkle_root(leaf_digests: torch.Tensor) -> torch.Tensor:
    """[T][32] roots, no levels kept"""
    L, T = _leaf_shape(leaf_digests)
    roots = _digests(T, device=leaf_digests.device)
    _chk(lib.scl_hip_merkle_root(_dev(roots), _dev(leaf_digests), C.c_size_t(L), C.c_size_t(T), _stream()))
    return roots


def merkle_paths(tree: torch.Tensor, L: int, T: int = 1, leaf_index=None, tree_index=None, first_leaf: int = 0,
                 k: int | None = None) -> torch.Tensor:
    """[depth][k][32] siblings.  Index arrays (device int64) or the regular pattern tree = q mod T, leaf = first_leaf + q / T"""
    li, ti = _index(leaf_index, tree.device), _index(tree_index, tree.device)
    if k is None:
        k = li.numel() if li is not None else ti.numel() if ti is not None else T
    for t in (li, ti):
        if t is not None and t.numel() != k:
            raise SclError(ERR_SIZE_MISMATCH, "merkle_paths: an index array does not hold k entries")
    if tree.numel() != merkle_tree_bytes(L, T):
        raise SclError(ERR_SIZE_MISMATCH, "merkle_paths: the tree buffer does not have the size of (L, T)")
    path = _digests(merkle_depth(L), k, device=tree.device)
    _chk(lib.scl_hip_merkle_paths(_dev(path), _dev(tree), C.c_size_t(L), C.c_size_t(T), _dev(li) if li is not None else None,
                                  _dev(ti) if ti is not None else None, C.c_size_t(first_leaf), C.c_size_t(k), _stream()))
    return path


def merkle_verify(leaf_digests: torch.Tensor, path: torch.Tensor, roots: torch.Tensor, leaf_index=None, leaf: int = 0,
                  root_index=None) -> torch.Tensor:
    """uint8 [k]: 1 where leaf digest q with path[:, q] and its leaf index hashes up to its root"""
    depth, k = path.shape[0], path.shape[1]
    li, ri = _index(leaf_index, path.device), _index(root_index, path.device)
    if leaf_digests.numel() != k * 32 or any(t is not None and t.numel() != k for t in (li, ri)):
        raise SclError(ERR_SIZE_MISMATCH, "merkle_verify: k leaf digests / indices expected")
    ok = torch.empty(k, dtype=torch.uint8, device=path.device)
    _chk(lib.scl_hip_merkle_verify(_dev(ok), _dev(leaf_digests), _dev(li) if li is not None else None, C.c_size_t(leaf),
                                   _dev(path), C.c_size_t(depth), _dev(roots), _dev(ri) if ri is not None else None,
                                   C.c_size_t(roots.numel() // 32), C.c_size_t(k), _stream()))
    return ok


# ---- verifiable sharing: scl::math::EC<Secp256k1> over vectors, scl::ss::feldman* ---------------------------------------
EC_DBL = 6          # SCL_EC_OP_DBL, for ec_ew only
EC_LIMBS = 12       # X, Y, Z: four Montgomery limbs each
EC_WIRE_BYTES = 65  # 0x04 | x | y


def _points(t: torch.Tensor, what: str):
    if t.dtype != torch.int64 or t.dim() < 2 or t.shape[-1] != EC_LIMBS:
        raise SclError(ERR_BAD_ARG, f"{what}: int64 [..][12] points expected")
    return t


def ec_empty(*shape, device="cuda") -> torch.Tensor:
    return torch.empty(*shape, EC_LIMBS, dtype=torch.int64, device=device)


def ec_generator() -> np.ndarray:
    g = np.zeros(EC_LIMBS, dtype=np.uint64)
    _chk(lib.scl_hip_ec_generator(_hp(g)))
    return g


def ec_ew(op, a, b=None, out=None):
    """points [n][12]: ADD, SUB (a, b), NEG, EC_DBL (a); out may be a or b"""
    _points(a, "ec_ew a")
    if b is not None and _points(b, "ec_ew b").shape != a.shape:
        raise SclError(ERR_SIZE_MISMATCH, "")
    if out is None:
        out = torch.empty_like(a)
    else:
        _want(out, a.shape, "ec_ew out", a)
    _chk(lib.scl_hip_ec_ew(op, _dev(out), _dev(a), _dev(b) if b is not None else None, C.c_size_t(a.numel() // EC_LIMBS),
                           _stream()))
    return out


def ec_equal(a, b) -> torch.Tensor:
    """uint8 [n]: 1 where a[i] == b[i] as points"""
    if _points(a, "ec_equal a").shape != _points(b, "ec_equal b").shape:
        raise SclError(ERR_SIZE_MISMATCH, "")
    n = a.numel() // EC_LIMBS
    eq = torch.empty(n, dtype=torch.uint8, device=a.device)
    _chk(lib.scl_hip_ec_equal(_dev(eq), _dev(a), _dev(b), C.c_size_t(n), _stream()))
    return eq


def ec_base_table(base=None, device="cuda") -> torch.Tensor:
    """the window table of a base point (host limbs [12]; default: the generator), owned by the caller"""
    base = ec_generator() if base is None else _host(base).reshape(EC_LIMBS)
    table = torch.empty(lib.scl_hip_ec_base_table_bytes(), dtype=torch.uint8, device=device)
    _chk(lib.scl_hip_ec_base_table(_dev(table), _hp(base), _stream()))
    return table


def ec_mul_base(table, scalars, out=None):
    """SECP256K1_SCALAR elements [n][4] -> points [n][12], scalars[i] * B for the table's base B"""
    n = scalars.shape[0]
    _want(scalars, (n, 4), "ec_mul_base scalars")
    if out is None:
        out = ec_empty(n, device=scalars.device)
    else:
        _want(out, (n, EC_LIMBS), "ec_mul_base out", scalars)
    _chk(lib.scl_hip_ec_mul_base(_dev(out), _dev(table), _dev(scalars), C.c_size_t(n), _stream()))
    return out


def ec_lincomb(points, scalars, out=None):
    """points [m][N][12] (rows may sit a pitch apart), scalars [m][4] on the device -> [N][12]: sum_k scalars[k] * points[k]"""
    _points(points, "ec_lincomb points")
    ptr, stride = _dev_rows(points)
    m, N = points.shape[0], points.shape[1]
    _want(scalars, (m, 4), "ec_lincomb scalars", points)
    if out is None:
        out = ec_empty(N, device=points.device)
    else:
        _want(out, (N, EC_LIMBS), "ec_lincomb out", points)
    _chk(lib.scl_hip_ec_lincomb(_dev(out), ptr, C.c_size_t(stride), C.c_size_t(m), _dev(scalars), C.c_size_t(N), _stream()))
    return out


def ec_wire_pack(points) -> torch.Tensor:
    """points [n][12] -> uint8 [n][65] Serializer<EC> images"""
    n = _points(points, "ec_wire_pack").numel() // EC_LIMBS
    out = torch.empty(n, EC_WIRE_BYTES, dtype=torch.uint8, device=points.device)
    _chk(lib.scl_hip_ec_wire_pack(_dev(out), _dev(points), C.c_size_t(n), _stream()))
    return out


def ec_wire_unpack(raw):
    """uint8 [n][65] -> (points [n][12], status uint8 [n]: non-zero for an image that is not uncompressed)"""
    if raw.dtype != torch.uint8 or raw.dim() != 2 or raw.shape[1] != EC_WIRE_BYTES:
        raise SclError(ERR_BAD_ARG, "ec_wire_unpack: a uint8 [n][65] tensor is expected")
    n = raw.shape[0]
    out = ec_empty(n, device=raw.device)
    status = torch.empty(n, dtype=torch.uint8, device=raw.device)
    _chk(lib.scl_hip_ec_wire_unpack(_dev(out), _dev(status), _dev(raw), C.c_size_t(n), _stream()))
    return out, status


def feldman_commit(gtable, secrets, shares, t: int, out=None):
    """secrets [N][4], shares [n][N][4] (the SoA share matrix, n >= t) -> commitments [t + 1][N][12]"""
    N = secrets.shape[0]
    _want(secrets, (N, 4), "feldman_commit secrets")
    if shares.dim() != 3 or shares.shape[0] < t or shares.shape[1] != N or shares.shape[2] != 4 or shares.dtype != torch.int64:
        raise SclError(ERR_SIZE_MISMATCH, "feldman_commit: shares [n >= t][N][4] expected")
    ptr, stride = _dev_rows(shares)
    if out is None:
        out = ec_empty(t + 1, N, device=secrets.device)
    else:
        _want(out, (t + 1, N, EC_LIMBS), "feldman_commit out", secrets)
    _chk(lib.scl_hip_feldman_commit(_dev(out), C.c_size_t(N), _dev(gtable), _dev(secrets), ptr, C.c_size_t(stride),
                                    C.c_size_t(t), C.c_size_t(N), _stream()))
    return out


def feldman_lambda(t: int, index: int, device="cuda") -> torch.Tensor:
    """the Lagrange basis over the nodes 0..t at `index` (feldman.h:139-140), on the device"""
    nodes = np.stack([_mont_small(k) for k in range(t + 1)])
    return to_device(lagrange_basis(SECP256K1_SCALAR, t + 1, nodes, _mont_small(index)), device)


def _mont_small(v: int) -> np.ndarray:
    """v as a SECP256K1_SCALAR element (Montgomery limbs)"""
    q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
    m = (v % q) * (1 << 256) % q
    return np.array([(m >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)


def feldman_verify(gtable, share, commitments, lam, scratch=None, out=None):
    """share [N][4], commitments [t + 1][N][12], lam = feldman_lambda(t, index) -> uint8 [N] verdicts"""
    N = share.shape[0]
    _want(share, (N, 4), "feldman_verify share")
    _points(commitments, "feldman_verify commitments")
    ptr, stride = _dev_rows(commitments)
    t = commitments.shape[0] - 1
    _want(lam, (t + 1, 4), "feldman_verify lambda", share)
    if commitments.shape[1] != N:
        raise SclError(ERR_SIZE_MISMATCH, "feldman_verify: commitments [t + 1][N][12] expected")
    if scratch is None:
        scratch = ec_empty(2 * N, device=share.device)
    else:
        _want(scratch, (2 * N, EC_LIMBS), "feldman_verify scratch", share)
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=share.device)
    _chk(lib.scl_hip_feldman_verify(_dev(out), _dev(share), ptr, C.c_size_t(stride), C.c_size_t(t), _dev(lam), _dev(gtable),
                                    _dev(scratch), C.c_size_t(N), _stream()))
    return out


# ---- scl::ss::pedersen*: a second base H (a window table of its own, ec_base_table(h)) beside the generator ----------------
def ec_mul_two_base(gtable, htable, a, b, out=None):
    """SECP256K1_SCALAR elements a, b [n][4] -> points [n][12], a[i] * G + b[i] * H for the tables' bases"""
    n = a.shape[0]
    _want(a, (n, 4), "ec_mul_two_base a")
    _want(b, (n, 4), "ec_mul_two_base b", a)
    if out is None:
        out = ec_empty(n, device=a.device)
    else:
        _want(out, (n, EC_LIMBS), "ec_mul_two_base out", a)
    _chk(lib.scl_hip_ec_mul_two_base(_dev(out), _dev(gtable), _dev(htable), _dev(a), _dev(b), C.c_size_t(n), _stream()))
    return out


def ec_matmul(matrix, points, out=None):
    """matrix [rows][p][4] scalars on the device, points [p][cols][12] (rows may sit a pitch apart) -> [rows][cols][12]:
    out[i][c] = sum_k matrix[i][k] * points[k][c], the commitment side of ss::apply"""
    _points(points, "ec_matmul points")
    if points.dim() != 3:
        raise SclError(ERR_BAD_ARG, "ec_matmul: points [p][cols][12] expected")
    ptr, stride = _dev_rows(points)
    p, cols = points.shape[0], points.shape[1]
    if matrix.dim() != 3 or matrix.shape[1] != p:
        raise SclError(ERR_SIZE_MISMATCH, "ec_matmul: matrix [rows][p][4] expected")
    rows = matrix.shape[0]
    _want(matrix, (rows, p, 4), "ec_matmul matrix", points)
    if out is None:
        out = ec_empty(rows, cols, device=points.device)
    else:
        _want(out, (rows, cols, EC_LIMBS), "ec_matmul out", points)
    _chk(lib.scl_hip_ec_matmul(_dev(out), C.c_size_t(cols), _dev(matrix), C.c_size_t(rows), C.c_size_t(p), ptr, C.c_size_t(stride),
                               C.c_size_t(cols), _stream()))
    return out


def pedersen_commit(gtable, htable, secrets, shares, t: int, out=None):
    """secrets [2][N][4] ({secret, blinding}), shares [2][n][N][4] (shamir_share_prg_packed's layout, n >= t) -> commitments
    [t + 1][N][12]"""
    if secrets.dim() != 3 or secrets.shape[0] != 2:
        raise SclError(ERR_SIZE_MISMATCH, "pedersen_commit: secrets [2][N][4] expected")
    N = secrets.shape[1]
    _want(secrets, (2, N, 4), "pedersen_commit secrets")
    if shares.dim() != 4 or shares.shape[0] != 2 or shares.shape[1] < t or shares.shape[2] != N:
        raise SclError(ERR_SIZE_MISMATCH, "pedersen_commit: shares [2][n >= t][N][4] expected")
    n = shares.shape[1]
    _want(shares, (2, n, N, 4), "pedersen_commit shares", secrets)
    if out is None:
        out = ec_empty(t + 1, N, device=secrets.device)
    else:
        _want(out, (t + 1, N, EC_LIMBS), "pedersen_commit out", secrets)
    _chk(lib.scl_hip_pedersen_commit(_dev(out), C.c_size_t(N), _dev(gtable), _dev(htable), _dev(secrets), C.c_size_t(N),
                                     _dev(shares), C.c_size_t(N), C.c_size_t(t), C.c_size_t(n), C.c_size_t(N), _stream()))
    return out


def pedersen_verify(gtable, htable, share, rand, commitments, lam, scratch=None, out=None):
    """share, rand [N][4], commitments [t + 1][N][12], lam = feldman_lambda(t, index) -> uint8 [N] verdicts"""
    N = share.shape[0]
    _want(share, (N, 4), "pedersen_verify share")
    _want(rand, (N, 4), "pedersen_verify rand", share)
    _points(commitments, "pedersen_verify commitments")
    ptr, stride = _dev_rows(commitments)
    t = commitments.shape[0] - 1
    _want(lam, (t + 1, 4), "pedersen_verify lambda", share)
    if commitments.shape[1] != N:
        raise SclError(ERR_SIZE_MISMATCH, "pedersen_verify: commitments [t + 1][N][12] expected")
    if scratch is None:
        scratch = ec_empty(2 * N, device=share.device)
    else:
        _want(scratch, (2 * N, EC_LIMBS), "pedersen_verify scratch", share)
    if out is None:
        out = torch.empty(N, dtype=torch.uint8, device=share.device)
    _chk(lib.scl_hip_pedersen_verify(_dev(out), _dev(share), _dev(rand), ptr, C.c_size_t(stride), C.c_size_t(t), _dev(lam),
                                     _dev(gtable), _dev(htable), _dev(scratch), C.c_size_t(N), _stream()))
    return out


# ---- signatures: scl::util::ECDSA over batches ----------------------------------------------------------------------------
def ec_mul_scratch(n: int, device="cuda") -> torch.Tensor:
    """the window-table scratch of ec_mul / ecdsa_verify for n items (contents meaningless between calls)"""
    return torch.empty(lib.scl_hip_ec_mul_scratch_bytes(C.c_size_t(n)), dtype=torch.uint8, device=device)


def _mul_scratch(scratch, n: int, like: torch.Tensor, what: str):
    if scratch is None:
        return ec_mul_scratch(n, device=like.device)
    if scratch.dtype != torch.uint8 or scratch.numel() < lib.scl_hip_ec_mul_scratch_bytes(C.c_size_t(n)) or scratch.device != like.device:
        raise SclError(ERR_SIZE_MISMATCH, f"{what}: scratch must be uint8, of ec_mul_scratch(n)'s size")
    return scratch


def ec_mul(points, scalars, scratch=None, out=None):
    """points [n][12], SECP256K1_SCALAR elements [n][4] -> [n][12]: scalars[i] * points[i]; out may be points"""
    n = scalars.shape[0]
    _want(scalars, (n, 4), "ec_mul scalars")
    _want(_points(points, "ec_mul points"), (n, EC_LIMBS), "ec_mul points", scalars)
    if out is None:
        out = ec_empty(n, device=scalars.device)
    else:
        _want(out, (n, EC_LIMBS), "ec_mul out", scalars)
    scratch = _mul_scratch(scratch, n, scalars, "ec_mul")
    _chk(lib.scl_hip_ec_mul(_dev(out), _dev(points), _dev(scalars), _dev(scratch), C.c_size_t(n), _stream()))
    return out


def ecdsa_conversion(points, out=None):
    """points [n][12] -> SECP256K1_SCALAR elements [n][4]: the affine x mod the group order (ECDSA::conversionFunc)"""
    n = _points(points, "ecdsa_conversion").numel() // EC_LIMBS
    if out is None:
        out = torch.empty(n, 4, dtype=torch.int64, device=points.device)
    else:
        _want(out, (n, 4), "ecdsa_conversion out", points)
    _chk(lib.scl_hip_ecdsa_conversion(_dev(out), _dev(points), C.c_size_t(n), _stream()))
    return out


def _digest_rows(digests, n: int, what: str):
    if digests.dtype != torch.uint8 or tuple(digests.shape) != (n, 32):
        raise SclError(ERR_SIZE_MISMATCH, f"{what}: digests must be uint8 [n][32]")
    return digests


def ecdsa_sign(gtable, sk, nonces, digests, status=None, out=None):
    """sk [1][4] (one key) or [n][4], nonces [n][4], digests uint8 [n][32] -> signatures [n][8] (r then s).  A zero nonce writes
    (0, 0) and sets `status` (ew_status_buffer(), never cleared here) to 1."""
    n = nonces.shape[0]
    _want(nonces, (n, 4), "ecdsa_sign nonces")
    if sk.shape[0] not in (1, n):
        raise SclError(ERR_SIZE_MISMATCH, "ecdsa_sign: one secret key, or one per signature")
    _want(sk, (sk.shape[0], 4), "ecdsa_sign sk", nonces)
    _digest_rows(digests, n, "ecdsa_sign")
    if status is not None and (status.dtype != torch.int32 or status.numel() != 1 or not status.is_cuda):
        raise SclError(ERR_BAD_ARG, "status: one int32 element on the GPU")
    if out is None:
        out = torch.empty(n, 8, dtype=torch.int64, device=nonces.device)
    else:
        _want(out, (n, 8), "ecdsa_sign out", nonces)
    _chk(lib.scl_hip_ecdsa_sign(_dev(out), _dev(gtable), _dev(sk), C.c_size_t(0 if sk.shape[0] == 1 else 1), _dev(nonces),
                                _dev(digests), _dev(status) if status is not None else None, C.c_size_t(n), _stream()))
    return out


def _verdicts(out, n: int, like: torch.Tensor, what: str):
    """the uint8 [n] verdict buffer of a verification: a new one, or the caller's after the checks _want makes for limbs"""
    if out is None:
        return torch.empty(n, dtype=torch.uint8, device=like.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (n,) or out.device != like.device:
        raise SclError(ERR_SIZE_MISMATCH, f"{what}: out must be uint8 [n] on the signatures' device")
    return out


def ecdsa_verify(gtable, pk, sig, digests, scratch=None, out=None):
    """pk [1][12] (one key) or [n][12], signatures [n][8], digests uint8 [n][32] -> uint8 [n]: 1 accepted, 0 rejected, 2 s == 0"""
    n = sig.shape[0]
    _want(sig, (n, 8), "ecdsa_verify signatures")
    _points(pk, "ecdsa_verify pk")
    if pk.dim() != 2 or pk.shape[0] not in (1, n):
        raise SclError(ERR_SIZE_MISMATCH, "ecdsa_verify: one public key, or one per signature")
    _digest_rows(digests, n, "ecdsa_verify")
    scratch = _mul_scratch(scratch, n, sig, "ecdsa_verify")
    out = _verdicts(out, n, sig, "ecdsa_verify")
    _chk(lib.scl_hip_ecdsa_verify(_dev(out), _dev(sig), _dev(digests), _dev(pk), C.c_size_t(0 if pk.shape[0] == 1 else 1),
                                  _dev(gtable), _dev(scratch), C.c_size_t(n), _stream()))
    return out


def ecdsa_verify_base(gtable, qtable, sig, digests, out=None):
    """the verdicts of ecdsa_verify for ONE signer, from the window table of the signer's key (ec_base_table(pk))"""
    n = sig.shape[0]
    _want(sig, (n, 8), "ecdsa_verify_base signatures")
    _digest_rows(digests, n, "ecdsa_verify_base")
    if qtable.numel() * qtable.element_size() != lib.scl_hip_ec_base_table_bytes():
        raise SclError(ERR_SIZE_MISMATCH, "ecdsa_verify_base: qtable is not a window table")
    out = _verdicts(out, n, sig, "ecdsa_verify_base")
    _chk(lib.scl_hip_ecdsa_verify_base(_dev(out), _dev(sig), _dev(digests), _dev(qtable), _dev(gtable), C.c_size_t(n), _stream()))
    return out


def stream_copy(dst: torch.Tensor, src: torch.Tensor):
    _chk(lib.scl_hip_stream_copy(_dev(dst), _dev(src), C.c_size_t(src.numel() * src.element_size()), _stream()))


class Timer:
    """HIP-event timer on the stream the kernels are launched on (torch's current stream)"""

    def __init__(self):
        self._h = C.c_void_p()
        _chk(lib.scl_hip_timer_create(C.byref(self._h)))

    def start(self):
        _chk(lib.scl_hip_timer_start(self._h, _stream()))

    def stop(self):
        _chk(lib.scl_hip_timer_stop(self._h, _stream()))

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        _chk(lib.scl_hip_timer_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            lib.scl_hip_timer_destroy(self._h)
        except Exception:
            pass
