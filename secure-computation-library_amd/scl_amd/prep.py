"""scl_amd.prep -- Python harness over libscl_hip_prep.so, the preprocessing extension beside the engine (include/scl_hip_prep.h).

The trusted dealer of multiplication triples ([a], [b], [c = a b]) in the reference's PRG order (test/scl/protocol/triple.h:37-48):
`deal_triples_additive` and `deal_triples_shamir` deal N triples among n parties from one seed, the triples a reference run with
that seed deals one after another.  What they return goes to scl_amd.mpc.beaver_mask / beaver_finish and to the engine's recover
calls as it lies.  Plumbing only, like scl_amd itself: torch device buffers and the current HIP stream go to the C ABI; there is
no CPU or torch fallback.  Tensors are those of scl_amd: int64 limbs, a share matrix SoA `[party][triple][limb]`.
"""
from __future__ import annotations

import ctypes as C

import torch

import scl_amd as _scl  # the engine first: libscl_hip_prep.so links against libscl_hip.so and finds it loaded
from scl_amd import _abi

lib, _SO = _abi.load("scl_hip_prep")

ADDITIVE, SHAMIR = 0, 1     # scheme of triple_blocks
TWO_PASS = 1                # flags bit 0 of deal_triples_shamir


# argtypes / restype of every entry point from the prototypes of include/scl_hip_prep.h; the boundary's version is compared first
_NPROTO = _abi.declare(lib, _SO, "scl_hip_prep.h", "scl_prep_", "SCL_PREP_ABI_VERSION", "scl_amd.prep")


_chk = _scl._checker(lib.scl_prep_last_error)


def triple_blocks(field, scheme: int, n: int, t: int = 0) -> int:
    """AES blocks one triple consumes (B of include/scl_hip_prep.h): a PRG that dealt N triples has advanced by N * B; triples
    [f, f + k) of a long run are the call with counter0 + f * B.  Raises for arguments the deal calls refuse."""
    B = lib.scl_prep_triple_blocks(field, scheme, n, t)
    if B == 0:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"triple_blocks: field {field:#x}, scheme {scheme}, n = {n}, t = {t} is not a case the dealer accepts")
    return B


def triples_scratch_bytes(field, N: int, n: int, t: int, flags: int = 0) -> int:
    """bytes of scratch deal_triples_shamir needs for this case: 0 where the fused kernel deals it"""
    return lib.scl_prep_triples_scratch_bytes(field, N, n, t, flags)


def _outs(field, n, N, out, device, what):
    L = _scl.limbs(field)
    if out is None:
        abc = torch.empty(3, n, N, L, dtype=torch.int64, device=device)
        out = (abc[0], abc[1], abc[2])
    if len(out) != 3:
        raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what}: out is the three matrices (a, b, c)")
    ptrs, stride = [], None
    for name, m in zip("abc", out):
        _scl._want(m, (n, N, L), f"{what} out {name}", out[0])
        p, s = _scl._dev_rows(m)
        if stride is not None and s != stride:
            raise _scl.SclError(_scl.ERR_BAD_ARG, f"{what} out {name}: row stride {s}, a has {stride} (the matrices share one stride)")
        stride = s
        ptrs.append(p)
    return tuple(out), ptrs, stride


def deal_triples_additive(field, N: int, n: int, seed: bytes, counter0: int = 0, out=None, device="cuda"):
    """N additive triples among n >= 2 parties (scl_prep_triples_additive_prg): returns (a, b, c), each [n][N][L], the rows of
    party i being its shares -- sum_i a[i] * sum_i b[i] = sum_i c[i].  `out`: three such tensors of one row stride."""
    out, ptrs, stride = _outs(field, n, N, out, device, "deal_triples_additive")
    _chk(lib.scl_prep_triples_additive_prg(field, *ptrs, C.c_size_t(stride), C.c_size_t(N), C.c_size_t(n), seed, C.c_size_t(len(seed)),
                                           C.c_uint64(counter0), _scl._stream()))
    return out


def deal_triples_shamir(field, N: int, t: int, n: int, seed: bytes, counter0: int = 0, out=None, scratch=None, flags: int = 0, device="cuda"):
    """N Shamir (n, t) triples at the nodes 1..n (scl_prep_triples_shamir_prg): returns (a, b, c), each [n][N][L].  Where the case
    takes the two-pass path (triples_scratch_bytes > 0) the scratch is `scratch` -- an int64 tensor of at least that many bytes --
    or allocated here; pass one when the call is captured into a graph."""
    out, ptrs, stride = _outs(field, n, N, out, device, "deal_triples_shamir")
    need = triples_scratch_bytes(field, N, n, t, flags)
    sp = None
    if need:
        if scratch is None:
            scratch = torch.empty(need // 8, dtype=torch.int64, device=out[0].device)
        if scratch.dtype != torch.int64 or scratch.numel() * 8 < need or scratch.device != out[0].device:
            raise _scl.SclError(_scl.ERR_SIZE_MISMATCH, f"deal_triples_shamir: scratch must be an int64 tensor of at least {need} bytes on {out[0].device}")
        sp = _scl._dev(scratch)
    _chk(lib.scl_prep_triples_shamir_prg(field, *ptrs, C.c_size_t(stride), C.c_size_t(N), C.c_size_t(t), C.c_size_t(n), seed,
                                         C.c_size_t(len(seed)), C.c_uint64(counter0), sp, C.c_uint(flags), _scl._stream()))
    return out
