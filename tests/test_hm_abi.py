"""CPU-side checks of the honest-majority extension's boundary: libscl_hip_hm.so exports exactly the prototypes of
include/scl_hip_hm.h, the binding takes its ctypes prototypes from that header, scl_hm_double_blocks is the header's formula, and
every error the header promises is decided on the host, before a launch -- so each is reachable here, without a device, with
pointers that are never dereferenced."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, HM, check_engine_is_only_dependency, check_exports, check_latch_rule,
                         declared_symbols, expect, reaches_the_device_check)

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
SEED = b"hm abi"
TWO_PASS = 1
SYMBOLS = ["scl_hm_abi_version", "scl_hm_apply", "scl_hm_double_blocks", "scl_hm_double_scratch_bytes", "scl_hm_double_share_prg",
           "scl_hm_last_error", "scl_hm_mul_finish", "scl_hm_mul_mask"]


@pytest.fixture(scope="module")
def hm():
    import scl_amd.hm
    return scl_amd.hm


def esz(f):
    return 8 * O.LIMBS[f]


def deg_max(f):
    """the largest degree 2t the dealer takes: beyond it the engine's share call synchronises the stream"""
    return 16 if O.LIMBS[f] == 4 else 48


def ptrs(k, step=1 << 20):
    return [BASE + i * step for i in range(k)]


def double_args(f, N=8, t=1, n=4, stride=None, p=None, counter0=0, scratch=BASE + (8 << 20), flags=0):
    lo, hi = p or ptrs(2)
    return (f, lo, hi, N if stride is None else stride, N, t, n, SEED, len(SEED), counter0, scratch, flags, None)


def apply_args(f, N=8, m=3, n=4, batch=1, p=None, out_stride=None, in_stride=None, ldm=None, obs=None, ibs=None):
    out, inp, M = p or ptrs(3)
    os_, is_ = (N if out_stride is None else out_stride), (N if in_stride is None else in_stride)
    return (f, out, os_, m * os_ if obs is None else obs, inp, is_, n * is_ if ibs is None else ibs, M, n if ldm is None else ldm, m, n, batch, N, None)


def mask_args(f, N=8, rows=3, p=None, d_stride=None, op_stride=None):
    d, x, y, r2 = p or ptrs(4)
    return (f, d, N if d_stride is None else d_stride, x, y, r2, N if op_stride is None else op_stride, rows, N, None)


LAMBDA = np.zeros(64 * 4 + 4, dtype=np.uint64)


def finish_args(f, N=8, rows=3, m=4, p=None, z_stride=None, d_stride=None, r_stride=None, lam=True):
    z, dsh, r = p or ptrs(3)
    return (f, z, N if z_stride is None else z_stride, dsh, N if d_stride is None else d_stride, LAMBDA.ctypes.data if lam else None, m, r,
            N if r_stride is None else r_stride, rows, N, None)


def entry_points(hm):
    lib = hm.lib
    return [(lib.scl_hm_double_share_prg, double_args), (lib.scl_hm_apply, apply_args), (lib.scl_hm_mul_mask, mask_args),
            (lib.scl_hm_mul_finish, finish_args)]


def test_the_library_exports_the_header_and_nothing_else(hm):
    check_exports(HM, SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and not against the other extension libraries; every undefined
    scl_* symbol is a prototype of scl_hip.h"""
    check_engine_is_only_dependency(HM)


def test_version_and_prototypes_come_from_the_header(hm):
    assert hm.lib.scl_hm_abi_version() == 1
    assert hm._NPROTO == len(declared_symbols(HM)) == 8
    for name in declared_symbols(HM):
        assert getattr(hm.lib, name).argtypes is not None, name
    assert hm.lib.scl_hm_last_error.restype is C.c_char_p
    assert hm.lib.scl_hm_double_blocks.restype is C.c_size_t and hm.lib.scl_hm_double_scratch_bytes.restype is C.c_size_t
    d, a, k, fi = (hm.lib.scl_hm_double_share_prg.argtypes, hm.lib.scl_hm_apply.argtypes, hm.lib.scl_hm_mul_mask.argtypes,
                   hm.lib.scl_hm_mul_finish.argtypes)
    assert len(d) == 13 and d[0] is C.c_int and [d[i] for i in (1, 2, 7, 10, 12)] == [C.c_void_p] * 5 and d[9] is C.c_uint64 and d[11] is C.c_uint
    assert len(a) == 14 and [a[i] for i in (1, 4, 7, 13)] == [C.c_void_p] * 4 and [a[i] for i in (2, 3, 5, 6, 8, 9, 10, 11, 12)] == [C.c_size_t] * 9
    assert len(k) == 10 and [k[i] for i in (1, 3, 4, 5, 9)] == [C.c_void_p] * 5
    assert len(fi) == 12 and [fi[i] for i in (1, 3, 5, 7, 11)] == [C.c_void_p] * 5 and fi[6] is C.c_size_t
    with pytest.raises((C.ArgumentError, TypeError)):
        hm.lib.scl_hm_apply(0)                                     # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        hm.lib.scl_hm_double_share_prg(*double_args("m61"))        # not an int


def test_double_blocks_is_the_headers_formula(hm):
    """B = BPE + ceil((t+1) E / 16) + ceil((2t+1) E / 16) on a grid, the two worked values of the header; 0 for what the deal call
    refuses"""
    lib = hm.lib
    for f in FIELDS + RINGS:
        E = O.byte_size(f)
        for t in (0, 1, 2, 3, 4, 8, 9, 24, 25, 1000):
            for n in (2 * t, 2 * t + 1, 2 * t + 7, 65535, 65536):
                ok = f in FIELDS and 2 * t <= deg_max(f) and 2 * t < n <= 65535
                want = (E + 15) // 16 + ((t + 1) * E + 15) // 16 + ((2 * t + 1) * E + 15) // 16 if ok else 0
                assert lib.scl_hm_double_blocks(f, n, t) == want, (f, n, t)
    for tag in (-1, 6, 0x100, 0x100 + 129):
        assert lib.scl_hm_double_blocks(tag, 4, 1) == 0
    assert hm.double_blocks(O.M61, 10, 3) == 1 + 2 + 4 == 7
    assert hm.double_blocks(O.SECP256K1_SCALAR, 10, 3) == 2 + 8 + 14 == 24
    import scl_amd
    with pytest.raises(scl_amd.SclError):
        hm.double_blocks(O.Z2K(64), 4, 1)
    with pytest.raises(scl_amd.SclError):
        hm.double_blocks(O.M61, 6, 3)


def test_scratch_bytes_names_the_two_pass_cases(hm):
    """0 where the fused kernel deals the case (Mersenne61, Mersenne127, GF(2^128) at t <= 3 without flags bit 0), else
    (1 + 3t) N elements"""
    lib = hm.lib
    for f in FIELDS:
        for t in (0, 1, 2, 3, 4, 5, 8):
            fused = f in (O.M61, O.M127, O.GF2_128) and t <= 3
            assert lib.scl_hm_double_scratch_bytes(f, 257, 20, t, 0) == (0 if fused else (1 + 3 * t) * 257 * esz(f)), (f, t)
            assert lib.scl_hm_double_scratch_bytes(f, 257, 20, t, TWO_PASS) == (1 + 3 * t) * 257 * esz(f)
            assert lib.scl_hm_double_scratch_bytes(f, 257, 20, t, 2) == 0         # an undefined flags bit
            assert lib.scl_hm_double_scratch_bytes(f, 257, 2 * t, t, TWO_PASS) == 0   # n <= 2t
        tm = deg_max(f) // 2
        assert lib.scl_hm_double_scratch_bytes(f, 257, 60, tm, 0) == (1 + 3 * tm) * 257 * esz(f)
        assert lib.scl_hm_double_scratch_bytes(f, 257, 60, tm + 1, 0) == 0            # a refused degree
    assert lib.scl_hm_double_scratch_bytes(O.Z2K(64), 257, 4, 1, TWO_PASS) == 0


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_nothing_to_do_is_ok_at_once(hm, f):
    """N == 0 (and rows == 0, batch == 0): SCL_OK before any argument is looked at"""
    lib = hm.lib
    assert lib.scl_hm_double_share_prg(f, None, None, 0, 0, 9, 0, None, 0, 0, None, 7, None) == OK
    assert lib.scl_hm_apply(f, None, 0, 0, None, 0, 0, None, 0, 0, 0, 1, 0, None) == OK
    assert lib.scl_hm_apply(f, None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 8, None) == OK
    assert lib.scl_hm_mul_mask(f, None, 0, None, None, None, 0, 3, 0, None) == OK
    assert lib.scl_hm_mul_mask(f, None, 0, None, None, None, 0, 0, 8, None) == OK
    assert lib.scl_hm_mul_finish(f, None, 0, None, 0, None, 99, None, 0, 3, 0, None) == OK
    assert lib.scl_hm_mul_finish(f, None, 0, None, 0, None, 99, None, 0, 0, 8, None) == OK


@pytest.mark.parametrize("tag", RINGS + [-1, 6, 0x100, 0x100 + 129, 0x7fffffff])
def test_rings_and_unknown_tags(hm, tag):
    """Shamir needs a field: a ring is refused like an unknown tag"""
    for fn, args in entry_points(hm):
        expect(HM, fn(*args(tag)), ERR_BAD_ARG, b"unknown field tag")


@pytest.mark.parametrize("f", FIELDS)
def test_null_and_misaligned_pointers(hm, f):
    off = 4 if O.LIMBS[f] == 1 else 8          # one limb: 8-byte alignment; wider: 16
    for (fn, args), k in zip(entry_points(hm), (2, 3, 4, 3)):
        for i in range(k):
            p = ptrs(k)
            p[i] = None
            expect(HM, fn(*args(f, p=p)), ERR_BAD_ARG, b"NULL")
            p = ptrs(k)
            p[i] += off
            expect(HM, fn(*args(f, p=p)), ERR_BAD_ARG, b"aligned")
    expect(HM, hm.lib.scl_hm_mul_finish(*finish_args(f, lam=False)), ERR_BAD_ARG, b"NULL")


@pytest.mark.parametrize("f", FIELDS)
def test_strides_parties_thresholds_and_flags(hm, f):
    lib = hm.lib
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=8, stride=7)), ERR_SIZE_MISMATCH, b"stride < N")
    for n, t in ((0, 0), (2, 1), (6, 3), (1, 1)):                                  # n <= 2t: degree 2t could not be opened
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, n=n, t=t)), ERR_BAD_ARG, b"larger than 2t")
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, n=65536)), ERR_BAD_ARG, b"65535")
    # a degree at which the engine's share call would synchronise the stream is refused; the last one below it is not
    tm = deg_max(f) // 2
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, t=tm + 1, n=200)), ERR_BAD_ARG, b"degree 2t must be at most %d" % deg_max(f))
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, t=65535, n=200)), ERR_BAD_ARG, b"degree")
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, t=tm, n=200, scratch=None)), ERR_BAD_ARG, b"scratch")
    for flags in (2, 3, 0x80000000):
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, flags=flags)), ERR_BAD_ARG, b"flags")
    expect(HM, lib.scl_hm_apply(*apply_args(f, out_stride=7)), ERR_SIZE_MISMATCH, b"out_stride < N")
    expect(HM, lib.scl_hm_apply(*apply_args(f, in_stride=7)), ERR_SIZE_MISMATCH, b"in_stride < N")
    expect(HM, lib.scl_hm_apply(*apply_args(f, ldm=3)), ERR_SIZE_MISMATCH, b"ldm < n")
    for m, n in ((0, 4), (3, 0), (3, 65536)):
        expect(HM, lib.scl_hm_apply(*apply_args(f, m=m, n=n, ldm=max(n, 1))), ERR_BAD_ARG, b"at least 1")
    expect(HM, lib.scl_hm_mul_mask(*mask_args(f, d_stride=7)), ERR_SIZE_MISMATCH, b"d_stride < N")
    expect(HM, lib.scl_hm_mul_mask(*mask_args(f, op_stride=7)), ERR_SIZE_MISMATCH, b"op_stride < N")
    for kw, word in (("z_stride", b"z_stride < N"), ("d_stride", b"d_stride < N"), ("r_stride", b"r_stride < N")):
        expect(HM, lib.scl_hm_mul_finish(*finish_args(f, **{kw: 7})), ERR_SIZE_MISMATCH, word)
    for m in (0, 65, 1000):                                                        # lambda travels with the launch: 1..64
        expect(HM, lib.scl_hm_mul_finish(*finish_args(f, m=m)), ERR_BAD_ARG, b"1..64")
        assert b"scl_hip_shamir_recover" in lib.scl_hm_last_error() and b"scl_hip_ew" in lib.scl_hm_last_error()


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps_and_the_allowed_aliases(hm, f):
    """every forbidden overlap is refused; the allowed aliases (d == r2, z == r, equal strides) and back-to-back operands pass the
    checks -- which shows as the call going on to ask for a device, where there is none"""
    import torch
    no_gpu = not torch.cuda.is_available()
    lib, e, N = hm.lib, esz(f), 8
    # double share: lo / hi, the scratch against either
    n = 4
    for i, j in ((0, 1), (1, 0)):
        p = ptrs(2)
        p[j] = p[i] + ((n - 1) * N + N - 1) * e          # starts at the last element of the other matrix
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=N, n=n, p=p)), ERR_BAD_ARG, b"overlap")
        p[j] = p[i] + n * N * e                           # back to back is in order: the check AFTER the overlap check is met
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=N, n=n, p=p, counter0=2 ** 64 - 8)), ERR_BAD_ARG, b"wraps")
    need = lib.scl_hm_double_scratch_bytes(f, N, 12, 4, 0)
    assert need == 13 * N * e
    for k in range(2):
        p = ptrs(2)
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=N, n=12, t=4, p=p, scratch=p[k] + ((12 * N - 1) * e & ~15))), ERR_BAD_ARG,
               b"scratch overlaps")
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=N, n=12, t=4, p=p, scratch=p[k] - need + 16)), ERR_BAD_ARG, b"scratch overlaps")
    # apply: out against in and against M, with and without batches
    m, n = 3, 4
    out, inp, M = ptrs(3)
    expect(HM, lib.scl_hm_apply(*apply_args(f, N=N, p=[inp + (n * N - 1) * e, inp, M])), ERR_BAD_ARG, b"out overlaps in")
    expect(HM, lib.scl_hm_apply(*apply_args(f, N=N, p=[inp - (m * N - 1) * e, inp, M])), ERR_BAD_ARG, b"out overlaps in")
    expect(HM, lib.scl_hm_apply(*apply_args(f, N=N, p=[M + (m * n - 1) * e, inp, M])), ERR_BAD_ARG, b"out overlaps M")
    expect(HM, lib.scl_hm_apply(*apply_args(f, N=N, batch=5, p=[inp + (5 * n * N - 1) * e, inp, M])), ERR_BAD_ARG, b"out overlaps in")
    expect(HM, lib.scl_hm_apply(*apply_args(f, N=N, batch=5, p=[inp - (5 * m * N - 1) * e, inp, M])), ERR_BAD_ARG, b"out overlaps in")
    # mask: d against x and y; d == r2 only exactly
    d, x, y, r2 = ptrs(4)
    rows = 3
    for k, word in ((1, b"x or y"), (2, b"x or y"), (3, b"d overlaps r2")):
        for delta in ((rows * N - 1) * e, -(rows * N - 1) * e, 32 if k == 3 else 0):     # (d == r2 exactly is the allowed alias)
            p = [d, x, y, r2]
            p[k] = d + (delta & ~15 if delta > 0 else -((-delta) & ~15))
            expect(HM, lib.scl_hm_mul_mask(*mask_args(f, N=N, rows=rows, p=p)), ERR_BAD_ARG, word)
    expect(HM, lib.scl_hm_mul_mask(*mask_args(f, N=N, rows=rows, p=[d, x, y, d], d_stride=N + 2, op_stride=N)), ERR_BAD_ARG, b"d overlaps r2")
    # finish: z against dsh; z == r only exactly
    z, dsh, r = ptrs(3)
    expect(HM, lib.scl_hm_mul_finish(*finish_args(f, N=N, p=[dsh + ((4 * N - 1) * e & ~15), dsh, r])), ERR_BAD_ARG, b"z overlaps dsh")
    expect(HM, lib.scl_hm_mul_finish(*finish_args(f, N=N, p=[z, z, r])), ERR_BAD_ARG, b"z overlaps dsh")
    expect(HM, lib.scl_hm_mul_finish(*finish_args(f, N=N, p=[z, dsh, z + 16 * 2])), ERR_BAD_ARG, b"z overlaps r")
    expect(HM, lib.scl_hm_mul_finish(*finish_args(f, N=N, p=[z, dsh, z], z_stride=N + 2, r_stride=N)), ERR_BAD_ARG, b"z overlaps r")
    if no_gpu:
        reaches_the_device_check(HM, lib.scl_hm_mul_mask(*mask_args(f, N=N, rows=rows, p=[d, x, y, d])))                      # d == r2
        reaches_the_device_check(HM, lib.scl_hm_mul_mask(*mask_args(f, N=N, rows=rows, p=[d, x, y, d], d_stride=N + 2, op_stride=N + 2)))
        reaches_the_device_check(HM, lib.scl_hm_mul_finish(*finish_args(f, N=N, p=[z, dsh, z])))                              # z == r
        reaches_the_device_check(HM, lib.scl_hm_mul_finish(*finish_args(f, N=N, p=[z, dsh, z], z_stride=N + 2, r_stride=N + 2)))
        reaches_the_device_check(HM, lib.scl_hm_mul_mask(*mask_args(f, N=N, rows=rows, p=[d, d + rows * N * e, y, r2])))      # back to back
        reaches_the_device_check(HM, lib.scl_hm_apply(*apply_args(f, N=N, p=[inp + n * N * e, inp, M])))


def test_a_two_pass_case_without_scratch_names_the_size_it_needs(hm):
    lib = hm.lib
    cases = [(O.SECP256K1_SCALAR, 1, 0), (O.MONT128, 3, 0), (O.M61, 4, 0), (O.M61, 3, TWO_PASS), (O.GF2_128, 4, 0), (O.M127, 0, TWO_PASS)]
    for f, t, flags in cases:
        need = lib.scl_hm_double_scratch_bytes(f, 257, 20, t, flags)
        assert need == (1 + 3 * t) * 257 * esz(f)
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=257, t=t, n=20, scratch=None, flags=flags)), ERR_BAD_ARG, str(need).encode())
        assert b"scratch" in lib.scl_hm_last_error()
        expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=257, t=t, n=20, scratch=BASE + (8 << 20) + 8, flags=flags)), ERR_BAD_ARG,
               b"aligned")


def test_a_block_range_that_wraps_the_counter_is_refused(hm):
    expect(HM, hm.lib.scl_hm_double_share_prg(*double_args(O.M61, N=8, counter0=2 ** 64 - 8)), ERR_BAD_ARG, b"wraps")
    expect(HM, hm.lib.scl_hm_double_share_prg(*double_args(O.SECP256K1_FIELD, N=2 ** 60, stride=2 ** 60, n=4, counter0=0)), ERR_BAD_ARG)


@pytest.mark.parametrize("f", FIELDS)
def test_a_well_formed_call_needs_a_device(hm, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    lib = hm.lib
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=8, t=3, n=10, stride=11, counter0=2 ** 32 - 5)), ERR_NO_DEVICE)
    expect(HM, lib.scl_hm_double_share_prg(*double_args(f, N=8, t=4, n=9, stride=8, flags=TWO_PASS)), ERR_NO_DEVICE)
    expect(HM, lib.scl_hm_apply(*apply_args(f, N=8, m=7, n=10, batch=10, ldm=12, out_stride=9, in_stride=90)), ERR_NO_DEVICE)
    expect(HM, lib.scl_hm_mul_mask(*mask_args(f, d_stride=9, op_stride=11)), ERR_NO_DEVICE)
    expect(HM, lib.scl_hm_mul_finish(*finish_args(f, m=64, z_stride=9, d_stride=10, r_stride=11)), ERR_NO_DEVICE)
    expect(HM, lib.scl_hm_mul_finish(*finish_args(f, m=1)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(hm):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    lib = hm.lib
    # calls that end at a later check when the modulus is in order
    check_latch_rule(HM, [(lib.scl_hm_double_share_prg, double_args(O.MONT128, flags=2), b"flags", ERR_BAD_ARG),
                          (lib.scl_hm_apply, apply_args(O.MONT128, m=0), b"at least 1", ERR_BAD_ARG),
                          (lib.scl_hm_mul_mask, mask_args(O.MONT128, d_stride=7), b"d_stride", ERR_SIZE_MISMATCH),
                          (lib.scl_hm_mul_finish, finish_args(O.MONT128, m=65), b"1..64", ERR_BAD_ARG)])
