"""CPU-side checks of the comparison extension's boundary: libscl_hip_cmp.so exports exactly the prototypes of
include/scl_hip_cmp.h, the binding takes its ctypes prototypes from that header, and every error the header promises is decided on
the host, before a launch -- so each is reachable here, without a device, with pointers that are never dereferenced: the
GF(2^128) tag, a ring tag, w == 0, w >= B, B > |p| - 2, m outside 1..64, cnt < 2, an unknown flag or `what`, SCL_CMP_LT_ONLY where
more than one node comes out, NULL, misalignment, a stride below N and each forbidden overlap."""
import ctypes as C
import os
import re

import pytest

import cmp_support as CS
import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, PKG, check_exports, check_last_error_per_thread, check_latch_rule,
                         declared_symbols, expect, header, reaches_the_device_check)

CMP = CS.CMP
FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
TOP = {O.M61: 59, O.M127: 125, O.MONT128: 126, O.SECP256K1_SCALAR: 254, O.SECP256K1_FIELD: 254}     # |p| - 2; Mont128 at 2^128 - 159
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
STEP = 1 << 20
LAMBDA = (C.c_uint64 * (64 * 4))()          # host memory the first level may read: 64 elements of any field


@pytest.fixture(scope="module")
def cmp():
    import scl_amd.cmp
    return scl_amd.cmp


def esz(f):
    return 8 * O.LIMBS[f]


def ptrs():
    """d / out, cmod, status, csh / lt, bits / nodes / rlow, r2 / x: 1 MiB apart"""
    return [BASE + i * STEP for i in range(6)]


def first_args(f, N=8, rows=3, w=5, B=9, m=3, flags=0, p=None, lam=LAMBDA, **strides):
    d, cmod, status, csh, bits, r2 = p or ptrs()
    P = 1 if flags & 1 else 2 * ((w + 1) // 2)
    s = lambda name, default: strides.get(name, default)
    return (f, d, s("d_plane_stride", N), s("d_row_stride", max(P, 1) * N), cmod, status, csh, s("c_stride", N), lam, m, bits, s("bits_plane_stride", N),
            s("bits_row_stride", B * N), r2, s("r2_plane_stride", N), s("r2_row_stride", max(P, 1) * N), w, B, rows, N, flags, None)


def level_args(f, N=8, rows=3, cnt=3, flags=0, p=None, **strides):
    d, _, _, _, nodes, r2 = p or ptrs()
    P = 1 if flags & 1 else 2 * ((cnt + 1) // 2)
    s = lambda name, default: strides.get(name, default)
    return (f, d, s("d_plane_stride", N), s("d_row_stride", P * N), nodes, s("n_plane_stride", N), s("n_row_stride", 2 * max(cnt, 1) * N), r2,
            s("r2_plane_stride", N), s("r2_row_stride", P * N), cnt, rows, N, flags, None)


def finish_args(f, N=8, rows=3, w=5, what=1, p=None, **strides):
    out, cmod, status, lt, rlow, x = p or ptrs()
    s = lambda name: strides.get(name, N)
    return (f, out, s("out_stride"), lt, s("lt_stride"), cmod, status, rlow, s("rlow_stride"), x, s("x_stride"), w, what, rows, N, None)


def entry_points(cmp):
    return [(cmp.lib.scl_cmp_first_mask, first_args, b"first_mask"), (cmp.lib.scl_cmp_level_mask, level_args, b"level_mask"),
            (cmp.lib.scl_cmp_finish, finish_args, b"finish")]


def test_the_library_exports_the_header_and_nothing_else(cmp):
    check_exports(CMP, CS.SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    CS.check_engine_is_only_dependency()


def test_version_and_prototypes_come_from_the_header(cmp):
    """the binding compares the version before it looks up another symbol (scl_amd/cmp.py through the one loader, scl_amd/_abi.py)
    and types every prototype"""
    assert cmp.lib.scl_cmp_abi_version() == 1 and re.search(r"#define\s+SCL_CMP_ABI_VERSION\s+1\b", header(CMP))
    assert '_abi.declare(lib, _SO, "scl_hip_cmp.h", "scl_cmp_", "SCL_CMP_ABI_VERSION"' in open(os.path.join(PKG, "scl_amd", "cmp.py")).read()
    assert cmp._NPROTO == len(declared_symbols(CMP)) == 7
    assert cmp.lib.scl_cmp_last_error.restype is C.c_char_p and cmp.lib.scl_cmp_levels.restype is C.c_size_t and cmp.lib.scl_cmp_planes.restype is C.c_size_t
    z, v, i, u = C.c_size_t, C.c_void_p, C.c_int, C.c_uint
    assert list(cmp.lib.scl_cmp_first_mask.argtypes) == [i, v, z, z, v, v, v, z, v, z, v, z, z, v, z, z, z, z, z, z, u, v]
    assert list(cmp.lib.scl_cmp_level_mask.argtypes) == [i, v, z, z, v, z, z, v, z, z, z, z, z, u, v]
    assert list(cmp.lib.scl_cmp_finish.argtypes) == [i, v, z, v, z, v, v, v, z, v, z, z, i, z, z, v]
    with pytest.raises((C.ArgumentError, TypeError)):
        cmp.lib.scl_cmp_finish(0)                                         # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        cmp.lib.scl_cmp_level_mask("m61", *level_args(O.M61)[1:])         # not an int


def test_levels_and_planes_are_the_loop_that_defines_them(cmp):
    for w in range(1, 300):
        assert cmp.lib.scl_cmp_levels(w) == CS.model_levels(w) == max(1, (w - 1).bit_length()), w
        assert cmp.lib.scl_cmp_planes(w) == CS.model_planes(w), w
    assert cmp.planes(59) == 119 and cmp.levels(59) == 6 and cmp.planes(1) == cmp.planes(2) == 1 and cmp.levels(1) == cmp.levels(2) == 1
    assert cmp.planes(0) == 0 and cmp.levels(0) == 0


@pytest.mark.parametrize("f", FIELDS + [O.GF2_128] + RINGS)
def test_nothing_to_do_is_ok_at_once(cmp, f):
    """N == 0 or rows == 0: SCL_OK before any argument is looked at"""
    for N, rows in ((0, 3), (8, 0)):
        assert cmp.lib.scl_cmp_first_mask(f, None, 0, 0, None, None, None, 0, None, 0, None, 0, 0, None, 0, 0, 0, 999, rows, N, 99, None) == OK
        assert cmp.lib.scl_cmp_level_mask(f, None, 0, 0, None, 0, 0, None, 0, 0, 0, rows, N, 99, None) == OK
        assert cmp.lib.scl_cmp_finish(f, None, 0, None, 0, None, None, None, 0, None, 0, 0, 99, rows, N, None) == OK


def test_gf2_128_is_refused_with_its_reason(cmp):
    for fn, args, who in entry_points(cmp):
        expect(CMP, fn(*args(O.GF2_128)), ERR_BAD_ARG, who, b"SCL_GF2_128 is refused", b"no integers below a prime")


@pytest.mark.parametrize("tag", RINGS)
def test_a_ring_is_refused_with_its_reason(cmp, tag):
    for fn, args, who in entry_points(cmp):
        expect(CMP, fn(tag, *args(O.M61)[1:]), ERR_BAD_ARG, who, b"ring", b"not a field")


@pytest.mark.parametrize("tag", [-1, 6, 7, 0x100, 0x100 + 129, 0x7fffffff])
def test_unknown_tags(cmp, tag):
    for fn, args, who in entry_points(cmp):
        expect(CMP, fn(tag, *args(O.M61)[1:]), ERR_BAD_ARG, who, b"unknown field tag")


@pytest.mark.parametrize("f", FIELDS)
def test_counts_out_of_range_and_short_strides(cmp, f):
    """w == 0, w >= B, B > |p| - 2, m outside 1..64, cnt < 2, unknown flags and `what`, LT_ONLY with more than one node out, each
    with its reason; every stride below N"""
    lib, top = cmp.lib, TOP[f]
    expect(CMP, lib.scl_cmp_first_mask(*first_args(f, w=0)), ERR_BAD_ARG, b"first_mask: w == 0")
    expect(CMP, lib.scl_cmp_first_mask(*first_args(f, w=9, B=9)), ERR_BAD_ARG, b"first_mask: w >= B")
    expect(CMP, lib.scl_cmp_first_mask(*first_args(f, B=top + 1)), ERR_BAD_ARG, b"first_mask: B > |p| - 2", b"at most %d" % top)
    for m in (0, 65):
        expect(CMP, lib.scl_cmp_first_mask(*first_args(f, m=m)), ERR_BAD_ARG, b"first_mask: m must be in 1..64")
    expect(CMP, lib.scl_cmp_first_mask(*first_args(f, flags=2)), ERR_BAD_ARG, b"first_mask: unknown flag")
    expect(CMP, lib.scl_cmp_first_mask(*first_args(f, w=3, flags=1)), ERR_BAD_ARG, b"first_mask: SCL_CMP_LT_ONLY", b"single node", b"w <= 2")
    for cnt in (0, 1):
        expect(CMP, lib.scl_cmp_level_mask(*level_args(f, cnt=cnt)), ERR_BAD_ARG, b"level_mask: cnt < 2")
    expect(CMP, lib.scl_cmp_level_mask(*level_args(f, flags=4)), ERR_BAD_ARG, b"level_mask: unknown flag")
    expect(CMP, lib.scl_cmp_level_mask(*level_args(f, cnt=3, flags=1)), ERR_BAD_ARG, b"level_mask: SCL_CMP_LT_ONLY", b"single node", b"cnt == 2")
    expect(CMP, lib.scl_cmp_finish(*finish_args(f, w=0)), ERR_BAD_ARG, b"finish: w == 0")
    expect(CMP, lib.scl_cmp_finish(*finish_args(f, w=top)), ERR_BAD_ARG, b"finish: w >= |p| - 2", b"at most %d" % top)
    for what in (-1, 3):
        expect(CMP, lib.scl_cmp_finish(*finish_args(f, what=what)), ERR_BAD_ARG, b"finish: unknown `what`")
    for name in ("d_plane_stride", "d_row_stride", "c_stride", "bits_plane_stride", "bits_row_stride", "r2_plane_stride", "r2_row_stride"):
        expect(CMP, lib.scl_cmp_first_mask(*first_args(f, **{name: 7})), ERR_SIZE_MISMATCH, b"first_mask: " + name.encode() + b" < N")
    for name in ("d_plane_stride", "d_row_stride", "n_plane_stride", "n_row_stride", "r2_plane_stride", "r2_row_stride"):
        expect(CMP, lib.scl_cmp_level_mask(*level_args(f, **{name: 7})), ERR_SIZE_MISMATCH, b"level_mask: " + name.encode() + b" < N")
    for name in ("out_stride", "lt_stride", "rlow_stride", "x_stride"):
        expect(CMP, lib.scl_cmp_finish(*finish_args(f, **{name: 7})), ERR_SIZE_MISMATCH, b"finish: " + name.encode() + b" < N")
    expect(CMP, lib.scl_cmp_first_mask(*first_args(f, rows=2 ** 61, d_row_stride=2 ** 40)), ERR_BAD_ARG, b"first_mask", b"d_dev overflows")
    expect(CMP, lib.scl_cmp_level_mask(*level_args(f, rows=2 ** 61, n_row_stride=2 ** 40)), ERR_BAD_ARG, b"level_mask", b"overflows")
    expect(CMP, lib.scl_cmp_finish(*finish_args(f, rows=2 ** 61, out_stride=2 ** 40)), ERR_BAD_ARG, b"finish", b"overflows")


@pytest.mark.parametrize("f", FIELDS)
def test_null_and_misaligned_pointers(cmp, f):
    """every pointer must be there, status and lambda too (x only where `what` looks at it); the element pointers are aligned to
    the element (8 bytes for one limb, else 16); the status is bytes and may start anywhere; each is named"""
    off = 4 if O.LIMBS[f] == 1 else 8
    slots = {b"first_mask": {0: b"d_dev", 1: b"cmod_dev", 2: b"status_dev", 3: b"csh_dev", 4: b"bits_dev", 5: b"r2_dev"},
             b"level_mask": {0: b"d_dev", 4: b"nodes_dev", 5: b"r2_dev"},
             b"finish": {0: b"out_dev", 1: b"cmod_dev", 2: b"status_dev", 3: b"lt_dev", 4: b"rlow_dev", 5: b"x_dev"}}
    for fn, args, who in entry_points(cmp):
        for i, name in slots[who].items():
            p = ptrs()
            p[i] = None
            expect(CMP, fn(*args(f, p=p)), ERR_BAD_ARG, who, name, b"NULL")
            if name != b"status_dev":
                p = ptrs()
                p[i] += off
                expect(CMP, fn(*args(f, p=p)), ERR_BAD_ARG, who, name, b"aligned")
    expect(CMP, cmp.lib.scl_cmp_first_mask(*first_args(f, lam=None)), ERR_BAD_ARG, b"first_mask: lambda_host is NULL")


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps_and_the_allowed_aliases(cmp, f):
    """first_mask and level_mask: no output on an input or on another output; finish: out on cmod or the status, out on x, rlow
    or lt at an offset or under another stride -- refused with both operands named.  out == x, rlow or lt with one stride passes
    the checks, which shows as the call going on to ask for a device, where there is none"""
    import torch
    lib, e, N, rows = cmp.lib, esz(f), 8, 3
    d, cmod, status, csh, bits, r2 = ptrs()
    fm = lambda p: lib.scl_cmp_first_mask(*first_args(f, N=N, rows=rows, p=p))
    expect(CMP, fm([bits + 16 * e, cmod, status, csh, bits, r2]), ERR_BAD_ARG, b"first_mask: d_dev overlaps bits_dev")
    expect(CMP, fm([r2, cmod, status, csh, bits, r2]), ERR_BAD_ARG, b"first_mask: d_dev overlaps r2_dev")
    expect(CMP, fm([d, cmod, status, d + 16 * e, bits, r2]), ERR_BAD_ARG, b"first_mask: d_dev overlaps csh_dev")
    expect(CMP, fm([d, d + (rows * 6 * N - 1) * e, status, csh, bits, r2]), ERR_BAD_ARG, b"first_mask: d_dev overlaps cmod_dev")
    expect(CMP, fm([d, cmod, cmod + N * e - 1, csh, bits, r2]), ERR_BAD_ARG, b"first_mask: cmod_dev overlaps status_dev")
    expect(CMP, fm([d, csh + 8 * e, status, csh, bits, r2]), ERR_BAD_ARG, b"first_mask: cmod_dev overlaps csh_dev")
    expect(CMP, fm([d, cmod, bits + 5, csh, bits, r2]), ERR_BAD_ARG, b"first_mask: status_dev overlaps bits_dev")
    lm = lambda p: lib.scl_cmp_level_mask(*level_args(f, N=N, rows=rows, p=p))
    expect(CMP, lm([bits, cmod, status, csh, bits, r2]), ERR_BAD_ARG, b"level_mask: d_dev overlaps nodes_dev")
    expect(CMP, lm([d, cmod, status, csh, bits, d + (rows * 4 * N - 1) * e]), ERR_BAD_ARG, b"level_mask: d_dev overlaps r2_dev")
    out, cmod, status, lt, rlow, x = ptrs()
    fi = lambda p, **kw: lib.scl_cmp_finish(*finish_args(f, N=N, rows=rows, p=p, **kw))
    expect(CMP, fi([cmod, cmod, status, lt, rlow, x]), ERR_BAD_ARG, b"finish: out_dev overlaps cmod_dev")
    expect(CMP, fi([out, cmod, out + 3, lt, rlow, x]), ERR_BAD_ARG, b"finish: out_dev overlaps status_dev")
    expect(CMP, fi([x + 16, cmod, status, lt, rlow, x]), ERR_BAD_ARG, b"finish: out_dev overlaps x_dev", b"may coincide")
    expect(CMP, fi([x, cmod, status, lt, rlow, x], out_stride=N + 2), ERR_BAD_ARG, b"finish: out_dev overlaps x_dev", b"may coincide")
    expect(CMP, fi([rlow + 16, cmod, status, lt, rlow, x]), ERR_BAD_ARG, b"finish: out_dev overlaps rlow_dev", b"may coincide")
    expect(CMP, fi([lt + 16, cmod, status, lt, rlow, x]), ERR_BAD_ARG, b"finish: out_dev overlaps lt_dev", b"may coincide")
    if not torch.cuda.is_available():
        reaches_the_device_check(CMP, fi([x, cmod, status, lt, rlow, x]))                      # in place on x
        reaches_the_device_check(CMP, fi([rlow, cmod, status, lt, rlow, x]))                   # in place on rlow
        reaches_the_device_check(CMP, fi([lt, cmod, status, lt, rlow, x]))                     # in place on lt
        reaches_the_device_check(CMP, fi([x, cmod, status, lt, rlow, x], out_stride=N + 2, x_stride=N + 2))
        reaches_the_device_check(CMP, fi([out, cmod, status, lt, x, x]))                       # two inputs may share memory
        reaches_the_device_check(CMP, fi([out, cmod, status, lt, rlow, None], what=0))         # SCL_CMP_MOD does not look at x
        reaches_the_device_check(CMP, fm(ptrs()))
        reaches_the_device_check(CMP, lm(ptrs()))


@pytest.mark.parametrize("f", FIELDS)
def test_a_well_formed_call_needs_a_device(cmp, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    top = TOP[f]
    for w, B, flags in ((1, 2, 0), (1, 2, 1), (2, 3, 1), (top - 1, top, 0), (5, top, 0)):
        for m in (1, 64):
            expect(CMP, cmp.lib.scl_cmp_first_mask(*first_args(f, w=w, B=B, m=m, flags=flags, d_plane_stride=11, c_stride=12)), ERR_NO_DEVICE)
        for what in (0, 1, 2):
            expect(CMP, cmp.lib.scl_cmp_finish(*finish_args(f, w=w, what=what, out_stride=11, rlow_stride=12)), ERR_NO_DEVICE)
    for cnt, flags in ((2, 0), (2, 1), (3, 0), (256, 0)):
        expect(CMP, cmp.lib.scl_cmp_level_mask(*level_args(f, cnt=cnt, flags=flags, n_plane_stride=9)), ERR_NO_DEVICE)
    p = ptrs()
    p[2] += 3                                                                           # the status starts anywhere
    expect(CMP, cmp.lib.scl_cmp_first_mask(*first_args(f, N=1, p=p)), ERR_NO_DEVICE)
    expect(CMP, cmp.lib.scl_cmp_finish(*finish_args(f, N=1, p=p)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(cmp):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # calls that end at a later check when the modulus is in order
    check_latch_rule(CMP, [(cmp.lib.scl_cmp_first_mask, first_args(O.MONT128, w=0), b"w == 0", ERR_BAD_ARG),
                           (cmp.lib.scl_cmp_level_mask, level_args(O.MONT128, d_row_stride=7), b"d_row_stride", ERR_SIZE_MISMATCH),
                           (cmp.lib.scl_cmp_finish, finish_args(O.MONT128, out_stride=7), b"out_stride", ERR_SIZE_MISMATCH)])


def test_the_last_error_is_per_thread(cmp):
    lib = cmp.lib
    check_last_error_per_thread(CMP, (lib.scl_cmp_finish, finish_args(O.M61, rlow_stride=7)), b"finish: rlow_stride < N",
                                (lib.scl_cmp_first_mask, first_args(O.M61, w=0)), b"first_mask: w == 0")
