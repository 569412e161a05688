"""CPU-side checks of the random-bit extension's boundary: libscl_hip_rb.so exports exactly the prototypes of
include/scl_hip_rb.h, the binding takes its ctypes prototypes from that header, and every error the header promises is decided on
the host, before a launch -- so each is reachable here, without a device, with pointers that are never dereferenced: the
GF(2^128) tag, a ring tag, an unknown flag bit, NULL, misalignment, a stride below N and each forbidden overlap."""
import ctypes as C
import os
import re

import pytest

import oracle_lib as O
import rb_support as RBS
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, PKG, check_exports, check_last_error_per_thread, check_latch_rule,
                         declared_symbols, expect, header, reaches_the_device_check)

RB = RBS.RB
FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
STEP = 1 << 20


@pytest.fixture(scope="module")
def rb():
    import scl_amd.rb
    return scl_amd.rb


def esz(f):
    return 8 * O.LIMBS[f]


def ptrs():
    """out / b, status, a / u, r: 1 MiB apart"""
    return [BASE + i * STEP for i in range(4)]


def sqrt_args(f, N=8, p=None, flags=0):
    out, status, a, _ = p or ptrs()
    return (f, out, status, a, N, flags, None)


def bits_args(f, N=8, rows=3, p=None, b_stride=None, r_stride=None):
    b, status, u, r = p or ptrs()
    return (f, b, N if b_stride is None else b_stride, status, u, r, N if r_stride is None else r_stride, rows, N, None)


def entry_points(rb):
    return [(rb.lib.scl_rb_sqrt, sqrt_args, b"sqrt"), (rb.lib.scl_rb_bits_finish, bits_args, b"bits_finish")]


def test_the_library_exports_the_header_and_nothing_else(rb):
    check_exports(RB, RBS.SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    RBS.check_engine_is_only_dependency()


def test_version_and_prototypes_come_from_the_header(rb):
    """the binding compares the version before it looks up another symbol (scl_amd/rb.py through the one loader, scl_amd/_abi.py)
    and types every prototype"""
    assert rb.lib.scl_rb_abi_version() == 1 and re.search(r"#define\s+SCL_RB_ABI_VERSION\s+1\b", header(RB))
    assert re.search(r"#define\s+SCL_RB_ODD_ROOT\s+1u", header(RB)) and re.search(r"#define\s+SCL_RB_INVERSE\s+2u", header(RB))
    assert (rb.ODD_ROOT, rb.INVERSE) == (RBS.ODD_ROOT, RBS.INVERSE) == (1, 2)
    assert '_abi.declare(lib, _SO, "scl_hip_rb.h", "scl_rb_", "SCL_RB_ABI_VERSION"' in open(os.path.join(PKG, "scl_amd", "rb.py")).read()
    assert rb._NPROTO == len(declared_symbols(RB)) == 4
    assert rb.lib.scl_rb_last_error.restype is C.c_char_p
    s, b = rb.lib.scl_rb_sqrt.argtypes, rb.lib.scl_rb_bits_finish.argtypes
    assert list(s) == [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint, C.c_void_p]
    assert list(b) == [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]
    with pytest.raises((C.ArgumentError, TypeError)):
        rb.lib.scl_rb_sqrt(0)                                       # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        rb.lib.scl_rb_bits_finish("m61", *bits_args(O.M61)[1:])     # not an int


@pytest.mark.parametrize("f", FIELDS + [O.GF2_128] + RINGS)
def test_nothing_to_do_is_ok_at_once(rb, f):
    """N == 0 or rows == 0: SCL_OK before any argument is looked at"""
    assert rb.lib.scl_rb_sqrt(f, None, None, None, 0, 9, None) == OK
    assert rb.lib.scl_rb_bits_finish(f, None, 0, None, None, None, 0, 3, 0, None) == OK
    assert rb.lib.scl_rb_bits_finish(f, None, 0, None, None, None, 0, 0, 8, None) == OK


def test_gf2_128_is_refused_with_its_reason(rb):
    for fn, args, who in entry_points(rb):
        expect(RB, fn(*args(O.GF2_128)), ERR_BAD_ARG, who, b"SCL_GF2_128 is refused", b"bijection")


@pytest.mark.parametrize("tag", RINGS)
def test_a_ring_is_refused_with_its_reason(rb, tag):
    for fn, args, who in entry_points(rb):
        expect(RB, fn(tag, *args(O.M61)[1:]), ERR_BAD_ARG, who, b"ring", b"not a field")


@pytest.mark.parametrize("tag", [-1, 6, 7, 0x100, 0x100 + 129, 0x7fffffff])
def test_unknown_tags(rb, tag):
    for fn, args, who in entry_points(rb):
        expect(RB, fn(tag, *args(O.M61)[1:]), ERR_BAD_ARG, who, b"unknown field tag")


@pytest.mark.parametrize("f", FIELDS)
def test_unknown_flag_bits_and_short_strides(rb, f):
    lib = rb.lib
    for flags in (4, 8, 7, 1 << 31):
        expect(RB, lib.scl_rb_sqrt(*sqrt_args(f, flags=flags)), ERR_BAD_ARG, b"sqrt: unknown flags bit")
    expect(RB, lib.scl_rb_bits_finish(*bits_args(f, b_stride=7)), ERR_SIZE_MISMATCH, b"bits_finish: b_stride < N")
    expect(RB, lib.scl_rb_bits_finish(*bits_args(f, r_stride=7)), ERR_SIZE_MISMATCH, b"bits_finish: r_stride < N")
    expect(RB, lib.scl_rb_bits_finish(*bits_args(f, rows=2 ** 61, b_stride=2 ** 40, r_stride=2 ** 40)), ERR_BAD_ARG, b"bits_finish", b"overflows")


@pytest.mark.parametrize("f", FIELDS)
def test_null_and_misaligned_pointers(rb, f):
    """every pointer must be there, status too; the element pointers are aligned to the element (8 bytes for one limb, else 16);
    the status is bytes and may start anywhere; each is named"""
    off = 4 if O.LIMBS[f] == 1 else 8
    for (fn, args, who), names in zip(entry_points(rb), ([b"out_dev", b"status_dev", b"a_dev"], [b"b_dev", b"status_dev", b"u_dev", b"r_dev"])):
        for i, name in enumerate(names):
            p = ptrs()
            p[i] = None
            expect(RB, fn(*args(f, p=p)), ERR_BAD_ARG, who, name, b"NULL")
            if name != b"status_dev":
                p = ptrs()
                p[i] += off
                expect(RB, fn(*args(f, p=p)), ERR_BAD_ARG, who, name, b"aligned")


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps_and_the_allowed_aliases(rb, f):
    """sqrt: out on a at an offset, status on out or a; bits_finish: b on u, b on r at an offset or under another stride, status on
    b, u or r -- refused with both operands named.  out == a and b == r with one stride pass the checks, which shows as the call
    going on to ask for a device, where there is none"""
    import torch
    lib, e, N, rows = rb.lib, esz(f), 8, 3
    out, status, a, r = ptrs()
    sq = lambda *p: lib.scl_rb_sqrt(*sqrt_args(f, N=N, p=list(p) + [r]))
    expect(RB, sq(a + 16, status, a), ERR_BAD_ARG, b"sqrt: out_dev overlaps a_dev", b"may coincide")
    expect(RB, sq(a - (N - 1) * e, status, a), ERR_BAD_ARG, b"sqrt: out_dev overlaps a_dev")
    expect(RB, sq(out, out + N * e - 1, a), ERR_BAD_ARG, b"sqrt: out_dev overlaps status_dev")
    expect(RB, sq(out, a, a), ERR_BAD_ARG, b"sqrt: a_dev overlaps status_dev")
    expect(RB, sq(out, a - N + 1, a), ERR_BAD_ARG, b"sqrt: a_dev overlaps status_dev")
    bf = lambda b, st, u, rr, bs=N, rs=N: lib.scl_rb_bits_finish(*bits_args(f, N=N, rows=rows, p=[b, st, u, rr], b_stride=bs, r_stride=rs))
    expect(RB, bf(a, status, a, r), ERR_BAD_ARG, b"bits_finish: b_dev overlaps u_dev")
    expect(RB, bf(a - (rows * N - 1) * e, status, a, r), ERR_BAD_ARG, b"bits_finish: b_dev overlaps u_dev")
    expect(RB, bf(out, status, out + 16 * e, r, bs=64), ERR_BAD_ARG, b"bits_finish: b_dev overlaps u_dev")      # a pitched b covers its gaps
    expect(RB, bf(r + 16, status, a, r), ERR_BAD_ARG, b"bits_finish: b_dev overlaps r_dev", b"may coincide")
    expect(RB, bf(r, status, a, r, bs=N + 2, rs=N), ERR_BAD_ARG, b"bits_finish: b_dev overlaps r_dev", b"may coincide")
    expect(RB, bf(out, out, a, r), ERR_BAD_ARG, b"bits_finish: b_dev overlaps status_dev")
    expect(RB, bf(out, a + 3, a, r), ERR_BAD_ARG, b"bits_finish: u_dev overlaps status_dev")
    expect(RB, bf(out, r + rows * N * e - 1, a, r), ERR_BAD_ARG, b"bits_finish: r_dev overlaps status_dev")
    if not torch.cuda.is_available():
        reaches_the_device_check(RB, sq(a, status, a))                                   # in place
        reaches_the_device_check(RB, sq(out, out + N * e, a))                            # back to back
        reaches_the_device_check(RB, bf(r, status, a, r))                                # in place, one stride
        reaches_the_device_check(RB, bf(r, status, a, r, bs=N + 2, rs=N + 2))
        reaches_the_device_check(RB, bf(out, status, r, r))                              # two inputs may share memory


@pytest.mark.parametrize("f", FIELDS)
def test_a_well_formed_call_needs_a_device(rb, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    for flags in (0, 1, 2, 3):
        expect(RB, rb.lib.scl_rb_sqrt(*sqrt_args(f, flags=flags)), ERR_NO_DEVICE)
    for rows in (1, 3, 17):
        expect(RB, rb.lib.scl_rb_bits_finish(*bits_args(f, rows=rows, b_stride=11, r_stride=12)), ERR_NO_DEVICE)
    p = ptrs()
    p[1] += 3                                                                           # the status starts anywhere
    expect(RB, rb.lib.scl_rb_sqrt(*sqrt_args(f, N=1, p=p)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(rb):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # calls that end at a later check when the modulus is in order
    check_latch_rule(RB, [(rb.lib.scl_rb_sqrt, sqrt_args(O.MONT128, flags=4), b"flags", ERR_BAD_ARG),
                          (rb.lib.scl_rb_bits_finish, bits_args(O.MONT128, b_stride=7), b"b_stride", ERR_SIZE_MISMATCH)])


def test_the_last_error_is_per_thread(rb):
    lib = rb.lib
    check_last_error_per_thread(RB, (lib.scl_rb_bits_finish, bits_args(O.M61, r_stride=7)), b"bits_finish: r_stride < N",
                                (lib.scl_rb_sqrt, sqrt_args(O.M61, flags=4)), b"sqrt: unknown flags")
