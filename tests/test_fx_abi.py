"""CPU-side checks of the fixed-point extension's boundary: libscl_hip_fx.so exports exactly the prototypes of
include/scl_hip_fx.h, the binding takes its ctypes prototypes from that header, and every error the header promises is decided on
the host, before a launch -- so each is reachable here, without a device, with pointers that are never dereferenced: the
GF(2^128) tag, a ring tag, a bit count, k or shift out of range, m outside 1..64, NULL, misalignment, a stride below N and each
forbidden overlap."""
import ctypes as C
import os
import re

import pytest

import fx_support as FXS
import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, PKG, check_exports, check_last_error_per_thread, check_latch_rule,
                         declared_symbols, expect, header, reaches_the_device_check)

FX = FXS.FX
FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
STEP = 1 << 20
LAMBDA = (C.c_uint64 * (64 * 4))()          # host memory the finish may read: 64 elements of any field


@pytest.fixture(scope="module")
def fx():
    import scl_amd.fx
    return scl_amd.fx


def esz(f):
    return 8 * O.LIMBS[f]


def ptrs():
    """out / c / y, rlow, x, bits / csh, status: 1 MiB apart"""
    return [BASE + i * STEP for i in range(5)]


def compose_args(f, N=8, rows=3, B=5, p=None, out_stride=None, plane_stride=None, row_stride=None):
    out, _, _, bits, _ = p or ptrs()
    return (f, out, N if out_stride is None else out_stride, bits, N if plane_stride is None else plane_stride,
            B * N if row_stride is None else row_stride, B, rows, N, None)


def mask_args(f, N=8, rows=3, B=5, k=4, shift=2, p=None, c_stride=None, rlow_stride=None, x_stride=None, plane_stride=None, row_stride=None):
    c, rlow, x, bits, _ = p or ptrs()
    s = lambda v: N if v is None else v
    return (f, c, s(c_stride), rlow, s(rlow_stride), x, s(x_stride), bits, s(plane_stride), B * N if row_stride is None else row_stride, k, shift, B,
            rows, N, None)


def finish_args(f, N=8, rows=3, B=5, shift=2, m=3, p=None, y_stride=None, c_stride=None, x_stride=None, rlow_stride=None, lam=LAMBDA):
    y, rlow, x, csh, status = p or ptrs()
    s = lambda v: N if v is None else v
    return (f, y, s(y_stride), status, csh, s(c_stride), lam, m, x, s(x_stride), rlow, s(rlow_stride), shift, B, rows, N, None)


def entry_points(fx):
    return [(fx.lib.scl_fx_compose, compose_args, b"compose"), (fx.lib.scl_fx_trunc_mask, mask_args, b"trunc_mask"),
            (fx.lib.scl_fx_trunc_finish, finish_args, b"trunc_finish")]


def test_the_library_exports_the_header_and_nothing_else(fx):
    check_exports(FX, FXS.SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    FXS.check_engine_is_only_dependency()


def test_version_and_prototypes_come_from_the_header(fx):
    """the binding compares the version before it looks up another symbol (scl_amd/fx.py through the one loader, scl_amd/_abi.py)
    and types every prototype"""
    assert fx.lib.scl_fx_abi_version() == 1 and re.search(r"#define\s+SCL_FX_ABI_VERSION\s+1\b", header(FX))
    assert '_abi.declare(lib, _SO, "scl_hip_fx.h", "scl_fx_", "SCL_FX_ABI_VERSION"' in open(os.path.join(PKG, "scl_amd", "fx.py")).read()
    assert fx._NPROTO == len(declared_symbols(FX)) == 6
    assert fx.lib.scl_fx_last_error.restype is C.c_char_p and fx.lib.scl_fx_max_bits.restype is C.c_size_t
    z, v, i = C.c_size_t, C.c_void_p, C.c_int
    assert list(fx.lib.scl_fx_compose.argtypes) == [i, v, z, v, z, z, z, z, z, v]
    assert list(fx.lib.scl_fx_trunc_mask.argtypes) == [i, v, z, v, z, v, z, v, z, z, z, z, z, z, z, v]
    assert list(fx.lib.scl_fx_trunc_finish.argtypes) == [i, v, z, v, v, z, v, z, v, z, v, z, z, z, z, z, v]
    with pytest.raises((C.ArgumentError, TypeError)):
        fx.lib.scl_fx_compose(0)                                       # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        fx.lib.scl_fx_trunc_mask("m61", *mask_args(O.M61)[1:])         # not an int


def test_max_bits_is_the_primes_bit_length_less_two(fx):
    import scl_amd as scl
    lib = fx.lib
    assert [lib.scl_fx_max_bits(f) for f in (O.M61, O.M127, O.SECP256K1_SCALAR, O.SECP256K1_FIELD)] == [59, 125, 254, 254]
    assert [lib.scl_fx_max_bits(t) for t in [O.GF2_128, -1, 6, 0x100] + RINGS] == [0] * 8
    try:
        for p in (FXS.MONT_P0, FXS.MONT_P1):
            scl.set_mont128_prime(p)
            assert lib.scl_fx_max_bits(O.MONT128) == FXS.max_bits(p) == fx.max_bits(O.MONT128)
    finally:
        scl.set_mont128_prime(FXS.MONT_P0)


@pytest.mark.parametrize("f", FIELDS + [O.GF2_128] + RINGS)
def test_nothing_to_do_is_ok_at_once(fx, f):
    """N == 0 or rows == 0: SCL_OK before any argument is looked at"""
    for N, rows in ((0, 3), (8, 0)):
        assert fx.lib.scl_fx_compose(f, None, 0, None, 0, 0, 999, rows, N, None) == OK
        assert fx.lib.scl_fx_trunc_mask(f, None, 0, None, 0, None, 0, None, 0, 0, 0, 0, 999, rows, N, None) == OK
        assert fx.lib.scl_fx_trunc_finish(f, None, 0, None, None, 0, None, 0, None, 0, None, 0, 0, 999, rows, N, None) == OK


def test_gf2_128_is_refused_with_its_reason(fx):
    for fn, args, who in entry_points(fx):
        expect(FX, fn(*args(O.GF2_128)), ERR_BAD_ARG, who, b"SCL_GF2_128 is refused", b"no integers below a prime")


@pytest.mark.parametrize("tag", RINGS)
def test_a_ring_is_refused_with_its_reason(fx, tag):
    for fn, args, who in entry_points(fx):
        expect(FX, fn(tag, *args(O.M61)[1:]), ERR_BAD_ARG, who, b"ring", b"not a field")


@pytest.mark.parametrize("tag", [-1, 6, 7, 0x100, 0x100 + 129, 0x7fffffff])
def test_unknown_tags(fx, tag):
    for fn, args, who in entry_points(fx):
        expect(FX, fn(tag, *args(O.M61)[1:]), ERR_BAD_ARG, who, b"unknown field tag")


@pytest.mark.parametrize("f", FIELDS)
def test_counts_out_of_range_and_short_strides(fx, f):
    """shift == 0, shift >= k, k > B, B > max, m outside 1..64, each with its reason; every stride below N"""
    lib = fx.lib
    top = lib.scl_fx_max_bits(f)
    expect(FX, lib.scl_fx_compose(*compose_args(f, B=0)), ERR_BAD_ARG, b"compose: B must be in 1..%d" % top)
    expect(FX, lib.scl_fx_compose(*compose_args(f, B=top + 1)), ERR_BAD_ARG, b"compose: B must be in 1..%d" % top)
    expect(FX, lib.scl_fx_trunc_mask(*mask_args(f, shift=0)), ERR_BAD_ARG, b"trunc_mask: shift == 0")
    expect(FX, lib.scl_fx_trunc_mask(*mask_args(f, k=4, shift=4)), ERR_BAD_ARG, b"trunc_mask: shift >= k")
    expect(FX, lib.scl_fx_trunc_mask(*mask_args(f, k=6, B=5)), ERR_BAD_ARG, b"trunc_mask: k > B")
    expect(FX, lib.scl_fx_trunc_mask(*mask_args(f, k=top + 1, B=top + 1)), ERR_BAD_ARG, b"trunc_mask: B > scl_fx_max_bits", b"at most %d" % top)
    expect(FX, lib.scl_fx_trunc_finish(*finish_args(f, shift=0)), ERR_BAD_ARG, b"trunc_finish: shift == 0")
    expect(FX, lib.scl_fx_trunc_finish(*finish_args(f, shift=5, B=5)), ERR_BAD_ARG, b"trunc_finish: shift >= B")
    expect(FX, lib.scl_fx_trunc_finish(*finish_args(f, B=top + 1)), ERR_BAD_ARG, b"trunc_finish: B > scl_fx_max_bits")
    for m in (0, 65):
        expect(FX, lib.scl_fx_trunc_finish(*finish_args(f, m=m)), ERR_BAD_ARG, b"trunc_finish: m must be in 1..64")
    expect(FX, lib.scl_fx_compose(*compose_args(f, out_stride=7)), ERR_SIZE_MISMATCH, b"compose: out_stride < N")
    expect(FX, lib.scl_fx_compose(*compose_args(f, plane_stride=7)), ERR_SIZE_MISMATCH, b"compose: plane_stride < N")
    expect(FX, lib.scl_fx_compose(*compose_args(f, row_stride=7)), ERR_SIZE_MISMATCH, b"compose: row_stride < N")
    for name in ("c_stride", "rlow_stride", "x_stride", "plane_stride", "row_stride"):
        expect(FX, lib.scl_fx_trunc_mask(*mask_args(f, **{name: 7})), ERR_SIZE_MISMATCH, b"trunc_mask: " + name.encode() + b" < N")
    for name in ("y_stride", "c_stride", "x_stride", "rlow_stride"):
        expect(FX, lib.scl_fx_trunc_finish(*finish_args(f, **{name: 7})), ERR_SIZE_MISMATCH, b"trunc_finish: " + name.encode() + b" < N")
    expect(FX, lib.scl_fx_compose(*compose_args(f, rows=2 ** 61, row_stride=2 ** 40)), ERR_BAD_ARG, b"compose", b"overflows")
    expect(FX, lib.scl_fx_trunc_finish(*finish_args(f, rows=2 ** 61, y_stride=2 ** 40)), ERR_BAD_ARG, b"trunc_finish", b"overflows")


@pytest.mark.parametrize("f", FIELDS)
def test_null_and_misaligned_pointers(fx, f):
    """every pointer must be there, status and lambda too; the element pointers are aligned to the element (8 bytes for one limb,
    else 16); the status is bytes and may start anywhere; each is named"""
    off = 4 if O.LIMBS[f] == 1 else 8
    slots = {b"compose": {0: b"out_dev", 3: b"bits_dev"}, b"trunc_mask": {0: b"c_dev", 1: b"rlow_dev", 2: b"x_dev", 3: b"bits_dev"},
             b"trunc_finish": {0: b"y_dev", 1: b"rlow_dev", 2: b"x_dev", 3: b"csh_dev", 4: b"status_dev"}}
    for fn, args, who in entry_points(fx):
        for i, name in slots[who].items():
            p = ptrs()
            p[i] = None
            expect(FX, fn(*args(f, p=p)), ERR_BAD_ARG, who, name, b"NULL")
            if name != b"status_dev":
                p = ptrs()
                p[i] += off
                expect(FX, fn(*args(f, p=p)), ERR_BAD_ARG, who, name, b"aligned")
    expect(FX, fx.lib.scl_fx_trunc_finish(*finish_args(f, lam=None)), ERR_BAD_ARG, b"trunc_finish: lambda_host is NULL")


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps_and_the_allowed_aliases(fx, f):
    """compose: out on the planes; trunc_mask: c on x at an offset or under another stride, c on rlow, c or rlow on the planes,
    rlow on x; trunc_finish: y on csh, y on x or rlow at an offset, status on anything -- refused with both operands named.  c == x
    and y == x or y == rlow with one stride pass the checks, which shows as the call going on to ask for a device, where there is
    none"""
    import torch
    lib, e, N, rows, B = fx.lib, esz(f), 8, 3, 5
    out, rlow, x, bits, status = ptrs()
    co = lambda o, b: lib.scl_fx_compose(*compose_args(f, N=N, rows=rows, B=B, p=[o, rlow, x, b, status]))
    expect(FX, co(bits, bits), ERR_BAD_ARG, b"compose: out_dev overlaps bits_dev")
    expect(FX, co(bits + (rows * B * N - 1) * e, bits), ERR_BAD_ARG, b"compose: out_dev overlaps bits_dev")
    mk = lambda c, lo, xx, b, cs=N, xs=N: lib.scl_fx_trunc_mask(*mask_args(f, N=N, rows=rows, B=B, p=[c, lo, xx, b, status], c_stride=cs, x_stride=xs))
    expect(FX, mk(x + 16, rlow, x, bits), ERR_BAD_ARG, b"trunc_mask: c_dev overlaps x_dev", b"may coincide")
    expect(FX, mk(x, rlow, x, bits, cs=N + 2), ERR_BAD_ARG, b"trunc_mask: c_dev overlaps x_dev", b"may coincide")
    expect(FX, mk(out, out, x, bits), ERR_BAD_ARG, b"trunc_mask: c_dev overlaps rlow_dev")
    expect(FX, mk(out, x, x, bits), ERR_BAD_ARG, b"trunc_mask: x_dev overlaps rlow_dev")
    expect(FX, mk(bits + 16 * e, rlow, x, bits), ERR_BAD_ARG, b"trunc_mask: c_dev overlaps bits_dev")
    expect(FX, mk(out, bits + (rows * B * N - 1) * e, x, bits), ERR_BAD_ARG, b"trunc_mask: rlow_dev overlaps bits_dev")
    fi = lambda y, lo, xx, cs, st, ys=N, xs=N: lib.scl_fx_trunc_finish(*finish_args(f, N=N, rows=rows, B=B, p=[y, lo, xx, cs, st], y_stride=ys, x_stride=xs))
    expect(FX, fi(bits, rlow, x, bits, status), ERR_BAD_ARG, b"trunc_finish: y_dev overlaps csh_dev")
    expect(FX, fi(x + 16, rlow, x, bits, status), ERR_BAD_ARG, b"trunc_finish: y_dev overlaps x_dev", b"may coincide")
    expect(FX, fi(x, rlow, x, bits, status, ys=N + 2), ERR_BAD_ARG, b"trunc_finish: y_dev overlaps x_dev", b"may coincide")
    expect(FX, fi(rlow + 16, rlow, x, bits, status), ERR_BAD_ARG, b"trunc_finish: y_dev overlaps rlow_dev", b"may coincide")
    expect(FX, fi(out, rlow, x, bits, out + 3), ERR_BAD_ARG, b"trunc_finish: y_dev overlaps status_dev")
    expect(FX, fi(out, rlow, x, bits, x + rows * N * e - 1), ERR_BAD_ARG, b"trunc_finish: x_dev overlaps status_dev")
    expect(FX, fi(out, rlow, x, bits, rlow), ERR_BAD_ARG, b"trunc_finish: rlow_dev overlaps status_dev")
    expect(FX, fi(out, rlow, x, bits, bits + 5), ERR_BAD_ARG, b"trunc_finish: csh_dev overlaps status_dev")
    if not torch.cuda.is_available():
        reaches_the_device_check(FX, mk(x, rlow, x, bits))                               # in place
        reaches_the_device_check(FX, mk(x, rlow, x, bits, cs=N + 2, xs=N + 2))
        reaches_the_device_check(FX, fi(x, rlow, x, bits, status))                       # in place on x
        reaches_the_device_check(FX, fi(rlow, rlow, x, bits, status))                    # in place on rlow
        reaches_the_device_check(FX, fi(out, x, x, bits, status))                        # two inputs may share memory
        reaches_the_device_check(FX, co(out, bits))


@pytest.mark.parametrize("f", FIELDS)
def test_a_well_formed_call_needs_a_device(fx, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    top = fx.lib.scl_fx_max_bits(f)
    for B, k, shift in ((2, 2, 1), (top, top, top - 1), (top, 2, 1)):
        expect(FX, fx.lib.scl_fx_compose(*compose_args(f, B=B, row_stride=B * 8 + 1)), ERR_NO_DEVICE)
        expect(FX, fx.lib.scl_fx_trunc_mask(*mask_args(f, B=B, k=k, shift=shift, c_stride=11, x_stride=12)), ERR_NO_DEVICE)
        for m in (1, 64):
            expect(FX, fx.lib.scl_fx_trunc_finish(*finish_args(f, B=B, shift=shift, m=m, y_stride=11, rlow_stride=12)), ERR_NO_DEVICE)
    p = ptrs()
    p[4] += 3                                                                           # the status starts anywhere
    expect(FX, fx.lib.scl_fx_trunc_finish(*finish_args(f, N=1, p=p)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(fx):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # calls that end at a later check when the modulus is in order
    check_latch_rule(FX, [(fx.lib.scl_fx_compose, compose_args(O.MONT128, out_stride=7), b"out_stride", ERR_SIZE_MISMATCH),
                          (fx.lib.scl_fx_trunc_mask, mask_args(O.MONT128, shift=0), b"shift == 0", ERR_BAD_ARG),
                          (fx.lib.scl_fx_trunc_finish, finish_args(O.MONT128, y_stride=7), b"y_stride", ERR_SIZE_MISMATCH)])


def test_the_last_error_is_per_thread(fx):
    lib = fx.lib
    check_last_error_per_thread(FX, (lib.scl_fx_trunc_finish, finish_args(O.M61, rlow_stride=7)), b"trunc_finish: rlow_stride < N",
                                (lib.scl_fx_trunc_mask, mask_args(O.M61, shift=0)), b"trunc_mask: shift == 0")
