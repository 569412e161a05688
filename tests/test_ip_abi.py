"""CPU-side checks of the inner-product extension's boundary: libscl_hip_ip.so exports exactly the prototypes of
include/scl_hip_ip.h, the binding takes its ctypes prototypes from that header, scl_ip_matmul_tile agrees with the header, and
every error the header promises is decided on the host, before a launch -- so each is reachable here, without a device, with
pointers that are never dereferenced."""
import ctypes as C
import re

import pytest

import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, IP, check_engine_is_only_dependency, check_exports,
                         check_last_error_per_thread, check_latch_rule, declared_symbols, expect, header, reaches_the_device_check)

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
SYMBOLS = ["scl_ip_abi_version", "scl_ip_dot_mask", "scl_ip_last_error", "scl_ip_matmul_mask", "scl_ip_matmul_tile"]
TILES = {1: (4, 4), 2: (2, 4), 4: (2, 2)}      # by limbs, as the header states them


@pytest.fixture(scope="module")
def ip():
    import scl_amd.ip
    return scl_amd.ip


def esz(f):
    return 8 * O.LIMBS[f]


def ptrs(k, step=1 << 20):
    return [BASE + i * step for i in range(k)]


def dot_args(f, N=8, rows=3, terms=4, p=None, d_stride=None, op_stride=None, xts=None, yts=None):
    d, x, y, r2 = p or ptrs(4)
    ops = N if op_stride is None else op_stride
    return (f, d, N if d_stride is None else d_stride, x, rows * ops if xts is None else xts, y, rows * ops if yts is None else yts, r2, ops,
            terms, rows, N, None)


def mat_args(f, N=8, a=2, K=3, b=2, batch=1, p=None, ds=None, xs=None, ys=None, rs=None, dbs=None, xbs=None, ybs=None, rbs=None):
    d, x, y, r2 = p or ptrs(4)
    ds, xs, ys, rs = [N if s is None else s for s in (ds, xs, ys, rs)]
    return (f, d, ds, a * b * ds if dbs is None else dbs, x, xs, a * K * xs if xbs is None else xbs, y, ys, K * b * ys if ybs is None else ybs,
            r2, rs, a * b * rs if rbs is None else rbs, a, K, b, batch, N, None)


def entry_points(ip):
    return [(ip.lib.scl_ip_dot_mask, dot_args), (ip.lib.scl_ip_matmul_mask, mat_args)]


def test_the_library_exports_the_header_and_nothing_else(ip):
    check_exports(IP, SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and not against the other extension libraries; every undefined
    scl_* symbol is a prototype of scl_hip.h"""
    check_engine_is_only_dependency(IP)


def test_version_and_prototypes_come_from_the_header(ip):
    assert ip.lib.scl_ip_abi_version() == 1 and re.search(r"#define\s+SCL_IP_ABI_VERSION\s+1\b", header(IP))
    assert ip._NPROTO == len(declared_symbols(IP)) == 5
    for name in declared_symbols(IP):
        assert getattr(ip.lib, name).argtypes is not None, name
    assert ip.lib.scl_ip_last_error.restype is C.c_char_p and ip.lib.scl_ip_matmul_tile.restype is None
    d, m, t = ip.lib.scl_ip_dot_mask.argtypes, ip.lib.scl_ip_matmul_mask.argtypes, ip.lib.scl_ip_matmul_tile.argtypes
    assert len(d) == 13 and d[0] is C.c_int and [d[i] for i in (1, 3, 5, 7, 12)] == [C.c_void_p] * 5
    assert [d[i] for i in (2, 4, 6, 8, 9, 10, 11)] == [C.c_size_t] * 7
    assert len(m) == 19 and m[0] is C.c_int and [m[i] for i in (1, 4, 7, 10, 18)] == [C.c_void_p] * 5
    assert [m[i] for i in (2, 3, 5, 6, 8, 9, 11, 12, 13, 14, 15, 16, 17)] == [C.c_size_t] * 13
    assert list(t) == [C.c_int, C.c_void_p, C.c_void_p]
    with pytest.raises((C.ArgumentError, TypeError)):
        ip.lib.scl_ip_dot_mask(0)                                   # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        ip.lib.scl_ip_matmul_mask(*mat_args("m61"))                 # not an int


def test_the_tile_query_agrees_with_the_header(ip):
    """4 x 4 for Mersenne61, 2 x 4 for the 16-byte fields, 2 x 2 for the 32-byte fields -- the header's sentence --; 0 x 0 for
    what the call refuses; a NULL out-pointer is skipped"""
    text = " ".join(header(IP).split())
    assert "4 x 4 for Mersenne61, 2 x 4 for the 16-byte fields, 2 x 2 for the 32-byte fields" in text
    assert "ceil(b/TL) a K + ceil(a/TI) K b + 2 a b" in text
    for f in FIELDS:
        assert ip.matmul_tile(f) == TILES[O.LIMBS[f]], f
    import scl_amd
    for tag in RINGS + [-1, 6, 0x7fffffff]:
        ti, tl = C.c_int(9), C.c_int(9)
        ip.lib.scl_ip_matmul_tile(tag, C.byref(ti), C.byref(tl))
        assert (ti.value, tl.value) == (0, 0)
        with pytest.raises(scl_amd.SclError):
            ip.matmul_tile(tag)
    tl = C.c_int(9)
    ip.lib.scl_ip_matmul_tile(O.M61, None, C.byref(tl))
    assert tl.value == 4


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_nothing_to_do_is_ok_at_once(ip, f):
    """N == 0, rows == 0, batch == 0: SCL_OK before any argument is looked at"""
    lib = ip.lib
    assert lib.scl_ip_dot_mask(f, None, 0, None, 0, None, 0, None, 0, 0, 3, 0, None) == OK
    assert lib.scl_ip_dot_mask(f, None, 0, None, 0, None, 0, None, 0, 0, 0, 8, None) == OK
    assert lib.scl_ip_matmul_mask(f, None, 0, 0, None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 3, 0, None) == OK
    assert lib.scl_ip_matmul_mask(f, None, 0, 0, None, 0, 0, None, 0, 0, None, 0, 0, 0, 0, 0, 0, 8, None) == OK


@pytest.mark.parametrize("tag", RINGS + [-1, 6, 0x100, 0x100 + 129, 0x7fffffff])
def test_rings_and_unknown_tags(ip, tag):
    """Shamir needs a field: a ring is refused like an unknown tag"""
    for fn, args in entry_points(ip):
        expect(IP, fn(*args(tag)), ERR_BAD_ARG, b"unknown field tag")


@pytest.mark.parametrize("f", FIELDS)
def test_null_and_misaligned_pointers(ip, f):
    """d, x and y must be there; r2 may be NULL (no addend) but not misaligned"""
    off = 4 if O.LIMBS[f] == 1 else 8          # one limb: 8-byte alignment; wider: 16
    for fn, args in entry_points(ip):
        for i in range(4):
            p = ptrs(4)
            p[i] = None
            if i < 3:
                expect(IP, fn(*args(f, p=p)), ERR_BAD_ARG, b"NULL")
            p = ptrs(4)
            p[i] += off
            expect(IP, fn(*args(f, p=p)), ERR_BAD_ARG, b"aligned")


@pytest.mark.parametrize("f", FIELDS)
def test_strides_terms_and_dimensions(ip, f):
    lib = ip.lib
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, terms=0)), ERR_BAD_ARG, b"terms")
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, d_stride=7)), ERR_SIZE_MISMATCH, b"d_stride < N")
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, op_stride=7)), ERR_SIZE_MISMATCH, b"op_stride < N")
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, terms=2 ** 40, xts=2 ** 40)), ERR_BAD_ARG, b"extent of x_dev overflows")
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, rows=2 ** 40, d_stride=2 ** 40)), ERR_BAD_ARG, b"extent of d_dev overflows")
    for kw, word in (("ds", b"d_stride < N"), ("xs", b"x_stride < N"), ("ys", b"y_stride < N"), ("rs", b"r2_stride < N")):
        expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, **{kw: 7})), ERR_SIZE_MISMATCH, word)
    for a, K, b in ((0, 3, 2), (2, 0, 2), (2, 3, 0), (65536, 3, 2), (2, 65536, 2), (2, 3, 65536)):
        expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, a=a, K=K, b=b)), ERR_BAD_ARG, b"at least 1 and at most 65535")
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, batch=3, dbs=2 * 2 * 8 - 1)), ERR_BAD_ARG, b"d_batch_stride", b"32 elements")
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, batch=2 ** 50, dbs=2 ** 20)), ERR_BAD_ARG, b"extent of d_dev overflows")
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, batch=2 ** 50, xbs=2 ** 20, dbs=32, p=[BASE, BASE + (1 << 62), BASE + (1 << 61), None])), ERR_BAD_ARG,
           b"overflows")


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps_and_the_allowed_aliases(ip, f):
    """every forbidden overlap is refused with both operands named; the allowed alias (d == r2, equal strides), inputs on one
    another and back-to-back operands pass the checks -- which shows as the call going on to ask for a device, where there is none"""
    import torch
    no_gpu = not torch.cuda.is_available()
    lib, e, N = ip.lib, esz(f), 8
    d, x, y, r2 = ptrs(4)
    rows, terms = 3, 4
    span = lambda count: ((count * N - 1) * e) & ~15      # the last aligned byte offset inside `count` dense rows
    # dot: d against x and y over ALL terms; d == r2 only exactly
    for k, name in ((1, b"x_dev"), (2, b"y_dev")):
        for off in (-span(terms * rows), span(rows), 0):      # the input's last term runs into d; the input starts in d's last row; exactly d
            p = [d, x, y, r2]
            p[k] = d + off
            expect(IP, lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=p)), ERR_BAD_ARG, b"d_dev overlaps", name)
    for delta in (span(rows), -span(rows), 32):
        expect(IP, lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, x, y, d + delta])), ERR_BAD_ARG, b"d_dev overlaps r2_dev",
               b"may coincide")
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, x, y, d], d_stride=N + 2)), ERR_BAD_ARG, b"d_dev overlaps r2_dev")
    # matmul: the same, over all batches
    a, K, b, batch = 2, 3, 2, 3
    for k, name, count in ((1, b"x_dev", batch * a * K), (2, b"y_dev", batch * K * b)):
        for off in (-span(count), span(batch * a * b), 0):
            p = [d, x, y, r2]
            p[k] = d + off
            expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=p)), ERR_BAD_ARG, b"d_dev overlaps", name)
    for delta in (span(batch * a * b), -span(batch * a * b), 32):
        expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, x, y, d + delta])), ERR_BAD_ARG, b"d_dev overlaps r2_dev", b"may coincide")
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, x, y, d], ds=N + 2, dbs=4 * (N + 2), rs=N, rbs=4 * (N + 2))), ERR_BAD_ARG,
           b"d_dev overlaps r2_dev")
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, x, y, d], dbs=4 * N + 2, rbs=4 * N + 4)), ERR_BAD_ARG, b"d_dev overlaps r2_dev")
    if no_gpu:
        ok = lambda rc: reaches_the_device_check(IP, rc)
        ok(lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, x, y, d])))                                      # d == r2
        ok(lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, x, y, d], d_stride=N + 2, op_stride=N + 2)))
        ok(lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, x, x, x])))                                      # inputs on one another
        ok(lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, x, y, r2], xts=0, yts=1)))                       # any term stride
        ok(lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, d + rows * N * e, y, None])))                    # back to back, no addend
        ok(lib.scl_ip_dot_mask(*dot_args(f, N=N, rows=rows, terms=terms, p=[d, d - terms * rows * N * e, y, r2])))
        ok(lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, x, y, d])))
        ok(lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, x, y, d], ds=N + 2, rs=N + 2)))
        ok(lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=1, p=[d, x, y, d], dbs=5, rbs=77)))                                   # batch == 1: batch strides ignored
        ok(lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, x, x, x], xbs=0, ybs=0)))
        ok(lib.scl_ip_matmul_mask(*mat_args(f, N=N, batch=batch, p=[d, d + batch * a * b * N * e, y, None])))


@pytest.mark.parametrize("f", FIELDS)
def test_a_well_formed_call_needs_a_device(ip, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    lib = ip.lib
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, d_stride=9, op_stride=11)), ERR_NO_DEVICE)
    expect(IP, lib.scl_ip_dot_mask(*dot_args(f, terms=1, rows=1)), ERR_NO_DEVICE)
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, a=5, K=7, b=3, batch=10, ds=9, xs=10, ys=11, rs=12)), ERR_NO_DEVICE)
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, a=1, K=7, b=1, batch=2)), ERR_NO_DEVICE)        # the inner-product route
    d, x, y, _ = ptrs(4)
    expect(IP, lib.scl_ip_matmul_mask(*mat_args(f, p=[d, x, y, None], rs=0)), ERR_NO_DEVICE)       # without r2 its stride means nothing


def test_mont128_honours_the_latch_rule(ip):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # calls that end at a later check when the modulus is in order
    check_latch_rule(IP, [(ip.lib.scl_ip_dot_mask, dot_args(O.MONT128, terms=0), b"terms", ERR_BAD_ARG),
                          (ip.lib.scl_ip_matmul_mask, mat_args(O.MONT128, K=0), b"at least 1", ERR_BAD_ARG)])


def test_the_last_error_is_per_thread(ip):
    lib = ip.lib
    check_last_error_per_thread(IP, (lib.scl_ip_dot_mask, dot_args(O.M61, terms=0)), b"dot_mask: terms",
                                (lib.scl_ip_matmul_mask, mat_args(O.M61, K=0)), b"matmul_mask")
