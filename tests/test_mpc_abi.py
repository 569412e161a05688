"""CPU-side checks of the protocol extension's boundary: libscl_hip_mpc.so exports exactly the prototypes of
include/scl_hip_mpc.h, the binding takes its ctypes prototypes from that header, and every error the header promises is decided
on the host, before a launch -- so each is reachable here, without a device, with pointers that are never dereferenced."""
import ctypes as C

import pytest

import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, MPC, check_engine_is_only_dependency, check_exports, check_latch_rule,
                         declared_symbols, expect)

TAGS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD, O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
SYMBOLS = ["scl_mpc_abi_version", "scl_mpc_beaver_finish", "scl_mpc_beaver_mask", "scl_mpc_last_error"]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch


@pytest.fixture(scope="module")
def mpc():
    import scl_amd.mpc
    return scl_amd.mpc


def ptrs(k, step=1 << 20):
    return [BASE + i * step for i in range(k)]


def mask_args(f, N=8, rows=1, de_stride=None, op_stride=None, p=None):
    de, x, y, a, b = p or ptrs(5)
    return (f, de, N if de_stride is None else de_stride, x, y, a, b, N if op_stride is None else op_stride, rows, N, None)


def finish_args(f, N=8, rows=1, ed_rows=0, z_stride=None, op_stride=None, p=None):
    z, e, d, a, b, c = p or ptrs(6)
    return (f, z, N if z_stride is None else z_stride, e, d, a, b, c, N if op_stride is None else op_stride, rows, ed_rows, N, None)


def test_the_library_exports_the_header_and_nothing_else(mpc):
    check_exports(MPC, SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and not against the other extension libraries; every undefined
    scl_* symbol is a prototype of scl_hip.h"""
    check_engine_is_only_dependency(MPC)


def test_version_and_prototypes_come_from_the_header(mpc):
    assert mpc.lib.scl_mpc_abi_version() == 1
    assert mpc._NPROTO == len(declared_symbols(MPC))
    for name in declared_symbols(MPC):
        assert getattr(mpc.lib, name).argtypes is not None, name
    assert mpc.lib.scl_mpc_last_error.restype is C.c_char_p
    m, f = mpc.lib.scl_mpc_beaver_mask.argtypes, mpc.lib.scl_mpc_beaver_finish.argtypes
    assert len(m) == 11 and m[0] is C.c_int and m[2] is C.c_size_t and m[1] is C.c_void_p and m[10] is C.c_void_p
    assert len(f) == 13 and [f[i] for i in (2, 8, 9, 10, 11)] == [C.c_size_t] * 5 and f[3] is C.c_void_p
    with pytest.raises((C.ArgumentError, TypeError)):
        mpc.lib.scl_mpc_beaver_mask(0)                    # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        mpc.lib.scl_mpc_beaver_finish(*finish_args("m61"))  # not an int


def test_the_engine_is_untouched_by_the_import(mpc):
    """scl_amd exports what it exported: the extension is a module of its own"""
    import scl_amd
    assert not hasattr(scl_amd, "beaver_mask") and not hasattr(scl_amd, "beaver_finish")
    assert scl_amd.lib.scl_hip_abi_version() == 2


@pytest.mark.parametrize("f", TAGS)
def test_nothing_to_do_is_ok_at_once(mpc, f):
    """N == 0 or rows == 0: SCL_OK before any pointer is looked at"""
    lib = mpc.lib
    assert lib.scl_mpc_beaver_mask(f, None, 0, None, None, None, None, 0, 1, 0, None) == OK
    assert lib.scl_mpc_beaver_mask(f, None, 0, None, None, None, None, 0, 0, 5, None) == OK
    assert lib.scl_mpc_beaver_finish(f, None, 0, None, None, None, None, None, 0, 1, 0, 0, None) == OK
    assert lib.scl_mpc_beaver_finish(f, None, 0, None, None, None, None, None, 0, 0, 0, 5, None) == OK


@pytest.mark.parametrize("f", TAGS)
def test_null_and_misaligned_pointers(mpc, f):
    lib = mpc.lib
    off = 4 if O.LIMBS[f] == 1 else 8          # one limb: 8-byte alignment; wider: 16
    for k in range(5):
        p = ptrs(5)
        p[k] = None
        expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, p=p)), ERR_BAD_ARG)
        assert b"NULL" in lib.scl_mpc_last_error()
        p = ptrs(5)
        p[k] += off
        expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, p=p)), ERR_BAD_ARG)
        assert b"aligned" in lib.scl_mpc_last_error()
    for k in range(6):
        p = ptrs(6)
        p[k] = None
        expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, p=p)), ERR_BAD_ARG)
        assert b"NULL" in lib.scl_mpc_last_error()
        p = ptrs(6)
        p[k] += off
        expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, p=p)), ERR_BAD_ARG)
        assert b"aligned" in lib.scl_mpc_last_error()


@pytest.mark.parametrize("f", TAGS)
def test_strides_and_ed_rows(mpc, f):
    lib = mpc.lib
    expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, N=8, rows=3, de_stride=7)), ERR_SIZE_MISMATCH)
    expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, N=8, rows=3, op_stride=7)), ERR_SIZE_MISMATCH)
    expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, N=8, rows=1, de_stride=0)), ERR_SIZE_MISMATCH)
    expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=8, rows=3, z_stride=7)), ERR_SIZE_MISMATCH)
    expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=8, rows=3, op_stride=7)), ERR_SIZE_MISMATCH)
    expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=8, rows=3, ed_rows=4)), ERR_BAD_ARG)
    assert b"ed_rows" in lib.scl_mpc_last_error()


@pytest.mark.parametrize("tag", [-1, 6, 0x100, 0x100 + 129, 0x7fffffff])
def test_unknown_tags(mpc, tag):
    expect(MPC, mpc.lib.scl_mpc_beaver_mask(*mask_args(tag)), ERR_BAD_ARG)
    assert b"unknown field tag" in mpc.lib.scl_mpc_last_error()
    expect(MPC, mpc.lib.scl_mpc_beaver_finish(*finish_args(tag)), ERR_BAD_ARG)
    assert b"unknown field tag" in mpc.lib.scl_mpc_last_error()


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps(mpc, f):
    """mask: de may overlap no operand.  finish: z may BE a, b or c at the operands' stride; any other overlap is refused"""
    lib, esz, N, rows = mpc.lib, 8 * O.LIMBS[f], 8, 3
    for k in range(1, 5):
        p = ptrs(5)
        p[k] = p[0] + (2 * rows - 1) * N * esz          # the operand starts inside the last row of de
        expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, N=N, rows=rows, p=p)), ERR_BAD_ARG)
        assert b"overlaps" in lib.scl_mpc_last_error()
    for k in (3, 4, 5):
        p = ptrs(6)
        p[0] = p[k] + esz                                # one element into a, b or c
        expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=N, rows=rows, p=p)), ERR_BAD_ARG)
        p = ptrs(6)
        p[0] = p[k]                                      # exactly a, b or c, but at another stride
        expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=N, rows=rows, z_stride=N + 2, op_stride=N, p=p)), ERR_BAD_ARG)
    for k in (1, 2):
        p = ptrs(6)
        p[k] = p[0] + (rows - 1) * N * esz               # e or d inside the last row of z
        expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=N, rows=rows, p=p)), ERR_BAD_ARG)
        assert b"e or d" in lib.scl_mpc_last_error()


@pytest.mark.parametrize("f", TAGS)
def test_a_well_formed_call_needs_a_device(mpc, f):
    """with everything in order the next thing the library asks for is a device; in place (z == a) is in order.  The rule can
    only be exercised where there is no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so
    the case skips itself there (decided before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    lib = mpc.lib
    expect(MPC, lib.scl_mpc_beaver_mask(*mask_args(f, N=8, rows=3, de_stride=9, op_stride=11)), ERR_NO_DEVICE)
    expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=8, rows=3, ed_rows=3, z_stride=9, op_stride=11)), ERR_NO_DEVICE)
    p = ptrs(6)
    p[0] = p[3]
    expect(MPC, lib.scl_mpc_beaver_finish(*finish_args(f, N=8, rows=3, ed_rows=1, z_stride=10, op_stride=10, p=p)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(mpc):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # a call that ends at ed_rows > rows when the modulus is in order
    check_latch_rule(MPC, [(mpc.lib.scl_mpc_beaver_finish, finish_args(O.MONT128, rows=1, ed_rows=2), b"ed_rows", ERR_BAD_ARG)])
