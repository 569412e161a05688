"""CPU-side checks of the batch-verification extension's boundary: libscl_hip_vf.so exports exactly the prototypes of
include/scl_hip_vf.h, the binding takes its ctypes prototypes from that header, scl_vf_coin_blocks / scl_vf_scratch_bytes /
scl_vf_launch_shape agree with the header, and every error the header promises is decided on the host, before a launch -- so each
is reachable here, without a device, with pointers that are never dereferenced."""
import ctypes as C
import os
import re

import pytest

import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, PKG, VF, check_engine_is_only_dependency, check_exports,
                         check_last_error_per_thread, check_latch_rule, declared_symbols, expect, header, reaches_the_device_check)

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
STEP = 1 << 20
SYMBOLS = ["scl_vf_abi_version", "scl_vf_coin_blocks", "scl_vf_combine", "scl_vf_combine_prg", "scl_vf_last_error", "scl_vf_launch_shape",
           "scl_vf_scratch_bytes"]
PRG = 1
SEED = b"vf abi"


@pytest.fixture(scope="module")
def vf():
    import scl_amd.vf
    return scl_amd.vf


def esz(f):
    return 8 * O.LIMBS[f]


def ptrs():
    """out, x, y, rho, scratch: 1 MiB apart"""
    return [BASE + i * STEP for i in range(5)]


def need(vf, f, rows, reps, N, flags):
    return vf.lib.scl_vf_scratch_bytes(f, rows, reps, N, flags)


def prg_args(vf, f, N=8, rows=3, reps=2, p=None, out_stride=None, op_stride=None, counter0=5, scratch_bytes=None, seed=SEED):
    out, x, y, _, scratch = p or ptrs()
    sb = need(vf, f, rows, reps, N, PRG) if scratch_bytes is None else scratch_bytes
    return (f, out, reps if out_stride is None else out_stride, x, y, N if op_stride is None else op_stride, rows, N, reps, seed, len(seed or b""),
            counter0, scratch, sb, None)


def rows_args(vf, f, N=8, rows=3, reps=2, p=None, out_stride=None, op_stride=None, rho_stride=None, scratch_bytes=None):
    out, x, y, rho, scratch = p or ptrs()
    sb = need(vf, f, rows, reps, N, 0) if scratch_bytes is None else scratch_bytes
    return (f, out, reps if out_stride is None else out_stride, x, y, N if op_stride is None else op_stride, rho, N if rho_stride is None else rho_stride,
            rows, N, reps, scratch, sb, None)


def entry_points(vf):
    return [(vf.lib.scl_vf_combine_prg, prg_args, b"combine_prg"), (vf.lib.scl_vf_combine, rows_args, b"combine")]


def test_the_library_exports_the_header_and_nothing_else(vf):
    check_exports(VF, SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and not against the other extension libraries; every undefined
    scl_* symbol is a prototype of scl_hip.h"""
    check_engine_is_only_dependency(VF)


def test_version_and_prototypes_come_from_the_header(vf):
    """the binding compares the version before it looks up another symbol (scl_amd/vf.py through the one loader, scl_amd/_abi.py)
    and types every prototype"""
    assert vf.lib.scl_vf_abi_version() == 1 and re.search(r"#define\s+SCL_VF_ABI_VERSION\s+1\b", header(VF))
    pkg = os.path.join(PKG, "scl_amd")
    assert '_abi.declare(lib, _SO, "scl_hip_vf.h", "scl_vf_", "SCL_VF_ABI_VERSION"' in open(os.path.join(pkg, "vf.py")).read()
    src = open(os.path.join(pkg, "_abi.py")).read()
    assert src.index('getattr(lib, prefix + "abi_version")') < src.index("have = version()") < src.index("for m in re.finditer")
    assert vf._NPROTO == len(declared_symbols(VF)) == 7
    for name in declared_symbols(VF):
        assert getattr(vf.lib, name).argtypes is not None, name
    assert vf.lib.scl_vf_last_error.restype is C.c_char_p and vf.lib.scl_vf_launch_shape.restype is None
    assert vf.lib.scl_vf_coin_blocks.restype is C.c_size_t and vf.lib.scl_vf_scratch_bytes.restype is C.c_size_t
    p, r = vf.lib.scl_vf_combine_prg.argtypes, vf.lib.scl_vf_combine.argtypes
    assert len(p) == 15 and p[0] is C.c_int and [p[i] for i in (1, 3, 4, 9, 12, 14)] == [C.c_void_p] * 6 and p[11] is C.c_uint64
    assert [p[i] for i in (2, 5, 6, 7, 8, 10, 13)] == [C.c_size_t] * 7
    assert len(r) == 14 and r[0] is C.c_int and [r[i] for i in (1, 3, 4, 6, 11, 13)] == [C.c_void_p] * 6
    assert [r[i] for i in (2, 5, 7, 8, 9, 10, 12)] == [C.c_size_t] * 7
    assert list(vf.lib.scl_vf_scratch_bytes.argtypes) == [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint]
    with pytest.raises((C.ArgumentError, TypeError)):
        vf.lib.scl_vf_combine(0)                                    # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        vf.lib.scl_vf_combine(*rows_args(vf, O.M61)[:0] + ("m61",) + rows_args(vf, O.M61)[1:])      # not an int


@pytest.mark.parametrize("f", FIELDS)
def test_coin_blocks_is_ceil_of_the_bytes_over_sixteen(vf, f):
    bs = O.byte_size(f)
    for N in (0, 1, 2, 3, 63, 64, 65, 257, 1025, 10 ** 7 + 1):
        assert vf.lib.scl_vf_coin_blocks(f, N) == -(-N * bs // 16) == vf.coin_blocks(f, N), N


def test_the_queries_refuse_what_the_calls_refuse(vf):
    import scl_amd
    for tag in RINGS + [-1, 6, 0x7fffffff]:
        assert vf.lib.scl_vf_coin_blocks(tag, 8) == 0 and vf.lib.scl_vf_scratch_bytes(tag, 3, 1, 8, 0) == 0
        with pytest.raises(scl_amd.SclError):
            vf.coin_blocks(tag, 8)
        with pytest.raises(scl_amd.SclError):
            vf.launch_shape(tag, 1, True)
    for reps in (0, 5):
        assert vf.lib.scl_vf_scratch_bytes(O.M61, 3, reps, 8, 0) == 0
        with pytest.raises(scl_amd.SclError):
            vf.launch_shape(O.M61, reps, False)
    assert vf.lib.scl_vf_scratch_bytes(O.M61, 3, 1, 8, 2) == 0                                   # an unknown flag
    assert vf.lib.scl_vf_scratch_bytes(O.M61, 2 ** 62, 4, 2 ** 40, 0) == 0                       # overflows
    assert vf.lib.scl_vf_scratch_bytes(O.SECP256K1_SCALAR, 1, 4, 2 ** 61, PRG) == 0
    r = C.c_int(9)
    vf.lib.scl_vf_launch_shape(O.M61, 1, 0, C.byref(r), None, None, None)                        # NULL out-pointers are skipped
    assert r.value == 8


@pytest.mark.parametrize("f", FIELDS)
def test_scratch_bytes_is_monotone_and_covers_the_partials(vf, f):
    """monotone in rows, reps and N, with and without the coefficient rows; never below rows * reps elements (one workgroup's
    partial sums); the two-pass fields' PRG scratch exceeds the plain one by reps rows of N elements, the fused field's does not"""
    e = esz(f)
    grid = [(rows, reps, N) for rows in (1, 2, 3, 10, 11) for reps in (1, 2, 3, 4) for N in (0, 1, 2, 3, 257, 1025, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8)]
    for flags in (0, PRG):
        val = {k: need(vf, f, *k, flags) for k in grid}
        for (rows, reps, N), v in val.items():
            assert v >= rows * reps * e and v % 16 == 0, (rows, reps, N)
            for other, w in val.items():
                if all(a <= b for a, b in zip((rows, reps, N), other)):
                    assert v <= w, ((rows, reps, N), other, flags)
    fused = vf.launch_shape(f, 1, True)[3]
    assert fused == (f == O.M61)
    for rows, reps, N in ((10, 2, 1025), (1, 4, 3)):
        extra = need(vf, f, rows, reps, N, PRG) - need(vf, f, rows, reps, N, 0)
        if fused:
            assert extra <= 0
        else:
            assert reps * N * e <= extra <= reps * (N + 1) * e + 16
    assert not vf.launch_shape(f, 1, False)[3]


@pytest.mark.parametrize("f", FIELDS)
def test_the_launch_shape_agrees_with_the_header(vf, f):
    """R * reps accumulators a lane: eight for Mersenne61, four for the 16-byte fields, two for the 32-byte ones (a launch of
    those serves two repetitions); the scratch is rows * reps partials per workgroup along N, ceil(N / cols_per_trip) of them up
    to max_groups"""
    budget, per_launch = {1: (8, 4), 2: (4, 4), 4: (2, 2)}[O.LIMBS[f]]
    for prg in (False, True):
        for reps in (1, 2, 3, 4):
            R, cols, groups, fused = vf.launch_shape(f, reps, prg)
            lr = min(reps, per_launch)
            want = 5 if fused and reps <= 2 else max(1, budget // (4 if lr >= 3 else lr))      # fused: 128 registers a lane
            assert R == want and groups == (256 if fused else 1024), (prg, reps)
            for N in (1, cols, cols + 1, 3 * cols, cols * groups + 1):
                G = min(-(-N // cols), groups)
                base = need(vf, f, 7, reps, N, PRG if (prg and fused) else 0)
                assert base == (7 * reps * G * esz(f) + 15) // 16 * 16, (prg, reps, N)


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_no_rows_is_ok_at_once(vf, f):
    """rows == 0: SCL_OK before any argument is looked at"""
    lib = vf.lib
    assert lib.scl_vf_combine_prg(f, None, 0, None, None, 0, 0, 8, 9, None, 0, 0, None, 0, None) == OK
    assert lib.scl_vf_combine(f, None, 0, None, None, 0, None, 0, 0, 8, 9, None, 0, None) == OK


@pytest.mark.parametrize("tag", RINGS + [-1, 6, 0x100, 0x100 + 129, 0x7fffffff])
def test_rings_and_unknown_tags(vf, tag):
    """Shamir needs a field: a ring is refused like an unknown tag"""
    assert vf.lib.scl_vf_combine_prg(tag, *prg_args(vf, O.M61)[1:]) == ERR_BAD_ARG and b"unknown field tag" in vf.lib.scl_vf_last_error()
    assert vf.lib.scl_vf_combine(tag, *rows_args(vf, O.M61)[1:]) == ERR_BAD_ARG and b"unknown field tag" in vf.lib.scl_vf_last_error()


@pytest.mark.parametrize("f", FIELDS)
def test_repetitions_strides_scratch_and_the_counter(vf, f):
    lib = vf.lib
    for fn, args, who in entry_points(vf):
        for reps in (0, 5):
            expect(VF, fn(*args(vf, f, reps=reps, out_stride=8, scratch_bytes=1 << 20)), ERR_BAD_ARG, who, b"reps must be at least 1 and at most 4")
        expect(VF, fn(*args(vf, f, reps=3, out_stride=2)), ERR_SIZE_MISMATCH, who, b"out_stride < reps")
        expect(VF, fn(*args(vf, f, op_stride=7)), ERR_SIZE_MISMATCH, who, b"op_stride < N")
        n = need(vf, f, 3, 2, 8, PRG if fn is lib.scl_vf_combine_prg else 0)
        expect(VF, fn(*args(vf, f, scratch_bytes=n - 1)), ERR_BAD_ARG, who, b"scratch_bytes", str(n).encode(), b"scl_vf_scratch_bytes")
        expect(VF, fn(*args(vf, f, scratch_bytes=0)), ERR_BAD_ARG, who, b"scratch_bytes")
        expect(VF, fn(*args(vf, f, rows=2 ** 61, scratch_bytes=1 << 20)), ERR_BAD_ARG, who, b"overflows")
        expect(VF, fn(*args(vf, f, rows=2 ** 40, op_stride=2 ** 40, scratch_bytes=1 << 62)), ERR_BAD_ARG, who, b"overflows")
    expect(VF, lib.scl_vf_combine(*rows_args(vf, f, rho_stride=7)), ERR_SIZE_MISMATCH, b"combine: rho_stride < N")
    B = lib.scl_vf_coin_blocks(f, 8)
    for c0 in (2 ** 64 - 1, 2 ** 64 - 2 * B, 2 ** 64 - 2 * B - 64):
        expect(VF, lib.scl_vf_combine_prg(*prg_args(vf, f, counter0=c0)), ERR_BAD_ARG, b"combine_prg: counter0 + reps * B wraps the 64-bit counter")
    expect(VF, lib.scl_vf_combine_prg(*prg_args(vf, f, seed=None)[:9] + (None, 4) + prg_args(vf, f)[11:]), ERR_BAD_ARG, b"seed_host is NULL")


@pytest.mark.parametrize("f", FIELDS)
def test_null_and_misaligned_pointers(vf, f):
    """out, x, scratch (and rho) must be there; y may be NULL (the plain form) but not misaligned; each is named"""
    off = 4 if O.LIMBS[f] == 1 else 8          # one limb: 8-byte alignment; wider: 16
    names = [b"out_dev", b"x_dev", b"y_dev", b"rho_dev", b"scratch_dev"]
    for fn, args, who in entry_points(vf):
        uses = (0, 1, 2, 4) if who == b"combine_prg" else (0, 1, 2, 3, 4)
        for i in uses:
            p = ptrs()
            p[i] = None
            if i != 2:
                expect(VF, fn(*args(vf, f, p=p)), ERR_BAD_ARG, who, names[i], b"NULL")
            p = ptrs()
            p[i] += 8 if i == 4 else off
            expect(VF, fn(*args(vf, f, p=p)), ERR_BAD_ARG, who, names[i], b"aligned")


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps_and_the_allowed_aliases(vf, f):
    """out and scratch against every operand and each other: refused with both operands named; inputs on one another and
    back-to-back operands pass the checks -- which shows as the call going on to ask for a device, where there is none"""
    import torch
    no_gpu = not torch.cuda.is_available()
    lib, e, N, rows, reps = vf.lib, esz(f), 8, 3, 2
    out, x, y, rho, scratch = ptrs()
    for fn, args, who in entry_points(vf):
        ins = [(1, b"x_dev"), (2, b"y_dev")] + ([(3, b"rho_dev")] if who == b"combine" else [])
        for k, name in ins:
            for base, written in ((out, b"out_dev"), (scratch, b"scratch_dev")):
                for offset in (0, 16):
                    p = [out, x, y, rho, scratch]
                    p[k] = base + offset
                    expect(VF, fn(*args(vf, f, N=N, rows=rows, reps=reps, p=p)), ERR_BAD_ARG, who, written + b" overlaps " + name)
            p = [out, x, y, rho, scratch]
            p[k] = out - (((reps if k == 3 else rows) * N - 1) * e & ~15)                # the input's last element runs into out
            expect(VF, fn(*args(vf, f, N=N, rows=rows, reps=reps, p=p)), ERR_BAD_ARG, who, b"out_dev overlaps " + name)
        for offset in (0, 16, -16):
            expect(VF, fn(*args(vf, f, N=N, rows=rows, reps=reps, p=[out, x, y, rho, out + offset])), ERR_BAD_ARG, who, b"out_dev overlaps scratch_dev")
        # a pitched out covers its gaps
        expect(VF, fn(*args(vf, f, N=N, rows=rows, reps=reps, out_stride=64, p=[out, out + 16 * e, y, rho, scratch])), ERR_BAD_ARG, who, b"out_dev overlaps x_dev")
        if no_gpu:
            ok = lambda rc: reaches_the_device_check(VF, rc)
            ok(fn(*args(vf, f, N=N, rows=rows, reps=reps, p=[out, x, x, x, scratch])))              # inputs on one another: sum rho x^2
            ok(fn(*args(vf, f, N=N, rows=rows, reps=reps, p=[out, x, x + 16, x + 32, scratch])))
            ok(fn(*args(vf, f, N=N, rows=rows, reps=reps, p=[out, out + rows * reps * e, None, rho, scratch])))     # back to back, plain
            ok(fn(*args(vf, f, N=N, rows=rows, reps=reps, p=[out, x, y, rho, out + rows * reps * e])))


@pytest.mark.parametrize("f", FIELDS)
def test_a_well_formed_call_needs_a_device(vf, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    for fn, args, who in entry_points(vf):
        for reps in (1, 2, 3, 4):
            expect(VF, fn(*args(vf, f, reps=reps, out_stride=reps + 3, op_stride=11)), ERR_NO_DEVICE)
        expect(VF, fn(*args(vf, f, rows=1, N=1, reps=1)), ERR_NO_DEVICE)
        out, x, _, rho, scratch = ptrs()
        expect(VF, fn(*args(vf, f, p=[out, x, None, rho, scratch])), ERR_NO_DEVICE)                # the plain form
        expect(VF, fn(*args(vf, f, N=0, p=[out, None, None, None, scratch])), ERR_NO_DEVICE)       # the empty sum still writes zeros
    expect(VF, vf.lib.scl_vf_combine_prg(*prg_args(vf, f, counter0=2 ** 64 - 2 ** 20)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(vf):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # calls that end at a later check when the modulus is in order
    check_latch_rule(VF, [(vf.lib.scl_vf_combine_prg, prg_args(vf, O.MONT128, reps=0, out_stride=4), b"reps", ERR_BAD_ARG),
                          (vf.lib.scl_vf_combine, rows_args(vf, O.MONT128, reps=0, out_stride=4), b"reps", ERR_BAD_ARG)])


def test_the_last_error_is_per_thread(vf):
    lib = vf.lib
    check_last_error_per_thread(VF, (lib.scl_vf_combine, rows_args(vf, O.M61, op_stride=7)), b"combine: op_stride < N",
                                (lib.scl_vf_combine_prg, prg_args(vf, O.M61, reps=0, out_stride=1)), b"combine_prg: reps")
