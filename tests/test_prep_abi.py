"""CPU-side checks of the preprocessing extension's boundary: libscl_hip_prep.so exports exactly the prototypes of
include/scl_hip_prep.h, the binding takes its ctypes prototypes from that header, scl_prep_triple_blocks is the header's formula,
and every error the header promises is decided on the host, before a launch -- so each is reachable here, without a device, with
pointers that are never dereferenced."""
import ctypes as C

import pytest

import oracle_lib as O
from abi_support import (ERR_BAD_ARG, ERR_NO_DEVICE, ERR_SIZE_MISMATCH, OK, PREP, check_engine_is_only_dependency, check_exports, check_latch_rule,
                         declared_symbols, expect)

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
SYMBOLS = ["scl_prep_abi_version", "scl_prep_last_error", "scl_prep_triple_blocks", "scl_prep_triples_additive_prg",
           "scl_prep_triples_scratch_bytes", "scl_prep_triples_shamir_prg"]
BASE = 1 << 24      # a 16-byte aligned address that is never read: every case below ends before a launch
SEED = b"prep abi"
ADDITIVE, SHAMIR, TWO_PASS = 0, 1, 1


@pytest.fixture(scope="module")
def prep():
    import scl_amd.prep
    return scl_amd.prep


def t_max(f):
    """the largest threshold the dealer takes: beyond it the engine's share call synchronises the stream"""
    return 16 if O.LIMBS[f] == 4 else 48


def ptrs(k, step=1 << 20):
    return [BASE + i * step for i in range(k)]


def additive_args(f, N=8, n=3, stride=None, p=None, counter0=0):
    a, b, c = p or ptrs(3)
    return (f, a, b, c, N if stride is None else stride, N, n, SEED, len(SEED), counter0, None)


def shamir_args(f, N=8, t=1, n=4, stride=None, p=None, counter0=0, scratch=BASE + (8 << 20), flags=0):
    a, b, c = p or ptrs(3)
    return (f, a, b, c, N if stride is None else stride, N, t, n, SEED, len(SEED), counter0, scratch, flags, None)


def test_the_library_exports_the_header_and_nothing_else(prep):
    check_exports(PREP, SYMBOLS)


def test_the_engine_is_its_only_project_dependency():
    """linked against libscl_hip.so, found beside it ($ORIGIN), and not against the other extension libraries; every undefined
    scl_* symbol is a prototype of scl_hip.h"""
    check_engine_is_only_dependency(PREP)


def test_version_and_prototypes_come_from_the_header(prep):
    assert prep.lib.scl_prep_abi_version() == 1
    assert prep._NPROTO == len(declared_symbols(PREP)) == 6
    for name in declared_symbols(PREP):
        assert getattr(prep.lib, name).argtypes is not None, name
    assert prep.lib.scl_prep_last_error.restype is C.c_char_p
    assert prep.lib.scl_prep_triple_blocks.restype is C.c_size_t and prep.lib.scl_prep_triples_scratch_bytes.restype is C.c_size_t
    a, s = prep.lib.scl_prep_triples_additive_prg.argtypes, prep.lib.scl_prep_triples_shamir_prg.argtypes
    assert len(a) == 11 and a[0] is C.c_int and [a[i] for i in (1, 2, 3, 7, 10)] == [C.c_void_p] * 5 and a[9] is C.c_uint64
    assert len(s) == 14 and [s[i] for i in (4, 5, 6, 7, 9)] == [C.c_size_t] * 5 and s[10] is C.c_uint64 and s[12] is C.c_uint and s[11] is C.c_void_p
    with pytest.raises((C.ArgumentError, TypeError)):
        prep.lib.scl_prep_triples_additive_prg(0)                          # too few arguments
    with pytest.raises((C.ArgumentError, TypeError)):
        prep.lib.scl_prep_triples_shamir_prg(*shamir_args("m61"))          # not an int


def test_the_engine_is_untouched_by_the_import(prep):
    """scl_amd exports what it exported: the extension is a module of its own"""
    import scl_amd
    assert not hasattr(scl_amd, "deal_triples_additive") and not hasattr(scl_amd, "deal_triples_shamir")
    assert scl_amd.lib.scl_hip_abi_version() == 2


def test_triple_blocks_is_the_headers_formula(prep):
    """B = (2 + 3 (n-1)) BPE and 2 BPE + 3 ceil((t+1) E / 16) on a grid; 0 for what the deal calls refuse"""
    lib = prep.lib
    for f in FIELDS + RINGS:
        E = O.byte_size(f)
        bpe = (E + 15) // 16
        for n in (2, 3, 5, 16, 1000):
            assert lib.scl_prep_triple_blocks(f, ADDITIVE, n, 0) == (2 + 3 * (n - 1)) * bpe == lib.scl_prep_triple_blocks(f, ADDITIVE, n, 99)
        for n in (0, 1):
            assert lib.scl_prep_triple_blocks(f, ADDITIVE, n, 0) == 0
        for t in (0, 1, 2, 3, 7, 8, 9, 16, 17, 42, 48, 49, 1000):
            ok = f in FIELDS and t <= t_max(f)                                           # Shamir shares over fields only
            want = 2 * bpe + 3 * (((t + 1) * E + 15) // 16) if ok else 0
            assert lib.scl_prep_triple_blocks(f, SHAMIR, 20, t) == want, (f, t)
        assert lib.scl_prep_triple_blocks(f, SHAMIR, 0, 1) == 0 and lib.scl_prep_triple_blocks(f, 2, 3, 1) == 0
    for tag in (-1, 6, 0x100, 0x100 + 129):
        assert lib.scl_prep_triple_blocks(tag, ADDITIVE, 3, 0) == 0 and lib.scl_prep_triple_blocks(tag, SHAMIR, 4, 1) == 0
    assert prep.triple_blocks(O.M61, prep.ADDITIVE, 2) == 5 and prep.triple_blocks(O.M61, prep.SHAMIR, 10, 3) == 8
    assert prep.triple_blocks(O.SECP256K1_SCALAR, prep.SHAMIR, 10, 3) == 4 + 3 * 8
    import scl_amd
    with pytest.raises(scl_amd.SclError):
        prep.triple_blocks(O.Z2K(64), prep.SHAMIR, 4, 1)


def test_scratch_bytes_names_the_two_pass_cases(prep):
    """0 where the fused kernel deals the case (Mersenne61, Mersenne127, GF(2^128) at t <= 7 without flags bit 0), else
    (3 + 3t) N elements"""
    lib = prep.lib
    for f in FIELDS:
        esz = 8 * O.LIMBS[f]
        for t in (0, 1, 3, 7, 8, 9):
            fused = f in (O.M61, O.M127, O.GF2_128) and t <= 7
            assert lib.scl_prep_triples_scratch_bytes(f, 257, 20, t, 0) == (0 if fused else (3 + 3 * t) * 257 * esz), (f, t)
            assert lib.scl_prep_triples_scratch_bytes(f, 257, 20, t, TWO_PASS) == (3 + 3 * t) * 257 * esz
            assert lib.scl_prep_triples_scratch_bytes(f, 257, 20, t, 2) == 0         # an undefined flags bit
        assert lib.scl_prep_triples_scratch_bytes(f, 257, 0, 1, TWO_PASS) == 0
        assert lib.scl_prep_triples_scratch_bytes(f, 257, 20, t_max(f), 0) == (3 + 3 * t_max(f)) * 257 * esz
        assert lib.scl_prep_triples_scratch_bytes(f, 257, 20, t_max(f) + 1, 0) == 0      # a refused threshold
    assert lib.scl_prep_triples_scratch_bytes(O.Z2K(64), 257, 4, 1, TWO_PASS) == 0


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_nothing_to_do_is_ok_at_once(prep, f):
    """N == 0: SCL_OK before any argument is looked at"""
    assert prep.lib.scl_prep_triples_additive_prg(f, None, None, None, 0, 0, 0, None, 0, 0, None) == OK
    assert prep.lib.scl_prep_triples_shamir_prg(f, None, None, None, 0, 0, 0, 0, None, 0, 0, None, 7, None) == OK


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_null_and_misaligned_pointers(prep, f):
    lib = prep.lib
    off = 4 if O.LIMBS[f] == 1 else 8          # one limb: 8-byte alignment; wider: 16
    for k in range(3):
        p = ptrs(3)
        p[k] = None
        expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, p=p)), ERR_BAD_ARG, b"NULL")
        if f in FIELDS:
            expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, p=p)), ERR_BAD_ARG, b"NULL")
        p = ptrs(3)
        p[k] += off
        expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, p=p)), ERR_BAD_ARG, b"aligned")
        if f in FIELDS:
            expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, p=p)), ERR_BAD_ARG, b"aligned")


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_strides_parties_and_flags(prep, f):
    lib = prep.lib
    expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, N=8, stride=7)), ERR_SIZE_MISMATCH, b"stride < N")
    for n in (0, 1):
        expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, n=n)), ERR_BAD_ARG, b"n must be >= 2")
    if f in FIELDS:
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=8, stride=7)), ERR_SIZE_MISMATCH, b"stride < N")
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, n=0)), ERR_BAD_ARG, b"n must be")
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, n=65536)), ERR_BAD_ARG, b"n must be")
        # a threshold at which the engine's share call would synchronise the stream is refused; the last one below it is not
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, t=t_max(f) + 1, n=200)), ERR_BAD_ARG, b"threshold t at most %d" % t_max(f))
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, t=65535, n=200)), ERR_BAD_ARG, b"threshold")
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, t=t_max(f), n=200, scratch=None)), ERR_BAD_ARG, b"scratch")
        for flags in (2, 3, 0x80000000):
            expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, flags=flags)), ERR_BAD_ARG, b"flags")
    else:       # Shamir shares over fields only, as scl_hip_shamir_share_prg
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f)), ERR_BAD_ARG, b"unknown field tag")


@pytest.mark.parametrize("tag", [-1, 6, 0x100, 0x100 + 129, 0x7fffffff])
def test_unknown_tags(prep, tag):
    expect(PREP, prep.lib.scl_prep_triples_additive_prg(*additive_args(tag)), ERR_BAD_ARG, b"unknown field tag")
    expect(PREP, prep.lib.scl_prep_triples_shamir_prg(*shamir_args(tag)), ERR_BAD_ARG, b"unknown field tag")


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR])
def test_overlaps(prep, f):
    """a, b and c may not overlap one another, nor the scratch any of them"""
    lib, esz, N, n = prep.lib, 8 * O.LIMBS[f], 8, 3
    for i, j in ((0, 1), (0, 2), (1, 2), (1, 0), (2, 0), (2, 1)):
        p = ptrs(3)
        p[j] = p[i] + ((n - 1) * N + N - 1) * esz        # starts at the last element of the other matrix
        expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, N=N, n=n, p=p)), ERR_BAD_ARG, b"overlap")
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=N, n=n, p=p)), ERR_BAD_ARG, b"overlap")
        p[j] = p[i] + n * N * esz                         # back to back is in order: the check AFTER the overlap check is met
        need = lib.scl_prep_triples_scratch_bytes(f, N, n, 9, 0)
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=N, n=n, t=9, p=p, scratch=None)), ERR_BAD_ARG, str(need).encode())
        expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, N=N, n=n, p=p, counter0=2 ** 64 - 8)), ERR_BAD_ARG, b"wraps")
    for k in range(3):
        p = ptrs(3)
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=N, n=n, t=9, p=p, scratch=p[k] + ((n * N - 1) * esz & ~15))), ERR_BAD_ARG,
               b"scratch overlaps")
        need = lib.scl_prep_triples_scratch_bytes(f, N, n, 9, 0)
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=N, n=n, t=9, p=p, scratch=p[k] - need + 16)), ERR_BAD_ARG,
               b"scratch overlaps")


def test_a_two_pass_case_without_scratch_names_the_size_it_needs(prep):
    lib = prep.lib
    cases = [(O.SECP256K1_SCALAR, 1, 0), (O.MONT128, 3, 0), (O.M61, 9, 0), (O.M61, 3, TWO_PASS), (O.GF2_128, 8, 0), (O.M127, 7, TWO_PASS)]
    for f, t, flags in cases:
        need = lib.scl_prep_triples_scratch_bytes(f, 257, 20, t, flags)
        assert need == (3 + 3 * t) * 257 * 8 * O.LIMBS[f]
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=257, t=t, n=20, scratch=None, flags=flags)), ERR_BAD_ARG,
               str(need).encode())
        assert b"scratch" in lib.scl_prep_last_error()
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=257, t=t, n=20, scratch=BASE + (8 << 20) + 8, flags=flags)), ERR_BAD_ARG,
               b"aligned")


def test_a_block_range_that_wraps_the_counter_is_refused(prep):
    lib = prep.lib
    expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(O.M61, N=8, n=3, counter0=2 ** 64 - 8)), ERR_BAD_ARG, b"wraps")
    expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(O.M61, N=8, counter0=2 ** 64 - 8)), ERR_BAD_ARG, b"wraps")


@pytest.mark.parametrize("f", FIELDS + RINGS)
def test_a_well_formed_call_needs_a_device(prep, f):
    """with everything in order the next thing the library asks for is a device.  The rule can only be exercised where there is
    no device: on a machine with a GPU these never-mapped addresses would reach a kernel, so the case skips itself there (decided
    before any work) and SCL_ERR_NO_DEVICE is covered by the run without a GPU alone."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: these addresses must not reach a kernel")
    lib = prep.lib
    expect(PREP, lib.scl_prep_triples_additive_prg(*additive_args(f, N=8, n=3, stride=11, counter0=2 ** 32 - 5)), ERR_NO_DEVICE)
    if f in FIELDS:
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=8, t=3, n=10, stride=11)), ERR_NO_DEVICE)
        expect(PREP, lib.scl_prep_triples_shamir_prg(*shamir_args(f, N=8, t=9, n=20, stride=8, flags=TWO_PASS)), ERR_NO_DEVICE)


def test_mont128_honours_the_latch_rule(prep):
    """scl_hip_mont128_set_prime's rule reaches the extension: a worker whose latched default went stale is refused (the engine's
    own check and message) until it re-latches; the main thread, which set its own modulus, is not disturbed"""
    # calls that end at a later check when the modulus is in order
    check_latch_rule(PREP, [(prep.lib.scl_prep_triples_additive_prg, additive_args(O.MONT128, n=1), b"n must be >= 2", ERR_BAD_ARG),
                            (prep.lib.scl_prep_triples_shamir_prg, shamir_args(O.MONT128, flags=2), b"flags", ERR_BAD_ARG)])
