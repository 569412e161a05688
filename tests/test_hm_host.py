"""Honest-majority multiplication, the host half: the Python model (tests/port_models.py) of the double-sharing discipline and of the protocol, built from
pieces of the CPU oracle only (Port.prg_blocks, from_bytes, ew, shamir_share_coeffs, lagrange_basis, matmul), pinned entry by
entry to what the REFERENCE produced (tests/golden/golden_hm.json); scl_amd.hm.hyper_invertible against the reference's
Matrix::hyperInvertible; the C++ mirror's ss::doubleShare, Matrix::hyperInvertible and the per-element forms of detail/hm.hpp
(tests/cxx/test_hm_api.cc) on the same entries; and the stand-alone check of those forms against one reduced operation at a time
(tests/cxx/hm_host_check.cc), plain and under the address and undefined-behaviour sanitizers.  The model also checks the kernels
in tests/test_gpu_hm.py.  Everything is exact.

The discipline (include/scl_hip_hm.h): E = byteSize, BPE = ceil(E/16), Bs(d) = ceil((d+1) E / 16).  Double sharing s owns the
blocks [counter0 + s B, counter0 + (s+1) B), B = BPE + Bs(t) + Bs(2t): r, one Vector::random(t+1) draw, one Vector::random(2t+1)
draw; the first element of each draw is discarded."""
import itertools
import json

import numpy as np
import pytest

import oracle_lib as O
from cxx_support import SANITIZE, host_check, mirror_binary, mirror_host_output, needed
from port_models import TAGS, double_blocks, from_hex, golden, model_double, model_him, model_open, model_protocol
from port_models import hm_protocol_entry as protocol_entry

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]


@pytest.fixture(scope="module")
def port():
    p = O.Port()
    p.mont128_set_prime((1 << 128) - 159)
    return p


def test_the_model_deals_the_fixtures_double_sharings(port):
    """every run: five consecutive double sharings at (3,1), (4,1), (7,3), (10,3), (9,4), and the run after a three-block burn"""
    runs = golden("hm")["double"]
    assert len(runs) == 24 and {(e["n"], e["t"]) for e in runs} == {(3, 1), (4, 1), (7, 3), (10, 3), (9, 4)}
    assert sum(e["burn"] == 3 for e in runs) == 4
    for e in runs:
        f = TAGS[e["field"]]
        lo, hi, _ = model_double(port, f, e["seed"].encode(), e["burn"], len(e["sharings"]), e["t"], e["n"])
        for got, k in ((lo, "lo"), (hi, "hi")):
            want = np.stack([from_hex(port, f, s[k]) for s in e["sharings"]], axis=1)
            assert np.array_equal(got, want), (e["field"], e["n"], e["t"], e["burn"], k)


def test_the_worked_block_counts():
    assert double_blocks(O.M61, 3) == 1 + 2 + 4 == 7 and double_blocks(O.SECP256K1_SCALAR, 3) == 2 + 8 + 14 == 24


def test_the_model_runs_the_fixtures_protocol(port):
    """n dealers, the extraction at both degrees, mask, open, finish, recover: every intermediate is the fixture's, z = x y"""
    runs = golden("hm")["protocol"]
    assert [(e["field"], e["n"], e["t"]) for e in runs] == [("m61", 4, 1), ("m61", 10, 3), ("secp256k1_scalar", 4, 1)]
    for e in runs:
        f = TAGS[e["field"]]
        want, S = protocol_entry(port, f, e)
        got = model_protocol(port, f, e["n"], e["t"], S, [d["seed"].encode() for d in e["dealers"]], b"hm inputs")
        for k in want:
            assert np.array_equal(got[k], want[k]), (e["field"], e["n"], k)
        assert np.array_equal(got["z"], port.ew(f, O.MUL, got["x"], got["y"]))


@pytest.mark.parametrize("f", [O.MONT128, O.GF2_128], ids=["mont128", "gf128"])
def test_the_model_multiplies_over_the_fields_the_reference_lacks(port, f):
    """Mont128 and GF(2^128) have no fixture: both sharings of a double sharing recover r, extraction keeps that, z = x y"""
    for n, t in ((4, 1), (10, 3)):
        lo, hi, r = model_double(port, f, b"no fixture", 5, 7, t, n)
        assert np.array_equal(model_open(port, f, lo), r) and np.array_equal(model_open(port, f, hi), r)
        assert np.array_equal(model_open(port, f, lo[:t + 1]), r) and np.array_equal(model_open(port, f, hi[:2 * t + 1]), r)
        g = model_protocol(port, f, n, t, 2, [b"d%d" % i for i in range(n)], b"in")
        assert np.array_equal(model_open(port, f, g["R_lo"]), model_open(port, f, g["R_hi"]))
        assert np.array_equal(g["z"], port.ew(f, O.MUL, g["x"], g["y"]))
        assert np.array_equal(model_open(port, f, g["z_shares"][:t + 1]), g["z"])              # [z] is a degree-t sharing


# ---- the hyper-invertible matrix -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hm():
    import scl_amd
    import scl_amd.hm
    scl_amd.set_mont128_prime((1 << 128) - 159)
    return scl_amd.hm


def test_hyper_invertible_equals_the_references(hm, port):
    runs = golden("hm")["him"]
    assert [(e["m"], e["n"]) for e in runs] == [(1, 1), (3, 4), (4, 4), (7, 10)] * 4
    for e in runs:
        f = TAGS[e["field"]]
        want = from_hex(port, f, e["rows"]).reshape(e["m"], e["n"], -1)
        assert np.array_equal(hm.hyper_invertible(f, e["m"], e["n"]), want), (e["field"], e["m"], e["n"])
        assert np.array_equal(model_him(port, f, e["m"], e["n"]), want), (e["field"], e["m"], e["n"])


@pytest.mark.parametrize("f", [O.MONT128, O.GF2_128], ids=["mont128", "gf128"])
def test_hyper_invertible_over_the_fields_the_reference_lacks(hm, port, f):
    for m, n in ((1, 1), (3, 4), (7, 10)):
        assert np.array_equal(hm.hyper_invertible(f, m, n), model_him(port, f, m, n))
    pts = [20, 21, 22]
    assert np.array_equal(hm.hyper_invertible(f, 3, 4, points=pts), model_him(port, f, 3, 4, pts))
    assert np.array_equal(hm.element(f, 5), port.from_int(f, 5))
    if f != O.GF2_128:
        assert np.array_equal(hm.element(f, -5), port.ew(f, O.SUB, port.from_int(f, 0)[None], port.from_int(f, 5)[None])[0])


def _det(port, f, A):
    """determinant of a k x k matrix [k][k][L], k <= 3, by the Leibniz formula"""
    k = A.shape[0]
    total = port.from_int(f, 0)[None]
    for perm in itertools.permutations(range(k)):
        term = port.from_int(f, 1)[None]
        for i in range(k):
            term = port.ew(f, O.MUL, term, A[i, perm[i]][None])
        sign = sum(1 for i in range(k) for j in range(i) if perm[j] > perm[i]) % 2
        total = port.ew(f, O.SUB if sign else O.ADD, total, term)
    return total[0]


def test_gf128_hyper_invertible_every_small_square_submatrix_is_invertible(hm, port):
    """(7,10) over GF(2^128) at the default points 11..17: every square submatrix up to size 3 has a non-zero determinant"""
    f = O.GF2_128
    M = hm.hyper_invertible(f, 7, 10)
    count = 0
    for k in (1, 2, 3):
        for rows in itertools.combinations(range(7), k):
            for cols in itertools.combinations(range(10), k):
                assert _det(port, f, M[np.ix_(rows, cols)]).any(), (rows, cols)
                count += 1
    assert count == 7 * 10 + 21 * 45 + 35 * 120


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_mirror_prints_the_fixture():
    """ss::doubleShare, Matrix::hyperInvertible and the protocol through hm_mask_one / hm_mac_step / hm_finish_one on the fixture's
    seeds, burns and shapes print the fixture (exit status 0: every z = x y)"""
    r = mirror_host_output("hm")
    assert json.loads(r.stdout) == golden("hm")
    dynamic = needed(mirror_binary("hm"))
    assert "libscl_hip_hm.so" in dynamic and "libscl_hip.so" in dynamic


def test_the_mirror_under_the_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined: the same output, no report"""
    r = mirror_host_output("hm", "test_hm_api_san", SANITIZE)
    assert json.loads(r.stdout) == golden("hm")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_per_element_forms_equal_the_reduced_operations(tmp_path):
    """every field struct: hm_mask_one, hm_finish_one and the accumulation step == mul / add / sub one at a time, at the extreme
    operands, at 10^5 uniform tuples, and over 1, 3, 10, 64, 65 and 300 terms, uniform and all at p - 1"""
    host_check(tmp_path, "hm_host_check.cc", "hm_host_check", ("-w", "-O2"))


def test_the_per_element_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    assert "runtime error" not in host_check(tmp_path, "hm_host_check.cc", "hm_host_check_san", ("-w",) + SANITIZE)
