"""Batch verification, the host half: the Python model (tests/port_models.py) of the random linear combination out[r][j] = sum_s rho_j[s] x[r][s] (y[r][s])
built from pieces of the CPU oracle only (Port.vector_random for the coin, Port.ew, Port.dot), pinned entry by entry to what the
REFERENCE produced (tests/golden/golden_vf.json); the same model over the fields the reference lacks on algebraic identities; and
the stand-alone check of the per-element forms of detail/vf.hpp against one reduced operation at a time
(tests/cxx/vf_host_check.cc), plain and under the address and undefined-behaviour sanitizers.  The model also checks the kernels
in tests/test_gpu_vf.py.  Everything is exact.

The coin (include/scl_hip_vf.h): rho_j is the j-th consecutive Vector::random(N) of a util::PRG that stands at block counter0.
A Vector::random(n) reads n * byteSize consecutive bytes of the stream from a block boundary on, so rho_j is FF::read over the
blocks [counter0 + j B, counter0 + (j + 1) B), B = ceil(N * byteSize / 16): Port.prg_blocks and Port.from_bytes, which the tests
below hold against Port.vector_random at counter0 = 0 and against the reference's coins at the fixture's counter0."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from cxx_support import SANITIZE, host_check, mirror_binary, mirror_host_output, needed
from port_models import TAGS3 as TAGS
from port_models import coin_blocks, degree_entry, from_hex, golden, golden_path, hex_rows, model_coins, model_combine, product_entry

GOLDEN = golden_path("vf")
FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
MONT_P = (1 << 128) - 159


def lies_on(port, f, shares, d):
    """shares [n][L] at the nodes 1..n: do shares d+1.. lie on the polynomial through the first d+1?  -> (bool, its value at 0)"""
    L, n = O.LIMBS[f], shares.shape[0]
    nodes = np.stack([port.from_int(f, i + 1) for i in range(d + 1)])
    at = lambda x: port.shamir_recover_at(f, shares[None, :d + 1], nodes, port.from_int(f, x))[0]
    return all(np.array_equal(at(i + 1), shares[i]) for i in range(d + 1, n)), at(0)


def model_product_check(port, f, a, b, c, rho):
    """every party's sum rho a b - sum rho c -> [n][L]"""
    return port.ew(f, O.SUB, model_combine(port, f, a, rho, b)[:, 0], model_combine(port, f, c, rho)[:, 0])


@pytest.fixture(scope="module")
def port():
    p = O.Port()
    p.mont128_set_prime(MONT_P)
    return p


def test_the_fixture_has_the_documented_shape():
    g = golden("vf")
    assert [e["field"] for e in g["combine"]] == [e["field"] for e in g["degree"]] == [e["field"] for e in g["product"]] == list(TAGS)
    for e in g["combine"]:
        assert [r["N"] for r in e["runs"]] == [1, 2, 5] and len(e["x"]) == len(e["y"]) == 3
        assert all(r["counter0"] == coin_blocks(TAGS[e["field"]], 3) > 0 for r in e["runs"])
    assert all((e["n"], e["t"], e["N"]) == (4, 1, 5) for e in g["degree"] + g["product"])
    assert os.path.getsize(GOLDEN) < 16 * 1024


def test_the_model_computes_the_fixtures_combinations(port):
    """every field, N = 1, 2, 5 (the first N columns of rows 5 apart), reps = 2 (reps = 1 is its first column), plain and product:
    the model's values are the reference's innerProd results; the inputs are the PRG's"""
    for e in golden("vf")["combine"]:
        f = TAGS[e["field"]]
        x, y = hex_rows(port, f, e["x"]), hex_rows(port, f, e["y"])
        assert np.array_equal(x, model_coins(port, f, b"vf inputs", 0, 5, 3)) and np.array_equal(y, model_coins(port, f, b"vf inputs y", 0, 5, 3))
        for r in e["runs"]:
            N, note = r["N"], (e["field"], r["N"])
            rho = model_coins(port, f, b"vf coin", r["counter0"], N, 2)
            assert np.array_equal(model_combine(port, f, x[:, :N], rho), hex_rows(port, f, r["plain"])), note
            assert np.array_equal(model_combine(port, f, x[:, :N], rho, y[:, :N]), hex_rows(port, f, r["product"])), note
            assert np.array_equal(model_combine(port, f, x[:, :N], rho[:1]), hex_rows(port, f, r["plain"])[:, :1]), note


def test_the_model_computes_the_fixtures_degree_check(port):
    """(4, 1), N = 5: every party's combined share is the reference's; the four lie on one line, which opens to sum rho secret;
    with one share of one column altered they do not"""
    for e in golden("vf")["degree"]:
        f = TAGS[e["field"]]
        rows, rho, secrets = degree_entry(port, f, e)
        combined = model_combine(port, f, rows, rho)[:, 0]
        assert np.array_equal(combined, from_hex(port, f, e["combined"])), e["field"]
        ok, opened = lies_on(port, f, combined, e["t"])
        assert ok and np.array_equal(opened, from_hex(port, f, [e["opened"]])[0]) and np.array_equal(opened, port.dot(f, rho[0], secrets))
        bad = rows.copy()
        bad[e["party"], e["column"]] = port.ew(f, O.ADD, bad[e["party"], e["column"]][None], port.from_int(f, 1)[None])[0]
        combined_bad = model_combine(port, f, bad, rho)[:, 0]
        assert np.array_equal(combined_bad, from_hex(port, f, e["combined_bad"])), e["field"]
        assert not lies_on(port, f, combined_bad, e["t"])[0]


def test_the_model_computes_the_fixtures_product_check(port):
    """(4, 1), N = 5 triples: every party's sum rho a b - sum rho c is the reference's and opens to 0 over all four shares; with
    delta on one column of c it opens to -rho delta, the reference's value, which is not 0"""
    for e in golden("vf")["product"]:
        f = TAGS[e["field"]]
        a, b, c, rho = product_entry(port, f, e)
        v = model_product_check(port, f, a, b, c, rho)
        assert np.array_equal(v, from_hex(port, f, e["v"])), e["field"]
        assert not port.shamir_recover(f, v[None]).any()
        delta = from_hex(port, f, [e["delta"]])
        c[:, e["column"]] = port.ew(f, O.ADD, np.ascontiguousarray(c[:, e["column"]]), np.repeat(delta, e["n"], axis=0))
        v_bad = model_product_check(port, f, a, b, c, rho)
        assert np.array_equal(v_bad, from_hex(port, f, e["v_bad"])), e["field"]
        off = port.shamir_recover(f, v_bad[None])[0]
        assert off.any() and np.array_equal(off, from_hex(port, f, [e["off"]])[0])
        zero = port.from_int(f, 0)[None]
        assert np.array_equal(off, port.ew(f, O.SUB, zero, port.ew(f, O.MUL, rho[0, e["column"]][None], delta))[0])


# ---- the model itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [O.MONT128, O.GF2_128, O.SECP256K1_FIELD], ids=["mont128", "gf128", "secp_field"])
def test_the_model_over_the_fields_without_a_fixture(port, f):
    """Mont128, GF(2^128) and the secp256k1 prime, algebraic identities only: the combination is linear in x; the product form
    is the plain form of x .* y; x == y gives sum rho x^2; a coin drawn at counter0 is the same coin drawn as separate vectors;
    repetition j of a call with more repetitions is the call with one at counter0 + j B; the empty sum is zero"""
    L, rows = O.LIMBS[f], 3
    for N in (1, 2, 5, 9):
        x1 = port.vector_random(f, b"vf-model-x1", rows * N).reshape(rows, N, L)
        x2 = port.vector_random(f, b"vf-model-x2", rows * N).reshape(rows, N, L)
        y = port.vector_random(f, b"vf-model-y", rows * N).reshape(rows, N, L)
        rho = model_coins(port, f, b"vf-model-coin", 7, N, 3)
        ew = lambda op, a, b: port.ew(f, op, np.ascontiguousarray(a).reshape(-1, L), np.ascontiguousarray(b).reshape(-1, L)).reshape(a.shape)
        both = model_combine(port, f, ew(O.ADD, x1, x2), rho)
        assert np.array_equal(both, ew(O.ADD, model_combine(port, f, x1, rho), model_combine(port, f, x2, rho))), N
        assert np.array_equal(model_combine(port, f, x1, rho, y), model_combine(port, f, ew(O.MUL, x1, y), rho)), N
        assert np.array_equal(model_combine(port, f, x1, rho, x1), model_combine(port, f, ew(O.MUL, x1, x1), rho)), N
        B = coin_blocks(f, N)
        for j in range(3):
            assert np.array_equal(rho[j], model_coins(port, f, b"vf-model-coin", 7 + j * B, N, 1)[0]), (N, j)
        assert np.array_equal(model_coins(port, f, b"vf-model-coin", 0, N, 1)[0], port.vector_random(f, b"vf-model-coin", N))
    assert not model_combine(port, f, np.zeros((rows, 0, L), dtype=np.uint64), np.zeros((2, 0, L), dtype=np.uint64)).any()


def test_coin_blocks_is_the_references_count():
    """ceil(N byteSize / 16): Mersenne61 two elements a block, the 16-byte fields one block an element, the 32-byte fields two"""
    for N in (0, 1, 2, 3, 257):
        assert coin_blocks(O.M61, N) == (N + 1) // 2 and coin_blocks(O.M127, N) == N and coin_blocks(O.SECP256K1_SCALAR, N) == 2 * N


# ---- the per-element forms -------------------------------------------------------------------------------------------------------
def test_the_per_element_forms_equal_the_reduced_operations(tmp_path):
    """every field struct: vf_take (two repetitions under one count), vf_combine_one, vf_take_partial and vf_sum_partials == mul
    and add one at a time, over 1, 2, 3, 63, 64, 65, 127, 128, 129 and 300 terms of (p-1)(p-1) and of (p-1)(p-1)(p-1), and
    uniform; the term count never passes the field's bound"""
    host_check(tmp_path, "vf_host_check.cc", "vf_host_check", ("-w", "-O2"))


def test_the_per_element_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    assert "runtime error" not in host_check(tmp_path, "vf_host_check.cc", "vf_host_check_san", ("-w",) + SANITIZE)


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_mirror_prints_the_fixture():
    """the mirror's Vector::random coins (ss::combineCoins on a util::PRG that drew and discarded three elements), ss::combine --
    held against vf_combine_one of detail/vf.hpp on the limbs --, ss::shamirSecretShare, ss::shamirRecoverD / P in the fixture's
    order: what it prints is the fixture (exit status 0: every open is what the harness of the reference required)"""
    r = mirror_host_output("vf")
    assert json.loads(r.stdout) == golden("vf")
    dynamic = needed(mirror_binary("vf"))
    assert "libscl_hip_vf.so" in dynamic and "libscl_hip.so" in dynamic
