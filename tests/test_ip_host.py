"""Inner and matrix products of Shamir sharings at one opening, the host half: the Python model (tests/port_models.py) of the local step
[d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t built from pieces of the CPU oracle only (Port.ew; Port.dot and Port.matmul check it column
by column), pinned entry by entry to what the REFERENCE produced (tests/golden/golden_ip.json); the same model over the fields the
reference lacks against plain Python integers (GF(2^128): the shift-xor multiplier of the GMAC tests); the stand-alone check of the
per-element forms of detail/ip.hpp against one reduced operation at a time (tests/cxx/ip_host_check.cc), plain and under the
address and undefined-behaviour sanitizers; and the C++ mirror's host mode (tests/cxx/test_ip_api.cc) on the fixture.  The model
also checks the kernels in tests/test_gpu_ip.py.  Everything is exact.

The fixture's order (tests/golden/make_golden_ip.py): the inputs come off ONE util::PRG term after term -- x_k, y_k, the sharing of
x_k, the sharing of y_k -- which is model_inputs of tests/port_models.py; [R] is model_double on the seed "ip dealer"."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from cxx_support import SANITIZE, host_check, mirror_binary, mirror_host_output, needed
from extremes import gf_mul
from port_models import TAGS3 as TAGS
from port_models import (ew as _ew, golden, golden_path, inner_entry, matrix_entry, model_dot_mask, model_finish, model_matmul_mask,
                         model_open)

GOLDEN = golden_path("ip")
FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
MONT_P = (1 << 128) - 159


@pytest.fixture(scope="module")
def port():
    p = O.Port()
    p.mont128_set_prime(MONT_P)
    return p


def test_the_fixture_has_the_documented_shape():
    g = golden("ip")
    assert [(e["field"], e["n"], e["t"], e["K"]) for e in g["inner"]] == [(f, n, t, K) for f in TAGS for n, t in ((4, 1), (10, 3)) for K in (1, 3, 5)]
    assert [(e["field"], e["n"], e["t"], e["a"], e["K"], e["b"]) for e in g["matrix"]] == [(f, 4, 1, 2, 3, 2) for f in TAGS]
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_the_model_computes_the_fixtures_inner_products(port):
    """every entry: every party's d, the opened d, every party's z and the recovered z are the reference's; z is Port.dot of the
    secrets"""
    for e in golden("ip")["inner"]:
        f = TAGS[e["field"]]
        xs, ys, lo, hi, want = inner_entry(port, f, e)
        note = (e["field"], e["n"], e["K"])
        d_shares = model_dot_mask(port, f, xs, ys, hi)
        assert np.array_equal(d_shares, want["d_shares"]), note
        d = model_open(port, f, d_shares)
        assert np.array_equal(d, want["d"]), note
        z_shares = model_finish(port, f, d, lo)
        assert np.array_equal(z_shares, want["z_shares"]), note
        z = model_open(port, f, z_shares)
        assert np.array_equal(z, want["z"]) and np.array_equal(z[0], port.dot(f, want["x"], want["y"])), note
        assert np.array_equal(model_open(port, f, z_shares[:e["t"] + 1]), z), note          # [z] is a degree-t sharing


def test_the_model_computes_the_fixtures_matrix_products(port):
    """2 x 3 times 3 x 2 at (4,1): every intermediate is the reference's; Z is Port.matmul of the secrets"""
    for e in golden("ip")["matrix"]:
        f = TAGS[e["field"]]
        X, Y, lo, hi, want = matrix_entry(port, f, e)
        n, a, K, b, L = e["n"], e["a"], e["K"], e["b"], O.LIMBS[f]
        d_shares = model_matmul_mask(port, f, X, Y, hi)
        assert np.array_equal(d_shares, want["d_shares"]), e["field"]
        d = model_open(port, f, d_shares.reshape(n, a * b, L))
        assert np.array_equal(d, want["d"]), e["field"]
        z_shares = model_finish(port, f, d, lo.reshape(n, a * b, L))
        assert np.array_equal(z_shares.reshape(want["z_shares"].shape), want["z_shares"]), e["field"]
        z = model_open(port, f, z_shares)
        assert np.array_equal(z, want["z"]), e["field"]
        assert np.array_equal(z.reshape(a, b, L), port.matmul(f, want["x"].reshape(a, K, L), want["y"].reshape(K, b, L))), e["field"]


# ---- the model itself ----------------------------------------------------------------------------------------------------------
def _plain(port, f, xi, yi, ri):
    """sum x y + r over the integers the elements ARE in memory (Montgomery residues: a product carries R^-1)"""
    if f == O.GF2_128:
        acc = ri
        for a, b in zip(xi, yi):
            acc ^= gf_mul(a, b)
        return acc
    p, R = {O.MONT128: (MONT_P, 1 << 128), O.SECP256K1_FIELD: (2 ** 256 - 2 ** 32 - 977, 1 << 256)}[f]
    return (sum(a * b for a, b in zip(xi, yi)) * pow(R, -1, p) + ri) % p


@pytest.mark.parametrize("f", [O.MONT128, O.GF2_128, O.SECP256K1_FIELD], ids=["mont128", "gf128", "secp_field"])
def test_the_model_over_the_fields_without_a_fixture(port, f):
    """Mont128, GF(2^128) and the secp256k1 prime: model_dot_mask and model_matmul_mask against plain Python integers (GF(2^128):
    the shift-xor multiplier), with and without the addend, and against Port.dot / Port.matmul column by column"""
    L, N = O.LIMBS[f], 5
    zero = np.zeros(L, dtype=np.uint64)
    for K in (1, 3, 7):
        x = port.vector_random(f, b"ip-model-x%d" % K, K * N).reshape(K, N, L)
        y = port.vector_random(f, b"ip-model-y%d" % K, K * N).reshape(K, N, L)
        r = port.vector_random(f, b"ip-model-r%d" % K, N)
        for r2 in (None, r):
            got = model_dot_mask(port, f, x, y, r2)
            for s in range(N):
                xi, yi = O.to_ints(x[:, s]), O.to_ints(y[:, s])
                assert O.to_ints(got[s:s + 1])[0] == _plain(port, f, xi, yi, 0 if r2 is None else O.to_ints(r2[s:s + 1])[0]), (K, s)
                with_dot = port.dot(f, x[:, s], y[:, s])
                assert np.array_equal(got[s], with_dot if r2 is None else port.ew(f, O.ADD, with_dot[None], r2[s:s + 1])[0])
    a, K, b = 2, 3, 2
    X = port.vector_random(f, b"ip-model-X", 2 * a * K * N).reshape(2, a, K, N, L)
    Y = port.vector_random(f, b"ip-model-Y", 2 * K * b * N).reshape(2, K, b, N, L)
    R2 = port.vector_random(f, b"ip-model-R", 2 * a * b * N).reshape(2, a, b, N, L)
    for r2 in (None, R2):
        got = model_matmul_mask(port, f, X, Y, r2)
        for q in range(2):
            for s in range(N):
                want = port.matmul(f, np.ascontiguousarray(X[q, :, :, s]), np.ascontiguousarray(Y[q, :, :, s]))
                if r2 is not None:
                    want = _ew(port, f, O.ADD, want, r2[q, :, :, s])
                assert np.array_equal(got[q, :, :, s], want), (q, s)
    assert np.array_equal(model_dot_mask(port, f, x[:1], y[:1], zero[None].repeat(N, axis=0)), port.ew(f, O.MUL, x[0], y[0]))


# ---- the per-element forms -------------------------------------------------------------------------------------------------------
def test_the_per_element_forms_equal_the_reduced_operations(tmp_path):
    """every field struct: ip_mac_step / ip_finish / ip_dot_one and a tile under one count == mul and add one at a time, over 1,
    2, 3, 4, 7, 63, 64, 65, 127, 128, 129 and 300 terms, uniform and all at p - 1, with and without the addend; the term count
    never passes the field's bound and the addend folds first exactly when the bound is met"""
    host_check(tmp_path, "ip_host_check.cc", "ip_host_check", ("-w", "-O2"))


def test_the_per_element_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    assert "runtime error" not in host_check(tmp_path, "ip_host_check.cc", "ip_host_check_san", ("-w",) + SANITIZE)


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_mirror_prints_the_fixture():
    """the mirror's ss::shamirSecretShare on its util::PRG in the fixture's order, the local step through ip_dot_one
    (detail/ip.hpp), the open and the finish: what it prints is the fixture (exit status 0: every z is the inner product)"""
    r = mirror_host_output("ip")
    assert json.loads(r.stdout) == golden("ip")
    dynamic = needed(mirror_binary("ip"))
    assert "libscl_hip_ip.so" in dynamic and "libscl_hip.so" in dynamic
