"""Batch verification, the host half: a Python model of the random linear combination out[r][j] = sum_s rho_j[s] x[r][s] (y[r][s])
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
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_triples_host import from_hex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_vf.json")
TAGS = {"m61": O.M61, "m127": O.M127, "secp256k1_scalar": O.SECP256K1_SCALAR}
FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
MONT_P = (1 << 128) - 159


# ---- the model ---------------------------------------------------------------------------------------------------------------
def coin_blocks(f, N):
    return -(-N * O.byte_size(f) // 16)


def model_coins(port, f, seed, counter0, N, reps):
    """-> rho [reps][N][L]: `reps` consecutive Vector::random(N) of a PRG on `seed` at block counter0"""
    bs, B = O.byte_size(f), coin_blocks(f, N)
    if N == 0:
        return np.zeros((reps, 0, O.LIMBS[f]), dtype=np.uint64)
    return np.stack([port.from_bytes(f, port.prg_blocks(seed, counter0 + j * B, B)[:N * bs]) for j in range(reps)])


def model_combine(port, f, x, rho, y=None):
    """x (y) [rows][N][L], rho [reps][N][L] -> [rows][reps][L]: Port.dot of rho_j with x_r (x_r .* y_r); the empty sum is zero"""
    rows, N, L = x.shape
    out = np.zeros((rows, rho.shape[0], L), dtype=np.uint64)
    if N == 0:
        return out
    for r in range(rows):
        m = np.ascontiguousarray(x[r]) if y is None else port.ew(f, O.MUL, np.ascontiguousarray(x[r]), np.ascontiguousarray(y[r]))
        for j in range(rho.shape[0]):
            out[r, j] = port.dot(f, np.ascontiguousarray(rho[j]), m)
    return out


def lies_on(port, f, shares, d):
    """shares [n][L] at the nodes 1..n: do shares d+1.. lie on the polynomial through the first d+1?  -> (bool, its value at 0)"""
    L, n = O.LIMBS[f], shares.shape[0]
    nodes = np.stack([port.from_int(f, i + 1) for i in range(d + 1)])
    at = lambda x: port.shamir_recover_at(f, shares[None, :d + 1], nodes, port.from_int(f, x))[0]
    return all(np.array_equal(at(i + 1), shares[i]) for i in range(d + 1, n)), at(0)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["data"]


def hex_rows(port, f, rows):
    return np.stack([from_hex(port, f, r) for r in rows])


def degree_entry(port, f, e):
    """-> rows [n][N][L] (party i's shares of the N secrets), rho [1][N][L], secrets"""
    secrets = port.vector_random(f, b"vf secrets", e["N"])
    assert np.array_equal(secrets, from_hex(port, f, e["secrets"]))
    shares = port.shamir_share(f, b"vf sharing", secrets, e["t"], e["n"])                  # [N][n][L], one PRG, secret after secret
    return np.ascontiguousarray(np.transpose(shares, (1, 0, 2))), model_coins(port, f, b"vf coin", e["counter0"], e["N"], 1), secrets


def product_entry(port, f, e):
    """-> a, b, c rows [n][N][L], rho [1][N][L]"""
    a, b = port.vector_random(f, b"vf a", e["N"]), port.vector_random(f, b"vf b", e["N"])
    assert np.array_equal(a, from_hex(port, f, e["a"])) and np.array_equal(b, from_hex(port, f, e["b"]))
    c = port.ew(f, O.MUL, a, b)
    sh = lambda seed, v: np.ascontiguousarray(np.transpose(port.shamir_share(f, seed, v, e["t"], e["n"]), (1, 0, 2)))
    return sh(b"vf share a", a), sh(b"vf share b", b), sh(b"vf share c", c), model_coins(port, f, b"vf coin", e["counter0"], e["N"], 1)


def model_product_check(port, f, a, b, c, rho):
    """every party's sum rho a b - sum rho c -> [n][L]"""
    return port.ew(f, O.SUB, model_combine(port, f, a, rho, b)[:, 0], model_combine(port, f, c, rho)[:, 0])


@pytest.fixture(scope="module")
def port():
    p = O.Port()
    p.mont128_set_prime(MONT_P)
    return p


def test_the_fixture_has_the_documented_shape():
    g = golden()
    assert [e["field"] for e in g["combine"]] == [e["field"] for e in g["degree"]] == [e["field"] for e in g["product"]] == list(TAGS)
    for e in g["combine"]:
        assert [r["N"] for r in e["runs"]] == [1, 2, 5] and len(e["x"]) == len(e["y"]) == 3
        assert all(r["counter0"] == coin_blocks(TAGS[e["field"]], 3) > 0 for r in e["runs"])
    assert all((e["n"], e["t"], e["N"]) == (4, 1, 5) for e in g["degree"] + g["product"])
    assert os.path.getsize(GOLDEN) < 16 * 1024


def test_the_model_computes_the_fixtures_combinations(port):
    """every field, N = 1, 2, 5 (the first N columns of rows 5 apart), reps = 2 (reps = 1 is its first column), plain and product:
    the model's values are the reference's innerProd results; the inputs are the PRG's"""
    for e in golden()["combine"]:
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
    for e in golden()["degree"]:
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
    for e in golden()["product"]:
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
def host_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++20", "-w", f"-I{ROOT}/include", *flags, "-o", exe, os.path.join(CXX, "vf_host_check.cc")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    return r.stdout + r.stderr


def test_the_per_element_forms_equal_the_reduced_operations(tmp_path):
    """every field struct: vf_take (two repetitions under one count), vf_combine_one, vf_take_partial and vf_sum_partials == mul
    and add one at a time, over 1, 2, 3, 63, 64, 65, 127, 128, 129 and 300 terms of (p-1)(p-1) and of (p-1)(p-1)(p-1), and
    uniform; the term count never passes the field's bound"""
    host_check(tmp_path, "vf_host_check", ["-O2"])


def test_the_per_element_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    assert "runtime error" not in host_check(tmp_path, "vf_host_check_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                            "-fno-sanitize-recover=undefined"])


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def vf_binary(name="test_vf_api", flags=("-O2",)):
    """tests/cxx/test_vf_api.cc compiled against the mirror and the libraries (build() leaves it in place; rebuilt here when stale)"""
    from test_hm_host import _newest_header
    src, exe = os.path.join(CXX, "test_vf_api.cc"), os.path.join(CXX, "_build", name)
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(_newest_header(), os.path.getmtime(src)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{lib}", "-lscl_hip_vf", "-lscl_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def test_the_mirror_prints_the_fixture():
    """the mirror's Vector::random coins (ss::combineCoins on a util::PRG that drew and discarded three elements), ss::combine --
    held against vf_combine_one of detail/vf.hpp on the limbs --, ss::shamirSecretShare, ss::shamirRecoverD / P in the fixture's
    order: what it prints is the fixture (exit status 0: every open is what the harness of the reference required)"""
    r = subprocess.run([vf_binary(), "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.loads(r.stdout) == golden()
    needed = subprocess.run(["readelf", "-d", vf_binary()], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip_vf.so" in needed and "libscl_hip.so" in needed
