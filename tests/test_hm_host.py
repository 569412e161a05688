"""Honest-majority multiplication, the host half: a Python model of the double-sharing discipline and of the protocol built from
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
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_triples_host import _horner_at_bit_patterns, _newest_header, _random, _stream, bpe, from_hex, poly_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_hm.json")
TAGS = {"m61": O.M61, "m127": O.M127, "secp256k1_scalar": O.SECP256K1_SCALAR, "secp256k1_field": O.SECP256K1_FIELD}
FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]


# ---- the model ---------------------------------------------------------------------------------------------------------------
def double_blocks(f, t):
    return bpe(f) + poly_blocks(f, t) + poly_blocks(f, 2 * t)


def _share_draw(port, f, st, block, secret, d, n):
    """shamirSecretShare(secret, d, n, prg) with the prg at block `block` of each row of the stream -> [n][N][L]"""
    N, E, L = st.shape[0], O.byte_size(f), O.LIMBS[f]
    draw = port.from_bytes(f, np.ascontiguousarray(st[:, 16 * block:16 * block + (d + 1) * E]).tobytes()).reshape(N, d + 1, L)
    if d == 0:
        shares = np.repeat(secret[:, None, :], n, axis=1)
    elif f == O.GF2_128:
        shares = _horner_at_bit_patterns(port, f, secret, draw[:, 1:], n)
    else:
        shares = port.shamir_share_coeffs(f, secret, np.ascontiguousarray(draw[:, 1:]), n)     # element 0 is discarded
    return np.ascontiguousarray(np.transpose(shares, (1, 0, 2)))


def model_double(port, f, seed, counter0, N, t, n):
    """-> lo, hi as [n][N][L] (party-major, the device layout) and r [N][L]"""
    st = _stream(port, seed, counter0, N, double_blocks(f, t))
    r = _random(port, f, st, 0)
    return _share_draw(port, f, st, bpe(f), r, t, n), _share_draw(port, f, st, bpe(f) + poly_blocks(f, t), r, 2 * t, n), r


def model_inputs(port, f, seed, P, t, n):
    """P products' inputs off one PRG: x, y = FF::random, then the degree-t sharings of x and of y, product after product
    -> x, y [P][L], xs, ys [n][P][L]"""
    B = 2 * bpe(f) + 2 * poly_blocks(f, t)
    st = _stream(port, seed, 0, P, B)
    x, y = _random(port, f, st, 0), _random(port, f, st, bpe(f))
    return x, y, _share_draw(port, f, st, 2 * bpe(f), x, t, n), _share_draw(port, f, st, 2 * bpe(f) + poly_blocks(f, t), y, t, n)


def nodes(port, f, n):
    return np.stack([port.from_int(f, i + 1) for i in range(n)])


def model_him(port, f, m, n, points=None):
    """row i = the Lagrange basis of the nodes 1..n at the point -i (GF(2^128): at the bit pattern n + 1 + i) -> [m][n][L]"""
    zero = port.from_int(f, 0)
    if points is None:
        points = [n + 1 + i for i in range(m)] if f == O.GF2_128 else [-i for i in range(m)]
    xs = [port.from_int(f, p) if p >= 0 else port.ew(f, O.SUB, zero[None], port.from_int(f, -p)[None])[0] for p in points]
    return np.stack([port.lagrange_basis(f, nodes(port, f, n), x) for x in xs])


def model_apply(port, f, M, x):
    """out[k] = sum_i M[k][i] x[i]: M [m][n][L], x [n][N][L] -> [m][N][L]"""
    return port.matmul(f, M, x)


def model_mask(port, f, x, y, r2):
    return port.ew(f, O.ADD, port.ew(f, O.MUL, x, y), r2)


def model_open(port, f, dsh, lam=None):
    """dsh [m][N][L] at the nodes 1..m -> [N][L]"""
    if lam is None:
        lam = port.lagrange_basis(f, nodes(port, f, dsh.shape[0]), port.from_int(f, 0))
    return port.shamir_recover_lambda(f, np.ascontiguousarray(np.transpose(dsh, (1, 0, 2))), lam)


def model_finish(port, f, opened, r):
    """r [rows][N][L] -> opened - r"""
    return np.stack([port.ew(f, O.SUB, opened, row) for row in r])


def model_protocol(port, f, n, t, S, dealer_seeds, input_seed):
    """n dealers, S double sharings each, extraction with hyperInvertible(n - t, n), product p = S k + s -> dict of arrays:
    lo, hi [dealer][party][S], M, R_lo, R_hi [party][(n-t) S], x, y, xs, ys, d_shares, d, z_shares, z"""
    m = n - t
    deals = [model_double(port, f, s, 0, S, t, n) for s in dealer_seeds]
    lo, hi = np.stack([d[0] for d in deals]), np.stack([d[1] for d in deals])
    M = model_him(port, f, m, n)
    L = O.LIMBS[f]
    R_lo = np.stack([model_apply(port, f, M, np.ascontiguousarray(lo[:, j])).reshape(m * S, L) for j in range(n)])
    R_hi = np.stack([model_apply(port, f, M, np.ascontiguousarray(hi[:, j])).reshape(m * S, L) for j in range(n)])
    x, y, xs, ys = model_inputs(port, f, input_seed, m * S, t, n)
    d_shares = model_mask(port, f, xs, ys, R_hi)
    d = model_open(port, f, d_shares)
    z_shares = model_finish(port, f, d, R_lo)
    return {"lo": lo, "hi": hi, "M": M, "R_lo": R_lo, "R_hi": R_hi, "x": x, "y": y, "xs": xs, "ys": ys, "d_shares": d_shares, "d": d,
            "z_shares": z_shares, "z": model_open(port, f, z_shares)}


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["data"]


def protocol_entry(port, f, e):
    """one `protocol` run of the fixture in model_protocol's layout"""
    S = len(e["dealers"][0]["sharings"])
    col = lambda rows: np.stack([from_hex(port, f, r) for r in rows], axis=1)            # [p][party] -> [party][p]
    out = {"lo": np.stack([col([s["lo"] for s in d["sharings"]]) for d in e["dealers"]]),
           "hi": np.stack([col([s["hi"] for s in d["sharings"]]) for d in e["dealers"]]),
           "R_lo": col([s["v"] for k in e["R_lo"] for s in k]), "R_hi": col([s["v"] for k in e["R_hi"] for s in k])}
    for k in ("d_shares", "z_shares"):
        out[k] = col([p[k] for p in e["products"]])
    for k in ("x", "y", "d", "z"):
        out[k] = from_hex(port, f, e[k])
    return out, S


@pytest.fixture(scope="module")
def port():
    p = O.Port()
    p.mont128_set_prime((1 << 128) - 159)
    return p


def test_the_model_deals_the_fixtures_double_sharings(port):
    """every run: five consecutive double sharings at (3,1), (4,1), (7,3), (10,3), (9,4), and the run after a three-block burn"""
    runs = golden()["double"]
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
    runs = golden()["protocol"]
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
    runs = golden()["him"]
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
def hm_binary(name="test_hm_api", flags=("-O2",)):
    """tests/cxx/test_hm_api.cc compiled against the mirror and the libraries (build() leaves it in place; rebuilt here when stale)"""
    src, exe = os.path.join(CXX, "test_hm_api.cc"), os.path.join(CXX, "_build", name)
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(_newest_header(), os.path.getmtime(src)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{lib}", "-lscl_hip_hm", "-lscl_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def mirror_output(exe):
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_the_mirror_prints_the_fixture():
    """ss::doubleShare, Matrix::hyperInvertible and the protocol through hm_mask_one / hm_mac_step / hm_finish_one on the fixture's
    seeds, burns and shapes print the fixture (exit status 0: every z = x y)"""
    r = mirror_output(hm_binary())
    assert json.loads(r.stdout) == golden()
    needed = subprocess.run(["readelf", "-d", hm_binary()], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip_hm.so" in needed and "libscl_hip.so" in needed


def test_the_mirror_under_the_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined: the same output, no report"""
    exe = hm_binary("test_hm_api_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    r = mirror_output(exe)
    assert json.loads(r.stdout) == golden()
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def host_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++20", "-w", f"-I{ROOT}/include", *flags, "-o", exe, os.path.join(CXX, "hm_host_check.cc")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    return r.stdout + r.stderr


def test_the_per_element_forms_equal_the_reduced_operations(tmp_path):
    """every field struct: hm_mask_one, hm_finish_one and the accumulation step == mul / add / sub one at a time, at the extreme
    operands, at 10^5 uniform tuples, and over 1, 3, 10, 64, 65 and 300 terms, uniform and all at p - 1"""
    host_check(tmp_path, "hm_host_check", ["-O2"])


def test_the_per_element_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    assert "runtime error" not in host_check(tmp_path, "hm_host_check_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                                                            "-fno-sanitize-recover=undefined"])
