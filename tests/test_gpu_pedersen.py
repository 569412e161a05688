"""Pedersen VSS on the GPU: scl_hip_ec_mul_two_base, scl_hip_ec_matmul and scl_hip_pedersen_* (csrc/pedersen_unit.hip) against
what the reference computed (tests/golden/golden_pedersen.json) and against the big-integer Python model of
tests/secp256k1_model.py (pinned to that fixture by tests/test_pedersen_host.py) -- never against the library, except where a test says that two
entry points must agree.  Everything is exact: every comparison is byte equality of wire images or of verdict bytes.  The
model's work is kept to a few hundred scalar multiplications over the whole file."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest
import torch

from cxx_support import mirror_binary
from gpu_support import images, points_dev, rescale, scalars_dev, scalars_host
from secp256k1_model import G, Q, ec_from_image, ec_image, ec_mul, matrix_of, pedersen_commitment, pedersen_verify, run_commitments, run_pairs, scalar_of
from secp256k1_model import pedersen_golden as golden
from secp256k1_model import write_pedersen_cases as write_cases

pytestmark = pytest.mark.gpu
INF = b"\x06" + bytes(64)
H = ec_mul(42, G)


@pytest.fixture(scope="module")
def scl():
    import scl_amd
    assert torch.cuda.is_available()
    return scl_amd


@pytest.fixture(scope="module")
def gtable(scl):
    return scl.ec_base_table()


def table_of(scl, point):
    return scl.ec_base_table(scl.to_host(points_dev(scl, [point]))[0])


@pytest.fixture(scope="module")
def htable(scl):
    return table_of(scl, H)


def rnd_scalars(seed: int, count: int):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(32), "big") % Q for _ in range(count)]


# ---- mul_two_base -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_base_cases():
    """(a, b) and the model's image of a G + b H: the edge cases test_mul_two_base names and eight drawn pairs"""
    r = rnd_scalars(42, 18)
    pairs = [(0, 0), (r[0], 0), (0, r[1]), (Q - 42, 1), (42, 1), (Q - 1, Q - 1), (15 * 16 ** 63, 16 ** 63)]
    pairs += [(r[2 + 2 * i], r[3 + 2 * i]) for i in range(8)]
    want = [ec_image(pedersen_commitment(a, b, H)) for a, b in pairs]
    assert want[0] == INF and want[3] == INF and want[4] == ec_image(ec_mul(84, G))
    return pairs, want


@pytest.mark.parametrize("N", [1, 65])
def test_mul_two_base(scl, gtable, htable, N):
    """a G + b H with H = 42 G: (0, 0) and (q - 42, 1) give infinity (the second by a mixed addition of P and -P), (42, 1) is a
    mixed addition of equal points, (a, 0) and (0, b) leave one table unused, (q - 1, q - 1), only digit 63 set, eight drawn
    pairs.  N = 1 runs every pair in a call of its own, N = 65 tiles them over one full wave and a tail lane"""
    pairs, want = two_base_cases()
    if N == 1:
        for (a, b), w in zip(pairs, want):
            assert images(scl, scl.ec_mul_two_base(gtable, htable, scalars_dev(scl, [a]), scalars_dev(scl, [b]))) == [w], (a, b)
        return
    idx = [i % len(pairs) for i in range(N)]
    out = scl.ec_empty(N)
    got = scl.ec_mul_two_base(gtable, htable, scalars_dev(scl, [pairs[i][0] for i in idx]), scalars_dev(scl, [pairs[i][1] for i in idx]),
                              out=out)
    assert got is out and images(scl, got) == [want[i] for i in idx]


def test_mul_two_base_with_a_table_of_another_base_in_both_slots(scl):
    """the table of 7 G as both bases: a (7 G) + b (7 G) = 7 (a + b) G by the model"""
    pairs, _ = two_base_cases()
    table = table_of(scl, ec_mul(7, G))
    got = images(scl, scl.ec_mul_two_base(table, table, scalars_dev(scl, [a for a, _ in pairs]), scalars_dev(scl, [b for _, b in pairs])))
    assert got == [ec_image(ec_mul(7 * (a + b), G)) for a, b in pairs]


# ---- ec_matmul ----------------------------------------------------------------------------------------------------------
def matrix_dev(scl, M) -> torch.Tensor:
    return scalars_dev(scl, [v for row in M for v in row]).reshape(len(M), len(M[0]), 4)


def multiples_dev(scl, gtable, a, pitch: int = 0, rescaled: int = 0) -> torch.Tensor:
    """points [p][cols] with P[k][c] = a[k][c] G, rows `pitch` points further apart than they are long; rows past the first
    under random projective coordinates when `rescaled` (a seed) is given"""
    p, cols = len(a), len(a[0])
    rows = scl.ec_empty(p, cols + pitch)
    for k in range(p):
        pts = scl.ec_mul_base(gtable, scalars_dev(scl, a[k]))
        rows[k, :cols] = rescale(scl, pts, rescaled + k) if rescaled and k else pts
    return rows[:, :cols]


def check_matmul(scl, gtable, M, a, got):
    """got[i][c] == (sum_k M[i][k] a[k][c]) G: all of them against mul_base (pinned to the model in test_gpu_feldman.py), the two
    ends of every row against the model"""
    rows, cols = len(M), len(a[0])
    total = [[sum(m * a[k][c] for k, m in enumerate(M[i])) % Q for c in range(cols)] for i in range(rows)]
    got = images(scl, got)
    assert got == images(scl, scl.ec_mul_base(gtable, scalars_dev(scl, [v for row in total for v in row])))
    for i in range(rows):
        for c in {0, cols - 1}:
            assert got[i * cols + c] == ec_image(ec_mul(total[i][c], G)), (i, c)
    return got


@pytest.mark.parametrize("cols", [1, 65])
@pytest.mark.parametrize("p", [1, 5])
@pytest.mark.parametrize("rows", [1, 3])
def test_matmul(scl, gtable, rows, p, cols):
    """M [rows][p] times P [p][cols], P[k][c] = a[k][c] G under random projective coordinates, rows a pitch of cols + 3 apart:
    the identity and vandermonde(3, 5) (their leading rows x p block), rows that are all zero (infinity), whose only entry is
    q - 1 in the last column (top bit 255) and whose only entry is 1 (top bit 0: no doubling that matters), and drawn
    full-width entries"""
    a = [rnd_scalars(1000 * rows + 100 * p + cols + k, cols) for k in range(p)]
    points = multiples_dev(scl, gtable, a, pitch=3, rescaled=7)
    special = [[0] * p, [0] * (p - 1) + [Q - 1], [1] + [0] * (p - 1)]
    r = rnd_scalars(rows * p + cols, rows * p)
    matrices = [[[int(i == k) for k in range(p)] for i in range(rows)], [[(i + 1) ** k for k in range(p)] for i in range(rows)],
                [r[i * p:(i + 1) * p] for i in range(rows)]]
    matrices += [special] if rows == 3 else [[row] for row in special]
    for M in matrices:
        got = check_matmul(scl, gtable, M, a, scl.ec_matmul(matrix_dev(scl, M), points))
        for i, row in enumerate(M):
            if not any(row):
                assert got[i * cols:(i + 1) * cols] == [INF] * cols


def test_matmul_over_more_point_rows_than_one_launch_recodes(scl, gtable):
    """p = 257, rows = 2, cols = 1: the kernel recodes 256 scalars a launch, the 257th point row goes through a second launch
    that adds to dst.  P[k] = (k + 1) G; the scalars are 0 or 1 but for three drawn ones (first, last of the first launch, and
    the one of the second launch); row 1's entry in the second launch is 0, so that launch must leave its sum alone"""
    p, r = 257, rnd_scalars(257, 4)
    M = [[(k * 7 + i) % 3 % 2 for k in range(p)] for i in range(2)]
    M[0][0], M[0][255], M[0][256], M[1][5], M[1][256] = r[0], r[1], r[2], r[3], 0
    a = [[k + 1] for k in range(p)]
    points = scl.ec_mul_base(gtable, scalars_dev(scl, [k + 1 for k in range(p)])).reshape(p, 1, 12)
    check_matmul(scl, gtable, M, a, scl.ec_matmul(matrix_dev(scl, M), points))


def test_matmul_agrees_with_lincomb_row_by_row(scl, gtable):
    """the same operands through scl_hip_ec_lincomb, one call per row of M: equal points (compared with ec_equal: the two chains
    start at different bits, so the limbs may differ)"""
    rows, p, cols = 3, 5, 65
    a = [rnd_scalars(50 + k, cols) for k in range(p)]
    M = [rnd_scalars(60 + i, p) for i in range(rows)]
    M[1] = [3, 0, 1, 2, 0]
    points = multiples_dev(scl, gtable, a)
    got = scl.ec_matmul(matrix_dev(scl, M), points)
    for i in range(rows):
        assert scl.ec_equal(got[i], scl.ec_lincomb(points, scalars_dev(scl, M[i]))).cpu().tolist() == [1] * cols


# ---- pedersen_commit / pedersen_verify ----------------------------------------------------------------------------------
def share_run(scl, r):
    """the run's sharing on its seed through scl_hip_shamir_share_prg_packed: secrets [2][1][4], shares [2][n][1][4]"""
    secrets = scalars_dev(scl, [scalar_of(r["secret"]), scalar_of(r["randomness"])]).reshape(2, 1, 4)
    shares = scl.shamir_share_prg_packed(scl.SECP256K1_SCALAR, secrets, r["t"], r["n"], r["seed"].encode(), counter0=r["counter0"])
    return secrets, shares


@pytest.mark.parametrize("which", ["runs", "run5", "hom_runs", "apply"])
def test_pedersen_commit_and_verify_reproduce_the_reference(scl, gtable, htable, which):
    """every sharing of the fixture -- (t, n) in {(0,1), (1,2), (3,10), (4,24)} with seed "Pedersen", the 5-argument overload,
    the two of "Pedersen hom" and the five of "Pedersen apply" off one PRG each -- dealt by scl_hip_shamir_share_prg_packed:
    shares and commitments equal the reference's byte for byte, every party verifies, index 0 verifies the secret, the five
    tampered inputs give 0"""
    d = golden()
    f = scl.SECP256K1_SCALAR
    wrong = table_of(scl, ec_from_image(bytes.fromhex(d["h_wrong"])))
    for r in {"runs": d["runs"], "run5": [d["run5"]], "hom_runs": d["hom_runs"], "apply": d["apply"]["sharings"]}[which]:
        t, n = r["t"], r["n"]
        secrets, shares = share_run(scl, r)
        assert list(zip(scalars_host(scl, shares[0]), scalars_host(scl, shares[1]))) == run_pairs(r), (t, n)
        com = scl.pedersen_commit(gtable, htable, secrets, shares, t)
        assert [b.hex() for b in images(scl, com)] == r["commitments"], (t, n)
        assert scl.pedersen_verify(gtable, htable, secrets[0], secrets[1], com, scl.feldman_lambda(t, 0)).cpu().tolist() == [1]
        for p in range(n):
            ok = scl.pedersen_verify(gtable, htable, shares[0, p], shares[1, p], com, scl.feldman_lambda(t, p + 1))
            assert ok.cpu().tolist() == [1], (t, n, p)
        if t >= 1:
            s, b, one, lam = shares[0, n - 1], shares[1, n - 1], scalars_dev(scl, [1]), scl.feldman_lambda(t, n)
            g_first = com.clone()
            g_first[0] = points_dev(scl, [G])
            assert scl.pedersen_verify(gtable, htable, scl.ew(f, scl.ADD, s, one), b, com, lam).cpu().tolist() == [0]
            assert scl.pedersen_verify(gtable, htable, s, scl.ew(f, scl.ADD, b, one), com, lam).cpu().tolist() == [0]
            assert scl.pedersen_verify(gtable, htable, s, b, g_first, lam).cpu().tolist() == [0]
            assert scl.pedersen_verify(gtable, htable, s, b, com, scl.feldman_lambda(t, n - 1)).cpu().tolist() == [0]
            assert scl.pedersen_verify(gtable, wrong, s, b, com, lam).cpu().tolist() == [0]


def tiled_sharings(scl, runs, N):
    """lane s holds sharing s mod len(runs) of the fixture: secrets [2][N][4], shares [2][n][N][4], the images wanted"""
    n, pick = runs[0]["n"], [runs[s % len(runs)] for s in range(N)]
    secrets = torch.stack([scalars_dev(scl, [scalar_of(r[key]) for r in pick]) for key in ("secret", "randomness")])
    shares = torch.stack([torch.stack([scalars_dev(scl, [run_pairs(r)[i][c] for r in pick]) for i in range(n)]) for c in (0, 1)])
    want = [r["commitments"][k] for k in range(runs[0]["t"] + 1) for r in pick]
    return secrets.contiguous(), shares.contiguous(), want


def test_lanes_are_independent(scl, gtable, htable):
    """N = 65: lane s holds sharing s mod 5 of "Pedersen apply" (five different secrets, blindings and polynomials side by
    side); the commitments are the fixture's, tiled, and every party verifies in every lane"""
    runs, N = golden()["apply"]["sharings"], 65
    secrets, shares, want = tiled_sharings(scl, runs, N)
    com = scl.pedersen_commit(gtable, htable, secrets, shares, 2)
    assert [b.hex() for b in images(scl, com)] == want
    for p in range(5):
        assert scl.pedersen_verify(gtable, htable, shares[0, p], shares[1, p], com, scl.feldman_lambda(2, p + 1)).cpu().tolist() == [1] * N


def test_pedersen_verify_finds_exactly_the_planted_errors(scl, gtable, htable):
    """65 secrets of (10, 3) verified at the last party's index, one error of each kind a lane can carry planted at lanes 0, 31,
    63 and 64: share + 1, randomness + 1, commitment 0 replaced by G, and the share of the party before (the share is right,
    its index is not).  The verdicts are the complement of the planted set, and the model agrees on those four lanes and one
    honest one.  The fifth kind, another h, is the whole call's: every lane is refused"""
    f, N, t, n = scl.SECP256K1_SCALAR, 65, 3, 10
    secrets = torch.stack([scl.vector_random(f, N, b"planted-secrets"), scl.vector_random(f, N, b"planted-blindings")])
    shares = scl.shamir_share_prg_packed(f, secrets, t, n, b"planted")
    com = scl.pedersen_commit(gtable, htable, secrets, shares, t)
    lam, one = scl.feldman_lambda(t, n), scalars_dev(scl, [1])
    s, b = shares[0, n - 1].clone(), shares[1, n - 1].clone()
    assert scl.pedersen_verify(gtable, htable, s, b, com, lam).cpu().tolist() == [1] * N
    s[0:1] = scl.ew(f, scl.ADD, s[0:1].contiguous(), one)
    b[31:32] = scl.ew(f, scl.ADD, b[31:32].contiguous(), one)
    bad = com.clone()
    bad[0, 63] = points_dev(scl, [G])[0]
    s[64], b[64] = shares[0, n - 2, 64], shares[1, n - 2, 64]
    planted = {0, 31, 63, 64}
    assert scl.pedersen_verify(gtable, htable, s, b, bad, lam).cpu().tolist() == [int(i not in planted) for i in range(N)]
    got, sh, bl = images(scl, bad), scalars_host(scl, s), scalars_host(scl, b)
    for lane in sorted(planted | {33}):
        assert pedersen_verify(sh[lane], bl[lane], [ec_from_image(got[k * N + lane]) for k in range(t + 1)], n, H) == (lane == 33)
    wrong = table_of(scl, ec_mul(43, G))
    assert scl.pedersen_verify(gtable, wrong, shares[0, n - 1], shares[1, n - 1], com, lam).cpu().tolist() == [0] * N


def test_pedersen_is_additively_homomorphic(scl, gtable, htable):
    """"Pedersen hom": the fixture's two sharings off one PRG, their commitments added through ec_ew(ADD) and their shares over
    the field: the sums are the reference's, party 4's summed share verifies at 5 and the recovered pair at 0; the first
    sharing's own share does not verify against the summed commitments"""
    d = golden()
    f, hom = scl.SECP256K1_SCALAR, d["hom"]
    (sa, a), (sb, b) = (share_run(scl, r) for r in d["hom_runs"])
    ca, cb = scl.pedersen_commit(gtable, htable, sa, a, 4), scl.pedersen_commit(gtable, htable, sb, b, 4)
    com2 = scl.ec_ew(scl.ADD, ca.reshape(-1, 12), cb.reshape(-1, 12)).reshape(5, 1, 12)
    assert [x.hex() for x in images(scl, com2)] == hom["commitments"]
    sum2 = scl.ew(f, scl.ADD, a.reshape(-1, 4), b.reshape(-1, 4)).reshape(a.shape)
    assert list(zip(scalars_host(scl, sum2[0]), scalars_host(scl, sum2[1]))) == run_pairs({"shares": hom["shares"], "n": 10})
    assert scl.pedersen_verify(gtable, htable, sum2[0, 4], sum2[1, 4], com2, scl.feldman_lambda(4, 5)).cpu().tolist() == [1]
    total = scalars_dev(scl, [scalar_of(hom["sum_secret"]), scalar_of(hom["sum_randomness"])])
    assert scl.pedersen_verify(gtable, htable, total[0:1], total[1:2], com2, scl.feldman_lambda(4, 0)).cpu().tolist() == [1]
    assert scl.pedersen_verify(gtable, htable, a[0, 4], a[1, 4], com2, scl.feldman_lambda(4, 5)).cpu().tolist() == [0]


def test_apply_reproduces_the_reference_through_the_abi(scl, gtable, htable):
    """"Pedersen apply" over the C ABI: the commitments of the five sharings as P [5][3] (sharing-major), vandermonde(3, 5) and
    the identity through ec_matmul, the {share, randomness} rows through scl_hip_matmul: the fixture's outputs byte for byte,
    and every output share verifies at its party's index"""
    ap = golden()["apply"]
    f, runs = scl.SECP256K1_SCALAR, ap["sharings"]
    points = torch.stack([points_dev(scl, run_commitments(r)) for r in runs])                       # [5][3][12]
    pairs = scalars_dev(scl, [v for r in runs for pair in run_pairs(r) for v in pair]).reshape(5, 10, 4)  # [sharing][party, c]
    for key in ("vandermonde", "identity"):
        M, out = matrix_dev(scl, matrix_of(ap[key])), ap[key]["out"]
        rows = ap[key]["rows"]
        com = scl.ec_matmul(M, points)
        got = [x.hex() for x in images(scl, com)]
        sh = scalars_host(scl, scl.matmul(f, M, pairs))
        for j in range(5):
            for i in range(rows):
                assert got[3 * i:3 * i + 3] == out[j][i]["commitments"]
                assert "%064x%064x" % tuple(sh[(i * 5 + j) * 2:(i * 5 + j) * 2 + 2]) == out[j][i]["share"]
        res = scl.matmul(f, M, pairs).reshape(rows, 5, 2, 4)
        for j in range(5):  # the rows of the output are the secrets of a batch: N = rows
            ok = scl.pedersen_verify(gtable, htable, res[:, j, 0].contiguous(), res[:, j, 1].contiguous(),
                                     com.transpose(0, 1).contiguous(), scl.feldman_lambda(2, j + 1))
            assert ok.cpu().tolist() == [1] * rows


def test_cxx_batch_forms_agree_with_the_per_secret_forms(scl, tmp_path):
    """tests/cxx/test_pedersen_api --device: hip::Pedersen (include/scl_hip/hip/pedersen.h) shares, commits and verifies 65
    secrets of (10, 3) off one PRG as ss::pedersenSecretShare / pedersenVerify do secret by secret, and its apply gives the
    fixture's outputs on the fixture's inputs, every output share verifying at its index as in "Pedersen apply\""""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run(["timeout", "-k", "10", "300", mirror_binary("pedersen"), cases, "--device"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device: 65 secrets" in r.stdout and "device apply: 2 matrices" in r.stdout, r.stdout
    assert f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout


def test_commit_and_verify_capture_into_a_hip_graph(scl, gtable, htable):
    """commit then verify allocate nothing, copy nothing and do not synchronise: one capture on one stream, replayed twice on
    new shares (the second time with another lane planted)"""
    f, N, t, n = scl.SECP256K1_SCALAR, 65, 3, 10
    secrets = torch.stack([scl.vector_random(f, N, b"graph-secrets"), scl.vector_random(f, N, b"graph-blindings")])
    shares = scl.shamir_share_prg_packed(f, secrets, t, n, b"graph-0")
    com, scratch = scl.ec_empty(t + 1, N), scl.ec_empty(2 * N)
    ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
    lam, mine, blind = scl.feldman_lambda(t, 7), shares[0, 6].clone(), shares[1, 6].clone()

    def step():
        scl.pedersen_commit(gtable, htable, secrets, shares, t, out=com)
        scl.pedersen_verify(gtable, htable, mine, blind, com, lam, scratch=scratch, out=ok)

    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.synchronize()
    for seed, lane in ((b"graph-1", 2), (b"graph-2", 64)):
        fresh = scl.shamir_share_prg_packed(f, secrets, t, n, seed)
        shares.copy_(fresh)
        mine.copy_(fresh[0, 6])
        blind.copy_(fresh[1, 6])
        blind[lane] = fresh[1, 5, lane]
        ok.zero_()
        com.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert ok.cpu().tolist() == [int(i != lane) for i in range(N)]
        assert images(scl, com) == images(scl, scl.pedersen_commit(gtable, htable, secrets, fresh, t))


def test_error_paths(scl, gtable, htable):
    """a NULL operand, a misaligned buffer, a stride below the row length, n < t and dst over points return their codes with a
    message; n == 0 returns at once"""
    lib, N = scl.lib, 4
    pts, out, sc = scl.ec_empty(2, N), scl.ec_empty(2, N), scalars_dev(scl, list(range(1, 17)))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    size = C.c_size_t
    g, h, p, o, s = gtable.data_ptr(), htable.data_ptr(), pts.data_ptr(), out.data_ptr(), sc.data_ptr()
    assert lib.scl_hip_ec_mul_two_base(o, g, None, s, s, size(N), st) == scl.ERR_BAD_ARG
    assert b"NULL" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_mul_two_base(o + 8, g, h, s, s, size(N), st) == scl.ERR_BAD_ARG
    assert b"16-byte aligned" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_mul_two_base(o, g, h, s, s + 8, size(N), st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ec_matmul(o, size(N), None, size(2), size(2), p, size(N), size(N), st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ec_matmul(o, size(N), s + 8, size(2), size(2), p, size(N), size(N), st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ec_matmul(o, size(N - 1), s, size(2), size(2), p, size(N), size(N), st) == scl.ERR_SIZE_MISMATCH
    assert b"dst_stride < cols" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_matmul(o, size(N), s, size(2), size(2), p, size(N - 1), size(N), st) == scl.ERR_SIZE_MISMATCH
    assert b"row_stride < cols" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_matmul(p, size(N), s, size(2), size(2), p, size(N), size(N), st) == scl.ERR_BAD_ARG
    assert b"overlaps" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_matmul(p + 12 * 8 * (2 * N - 1), size(N), s, size(1), size(2), p, size(N), size(N), st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ec_matmul(o, size(N), s, size(2), size(0), p, size(N), size(N), st) == scl.ERR_BAD_ARG
    commit = lambda *a: lib.scl_hip_pedersen_commit(o, size(a[0]), g, h, s, size(a[1]), s, size(a[2]), size(a[3]), size(a[4]), size(N), st)
    assert commit(N, N, N, 1, 2) == scl.OK  # rows 0 and 1 of `out` from scalars 1..4 | 5..8 and 1..4 | 9..12
    assert commit(N, N, N, 3, 2) == scl.ERR_SIZE_MISMATCH
    assert b"n < t" in lib.scl_hip_last_error()
    assert commit(N - 1, N, N, 1, 2) == scl.ERR_SIZE_MISMATCH
    assert b"commit_stride < N" in lib.scl_hip_last_error()
    assert commit(N, N - 1, N, 1, 2) == scl.ERR_SIZE_MISMATCH
    assert commit(N, N, N - 1, 1, 2) == scl.ERR_SIZE_MISMATCH
    assert b"share_stride < N" in lib.scl_hip_last_error()
    assert lib.scl_hip_pedersen_commit(o, size(N), g, None, s, size(N), s, size(N), size(1), size(2), size(N), st) == scl.ERR_BAD_ARG
    ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
    verify = lambda rand, stride: lib.scl_hip_pedersen_verify(ok.data_ptr(), s, rand, o, size(stride), size(1), s, g, h, p, size(N), st)
    assert verify(None, N) == scl.ERR_BAD_ARG
    assert verify(s + 8, N) == scl.ERR_BAD_ARG
    assert verify(s, N - 1) == scl.ERR_SIZE_MISMATCH
    assert lib.scl_hip_ec_mul_two_base(None, None, None, None, None, size(0), st) == scl.OK
    assert lib.scl_hip_ec_matmul(None, size(0), None, size(0), size(3), None, size(0), size(5), st) == scl.OK
    assert lib.scl_hip_ec_matmul(None, size(0), None, size(3), size(3), None, size(0), size(0), st) == scl.OK
    assert lib.scl_hip_pedersen_commit(None, size(0), None, None, None, size(0), None, size(0), size(3), size(5), size(0), st) == scl.OK
    assert lib.scl_hip_pedersen_verify(None, None, None, None, size(0), size(3), None, None, None, None, size(0), st) == scl.OK
    torch.cuda.synchronize()
    want = [ec_image(pedersen_commitment(a, b, H)) for a, b in ((1, 5), (2, 6), (3, 7), (4, 8), (1, 9), (2, 10), (3, 11), (4, 12))]
    assert images(scl, out) == want
