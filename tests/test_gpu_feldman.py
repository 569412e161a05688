"""secp256k1 group arithmetic and Feldman VSS on the GPU: scl_hip_ec_* and scl_hip_feldman_* (csrc/ec_unit.hip) against what the
reference computed (tests/golden/golden_feldman.json) and against the big-integer Python model of tests/secp256k1_model.py
(pinned to that fixture by tests/test_feldman_host.py) -- never against the library.  Everything is exact: every comparison is byte equality of wire
images or of verdict bytes.  The model's work is kept under ~600 scalar multiplications over the whole file."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from cxx_support import mirror_binary
from gpu_support import images, points_dev, rescale, scalars_dev, scalars_host
from secp256k1_model import G, Q, ec_add, ec_from_image, ec_image, ec_mul, ec_neg, feldman_verify, golden, run_shares
from secp256k1_model import write_feldman_cases as write_cases

pytestmark = pytest.mark.gpu
R = 1 << 256
COUNTS = [1, 63, 64, 65, 300]


@pytest.fixture(scope="module")
def scl():
    import scl_amd
    assert torch.cuda.is_available()
    return scl_amd


@pytest.fixture(scope="module")
def gtable(scl):
    return scl.ec_base_table()


def fixed_scalars():
    """the fixture's scalars with their reference-computed multiples, and one non-zero window at either end (model)"""
    d = golden("feldman")
    ks = [int(m["k"], 16) for m in d["multiples"]]
    want = [bytes.fromhex(m["P"]) for m in d["multiples"]]
    for w in (0, 1, 63):
        for dgt in (1, 15):
            ks.append(16 ** w * dgt)
            want.append(ec_image(ec_mul(ks[-1], G)))
    return ks, want


def test_mul_base_fixed_scalars_and_grid_tails(scl, gtable):
    """k * G for the fixture's scalars (0, 1, 2, 3, 15, 16, 17, 2^64, 2^255, q - 1, eight random) and digits 1 and 15 in windows
    0, 1 and 63, tiled over counts around the block size: images equal the reference's and the model's; also scalar 0 gives
    infinity"""
    ks, want = fixed_scalars()
    assert want[0] == b"\x06" + bytes(64)
    for n in COUNTS:
        idx = [i % len(ks) for i in range(n)]
        got = images(scl, scl.ec_mul_base(gtable, scalars_dev(scl, [ks[i] for i in idx])))
        assert got == [want[i] for i in idx], n


def test_mul_base_with_a_table_of_another_base(scl):
    """a caller-owned table of 7 G: s * (7 G) = (7 s) G by the model"""
    ks, _ = fixed_scalars()
    seven_g = points_dev(scl, [ec_mul(7, G)])
    table = scl.ec_base_table(scl.to_host(seven_g)[0])
    got = images(scl, scl.ec_mul_base(table, scalars_dev(scl, ks)))
    assert got == [ec_image(ec_mul(7 * k, G)) for k in ks]
    assert table.numel() == 64 * 15 * 64 and scl.lib.scl_hip_ec_base_table_bytes() == table.numel()


def test_mul_base_random_scalars(scl, gtable):
    """300 random scalars against the model"""
    rng = np.random.default_rng(20)
    ks = [int.from_bytes(rng.bytes(32), "big") % Q for _ in range(300)]
    got = images(scl, scl.ec_mul_base(gtable, scalars_dev(scl, ks)))
    assert got == [ec_image(ec_mul(k, G)) for k in ks]


def test_elementwise_and_equality_on_the_fixture_identities(scl):
    """every identity of the fixture at n = 65 (tiled): P + Q, P + P through ADD, 2P, P - P = infinity, infinity as either
    operand, -P; operands under random projective coordinates; equality under rescaling; in place (dst == a)"""
    ids = golden("feldman")["identities"]
    n = 65
    pick = [ids[i % len(ids)] for i in range(n)]
    col = lambda key: [bytes.fromhex(c[key]) for c in pick]
    Pm, Qm = [ec_from_image(b) for b in col("P")], [ec_from_image(b) for b in col("Q")]
    assert any(p is None for p in Pm) and any(p == q for p, q in zip(Pm, Qm))
    flat_p, flat_q = points_dev(scl, Pm), points_dev(scl, Qm)
    inf = points_dev(scl, [None] * n)
    for a, b in ((flat_p, flat_q), (rescale(scl, flat_p, 1), rescale(scl, flat_q, 2))):
        assert images(scl, scl.ec_ew(scl.ADD, a, b)) == col("P+Q")
        assert images(scl, scl.ec_ew(scl.ADD, b, a)) == col("P+Q")
        assert images(scl, scl.ec_ew(scl.ADD, a, a)) == col("P+P")
        assert images(scl, scl.ec_ew(scl.EC_DBL, a)) == col("2P")
        assert images(scl, scl.ec_ew(scl.SUB, a, a)) == col("P-P") == [b"\x06" + bytes(64)] * n
        assert images(scl, scl.ec_ew(scl.ADD, a, inf)) == col("P+inf") == images(scl, scl.ec_ew(scl.ADD, inf, a))
        assert images(scl, scl.ec_ew(scl.NEG, a)) == col("-P")
        assert images(scl, scl.ec_ew(scl.SUB, a, b)) == [ec_image(ec_add(p, ec_neg(q))) for p, q in zip(Pm, Qm)]
        assert scl.ec_equal(a, flat_p).cpu().tolist() == [1] * n
        assert scl.ec_equal(a, b).cpu().tolist() == [int(c["P==Q"]) for c in pick]
        assert scl.ec_equal(a, scl.ec_ew(scl.NEG, a)).cpu().tolist() == [int(p is None) for p in Pm]
    work = rescale(scl, flat_p, 3)
    assert scl.ec_ew(scl.ADD, work, flat_q, out=work) is work
    assert images(scl, work) == col("P+Q")


@pytest.mark.parametrize("m", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 65])
def test_lincomb(scl, gtable, m, N):
    """sum_k lambda_k P[k][s] with lambda from {0, 1, q - 1, random}, a row of infinities, two equal rows (with lambda = 1 and
    q - 1 at m = 2 every sum is infinity), rows a pitch of N + 3 apart.  P[k][s] = a[k][s] G, so the sum is one known multiple
    of G: all N against mul_base (pinned to the model above), both ends against the model"""
    rng = np.random.default_rng(100 * m + N)
    rnd = lambda: int.from_bytes(rng.bytes(32), "big") % Q
    lam = {1: [rnd()], 2: [1, Q - 1], 5: [0, 1, Q - 1, rnd(), rnd()]}[m]
    a = [[rnd() for _ in range(N)] for _ in range(m)]
    if m == 2:
        a[1] = a[0]
    if m == 5:
        a[1] = [0] * N
        a[3] = a[2]
    rows = scl.ec_empty(m, N + 3)
    for k in range(m):
        scl.ec_mul_base(gtable, scalars_dev(scl, a[k]), out=rows[k, :N])
    points = rows[:, :N]
    if m > 1:
        points = torch.cat([points[:1], rescale(scl, points[1:].reshape(-1, 12), m).reshape(m - 1, N, 12)]).contiguous()
        rows[:, :N] = points
        points = rows[:, :N]
    got = images(scl, scl.ec_lincomb(points, scalars_dev(scl, lam)))
    total = [sum(l * a[k][s] for k, l in enumerate(lam)) % Q for s in range(N)]
    assert got == images(scl, scl.ec_mul_base(gtable, scalars_dev(scl, total)))
    for s in {0, N - 1}:
        assert got[s] == ec_image(ec_mul(total[s], G))
    if m == 2:
        assert got == [b"\x06" + bytes(64)] * N


def test_lincomb_over_more_rows_than_one_launch_recodes(scl):
    """m = 257: the kernel recodes 256 scalars a launch, the 257th row goes through a second launch that adds to dst.  Every
    row is G; the scalars are 1..256 and one random one in the last row, so the sum is one multiple of G by the model"""
    m, N = 257, 2
    r = int.from_bytes(np.random.default_rng(257).bytes(32), "big") % Q
    lam = list(range(1, m)) + [r]
    points = points_dev(scl, [G] * (m * N)).reshape(m, N, 12)
    got = images(scl, scl.ec_lincomb(points, scalars_dev(scl, lam)))
    assert got == [ec_image(ec_mul(sum(lam), G))] * N


def test_cxx_batch_forms_agree_with_the_per_secret_forms(scl, tmp_path):
    """tests/cxx/test_feldman_api --device: hip::Feldman (include/scl_hip/hip/feldman.h) over DeviceVector / ShareMatrix shares,
    commits and verifies 65 secrets of (10, 3) off one PRG; shares, commitments and verdicts (planted errors, a wrong index,
    summed sharings) equal those of ss::feldmanSecretShare / feldmanVerify secret by secret"""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run(["timeout", "-k", "10", "300", mirror_binary("feldman"), cases, "--device"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device: 65 secrets" in r.stdout and f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout


def test_wire_round_trip_and_flags(scl, gtable):
    """pack / unpack round trip with infinity among the points; 0x06 followed by garbage reads as infinity; an image with
    neither flag (compressed) raises its status byte and only its own; points with Z != 1 pack to the affine image"""
    _, want = fixed_scalars()
    raw = np.frombuffer(b"".join(want), dtype=np.uint8).copy().reshape(len(want), 65)
    pts, status = scl.ec_wire_unpack(torch.from_numpy(raw).cuda())
    assert not status.any() and images(scl, pts) == want
    assert images(scl, rescale(scl, pts, 9)) == want
    bad = raw.copy()
    bad[1, 0], bad[2, 0] = 0x03, 0x01  # infinity flag + garbage; a compressed image
    bad[3, 0] = 0x06
    bad[3, 1:] = 0xA5
    pts, status = scl.ec_wire_unpack(torch.from_numpy(bad).cuda())
    assert status.cpu().tolist() == [0, 0, 1] + [0] * (len(want) - 3)
    got = images(scl, pts)
    assert got[1] == got[3] == want[0] and got[4:] == want[4:]


@pytest.mark.parametrize("which", ["runs", "hom_runs"])
def test_feldman_commit_and_verify_reproduce_the_reference(scl, gtable, which):
    """the fixture's sharings -- (t, n) in {(0,1), (1,2), (3,10), (4,24)} with seed "feldman", and the two of "Feldman hom" off
    one PRG -- through scl_hip_shamir_share_prg over the scalar field: shares and commitments equal the reference's byte for
    byte, every party verifies, index 0 verifies the secret, the three tampered inputs give 0"""
    f = scl.SECP256K1_SCALAR
    for r in golden("feldman")[which]:
        t, n = r["t"], r["n"]
        secrets = scalars_dev(scl, [r["secret"]])
        shares = scl.shamir_share_prg(f, secrets, t, n, r["seed"].encode(), first_secret=r["first_secret"])
        assert scalars_host(scl, shares) == run_shares(r), (t, n)
        com = scl.feldman_commit(gtable, secrets, shares, t)
        assert [b.hex() for b in images(scl, com)] == r["commitments"], (t, n)
        assert scl.feldman_verify(gtable, secrets, com, scl.feldman_lambda(t, 0)).cpu().tolist() == [1]
        for p in range(n):
            assert scl.feldman_verify(gtable, shares[p], com, scl.feldman_lambda(t, p + 1)).cpu().tolist() == [1], (t, n, p)
        if t >= 1:
            last = shares[n - 1]
            off = scl.ew(f, scl.ADD, last, scalars_dev(scl, [1]))
            g_first = com.clone()
            g_first[0] = points_dev(scl, [G])
            assert scl.feldman_verify(gtable, off, com, scl.feldman_lambda(t, n)).cpu().tolist() == [0]
            assert scl.feldman_verify(gtable, last, g_first, scl.feldman_lambda(t, n)).cpu().tolist() == [0]
            assert scl.feldman_verify(gtable, last, com, scl.feldman_lambda(t, n - 1)).cpu().tolist() == [0]


def test_feldman_verify_finds_exactly_the_planted_errors(scl, gtable):
    """65 secrets of (10, 3), party 4's share altered at secrets 0 and 64: the verdicts are the complement of the planted set;
    the model agrees on the two ends and one in between"""
    f, N, t, n, p = scl.SECP256K1_SCALAR, 65, 3, 10, 4
    secrets = scl.vector_random(f, N, b"planted-secrets")
    shares = scl.shamir_share_prg(f, secrets, t, n, b"planted")
    com = scl.feldman_commit(gtable, secrets, shares, t)
    lam = scl.feldman_lambda(t, p + 1)
    assert scl.feldman_verify(gtable, shares[p], com, lam).cpu().tolist() == [1] * N
    mine = shares[p].clone()
    mine[0], mine[64] = shares[p][1], shares[p][63]
    assert scl.feldman_verify(gtable, mine, com, lam).cpu().tolist() == [0] + [1] * 63 + [0]
    got, sh = images(scl, com), scalars_host(scl, mine)
    for s in (0, 33, 64):
        assert feldman_verify(sh[s], [ec_from_image(got[k * N + s]) for k in range(t + 1)], p + 1) == (s == 33)


def test_feldman_is_additively_homomorphic(scl, gtable):
    """"Feldman hom" at N = 65: shares added over the field, commitments added through ec_ew(ADD); the sum of the secrets
    verifies at 0 and party 5's summed share at 6; the first sharing's share does not verify against the summed commitments"""
    f, N, t, n = scl.SECP256K1_SCALAR, 65, 4, 10
    s0, s1 = scl.vector_random(f, N, b"hom-s0"), scl.vector_random(f, N, b"hom-s1")
    a, b = scl.shamir_share_prg(f, s0, t, n, b"hom-a"), scl.shamir_share_prg(f, s1, t, n, b"hom-b")
    ca, cb = scl.feldman_commit(gtable, s0, a, t), scl.feldman_commit(gtable, s1, b, t)
    com2 = scl.ec_ew(scl.ADD, ca.reshape(-1, 12), cb.reshape(-1, 12)).reshape(t + 1, N, 12)
    sh2 = scl.ew(f, scl.ADD, a[5], b[5])
    assert scl.feldman_verify(gtable, scl.ew(f, scl.ADD, s0, s1), com2, scl.feldman_lambda(t, 0)).cpu().tolist() == [1] * N
    assert scl.feldman_verify(gtable, sh2, com2, scl.feldman_lambda(t, 6)).cpu().tolist() == [1] * N
    assert scl.feldman_verify(gtable, a[5], com2, scl.feldman_lambda(t, 6)).cpu().tolist() == [0] * N


def test_commit_and_verify_capture_into_a_hip_graph(scl, gtable):
    """commit then verify allocate nothing, copy nothing and do not synchronise: one capture, replayed on new shares"""
    f, N, t, n = scl.SECP256K1_SCALAR, 65, 3, 10
    secrets = scl.vector_random(f, N, b"graph-secrets")
    shares = scl.shamir_share_prg(f, secrets, t, n, b"graph-0")
    com, scratch = scl.ec_empty(t + 1, N), scl.ec_empty(2 * N)
    ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
    lam, mine = scl.feldman_lambda(t, 7), shares[6].clone()

    def step():
        scl.feldman_commit(gtable, secrets, shares, t, out=com)
        scl.feldman_verify(gtable, mine, com, lam, scratch=scratch, out=ok)

    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.synchronize()
    fresh = scl.shamir_share_prg(f, secrets, t, n, b"graph-1")
    shares.copy_(fresh)
    mine.copy_(fresh[6])
    mine[2] = fresh[5][2]
    ok.zero_()
    com.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1, 1, 0] + [1] * (N - 3)
    assert images(scl, com) == images(scl, scl.feldman_commit(gtable, secrets, fresh, t))


def test_error_paths(scl, gtable):
    """a misaligned buffer and a stride below the row length return their codes with a message; n == 0 returns at once"""
    lib, N = scl.lib, 4
    pts, sc = scl.ec_empty(N + 1), scalars_dev(scl, [1, 2, 3, 4, 5])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    size = C.c_size_t
    assert lib.scl_hip_ec_mul_base(pts.data_ptr() + 8, gtable.data_ptr(), sc.data_ptr(), size(N), st) == scl.ERR_BAD_ARG
    assert b"16-byte aligned" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_ew(scl.ADD, pts.data_ptr(), pts.data_ptr(), None, size(N), st) == scl.ERR_BAD_ARG
    assert b"NULL" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_ew(scl.MUL, pts.data_ptr(), pts.data_ptr(), pts.data_ptr(), size(N), st) == scl.ERR_BAD_ARG
    out = scl.ec_empty(N)
    assert lib.scl_hip_ec_lincomb(out.data_ptr(), pts.data_ptr(), size(N - 1), size(2), sc.data_ptr(), size(N), st) == scl.ERR_SIZE_MISMATCH
    assert b"row_stride < n" in lib.scl_hip_last_error()
    com = scl.ec_empty(2, N)
    assert lib.scl_hip_feldman_commit(com.data_ptr(), size(N - 1), gtable.data_ptr(), sc.data_ptr(), sc.data_ptr(), size(N), size(1),
                                      size(N), st) == scl.ERR_SIZE_MISMATCH
    assert b"commit_stride < N" in lib.scl_hip_last_error()
    inf = np.zeros(12, dtype=np.uint64)
    assert lib.scl_hip_ec_base_table(gtable.data_ptr(), inf.ctypes.data, st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ec_mul_base(None, None, None, size(0), st) == scl.OK
    assert lib.scl_hip_feldman_verify(None, None, None, size(0), size(3), None, None, None, size(0), st) == scl.OK
    torch.cuda.synchronize()
