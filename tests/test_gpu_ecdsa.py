"""Batched ECDSA over secp256k1 on the GPU: scl_hip_ec_mul and scl_hip_ecdsa_* (csrc/ecdsa_unit.hip) against what the reference
computed (tests/golden/golden_ecdsa.json) and against the big-integer Python model of tests/secp256k1_model.py (pinned by tests/test_ecdsa_host.py to
that fixture) -- never against the library.  Everything is exact: every comparison is byte equality of wire images, of scalar
images or of verdict bytes.  The model's work is kept to a few hundred scalar multiplications over the whole file."""
import ctypes as C
import functools
import hashlib
import subprocess

import numpy as np
import pytest
import torch

from cxx_support import mirror_binary
from gpu_support import images, limbs_of, points_dev, rescale, scalars_dev
from secp256k1_model import G, P, Q, conversion, digest_row, ec_from_image, ec_image, ec_mul, ecdsa_sign, ecdsa_verify, golden, sig_from_image
from secp256k1_model import write_ecdsa_cases as write_cases

pytestmark = pytest.mark.gpu
R = 1 << 256
COUNTS = [1, 63, 64, 65, 300]
INF = b"\x06" + bytes(64)


@pytest.fixture(scope="module")
def scl():
    import scl_amd
    assert torch.cuda.is_available()
    return scl_amd


@pytest.fixture(scope="module")
def gtable(scl):
    return scl.ec_base_table()


def scalar_images(scl, t: torch.Tensor):
    """SECP256K1_SCALAR elements -> their 32-byte FF::write images (the wire image behind its 4-byte count)"""
    raw = scl.wire_pack(scl.SECP256K1_SCALAR, t.reshape(-1, 4).contiguous()).cpu().numpy()[4:].tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(len(raw) // 32)]


def sig_images(scl, sig: torch.Tensor):
    """signatures [n][8] -> their 64-byte Signature::write images"""
    im = scalar_images(scl, sig)
    return [im[2 * i] + im[2 * i + 1] for i in range(len(im) // 2)]


def sigs_dev(scl, pairs) -> torch.Tensor:
    return scalars_dev(scl, [v for rs in pairs for v in rs]).reshape(len(pairs), 8)


def digests_dev(rows) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(b"".join(digest_row(d) for d in rows), dtype=np.uint8).copy().reshape(len(rows), 32)).cuda()


def raw_points(scl, coords) -> torch.Tensor:
    """(X, Y, Z) plain integers -> device points, on the curve or not"""
    return scl.to_device(np.array([limbs_of(c % P * R % P) for xyz in coords for c in xyz], dtype=np.uint64).reshape(len(coords), 12))


def tile(items, n):
    return [items[i % len(items)] for i in range(n)]


# ---- the cases, computed once ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mul_cases():
    """(P, k, image of k P): the fixture's -- four points, infinity among them, seventeen scalars --, then by the model digits 0
    and 15 in windows 0, 1 and 63 of a scalar that is all ones elsewhere"""
    d = golden("ecdsa")
    ks = [int(k, 16) for k in d["scalars"]]
    cases = [(ec_from_image(bytes.fromhex(m["P"])), k, bytes.fromhex(kp)) for m in d["mul"] for k, kp in zip(ks, m["kP"])]
    p = cases[17][0]
    ones = 2 ** 252 - 1
    for k in (ones & ~15, ones & ~0xF0, ones, 15, 15 << 4, 15 << 252):
        assert k < Q
        cases.append((p, k, ec_image(ec_mul(k, p))))
    return cases


@pytest.fixture(scope="module")
def sign_cases():
    """the fixture's fourteen signatures: (sk, nonce, digest, signature image)"""
    d = golden("ecdsa")
    s = d["sign"]
    out = [(int(s["sk"], 16), int(s["nonce_message"], 16), bytes.fromhex(s["digest_message"]), bytes.fromhex(s["sig_message"])),
           (int(s["sk"], 16), int(s["nonce_small"], 16), bytes.fromhex(s["digest_small"]), bytes.fromhex(s["sig_small"]))]
    out += [(int(g["sk"], 16), int(g["nonce"], 16), bytes.fromhex(g["digest"]), bytes.fromhex(g["sig"])) for g in d["signatures"]]
    return out


@pytest.fixture(scope="module")
def verify_cases():
    """(pk, (r, s), digest, verdict): the fixture's honest and tampered lanes in the order honest, r + 1, s + 1, other digest,
    other key -- so that accepted and rejected lanes alternate --, the reference's three, and by the model: s = 0 (2), r = 0,
    the forgery whose R is infinity, and u1 G == u2 Q (the addition is a doubling) both accepted and rejected"""
    d = golden("ecdsa")
    out = []
    for g in d["signatures"]:
        pk, other_pk = ec_from_image(bytes.fromhex(g["pk"])), ec_from_image(bytes.fromhex(g["other_pk"]))
        r, s = sig_from_image(g["sig"])
        dg, t = bytes.fromhex(g["digest"]), g["tampered"]
        out += [(pk, (r, s), dg, int(g["verify"])), (pk, ((r + 1) % Q, s), dg, int(t["r_plus_1"])), (pk, (r, (s + 1) % Q), dg, int(t["s_plus_1"])),
                (pk, (r, s), bytes.fromhex(g["other_digest"]), int(t["other_digest"])), (other_pk, (r, s), dg, int(t["other_key"]))]
    out += list(one_signer_cases())
    assert sorted({c[3] for c in out}) == [0, 1, 2]
    return out


@functools.lru_cache(maxsize=None)
def one_signer_cases():
    """lanes of ONE key (the reference's "ECDSA sign" key): its three verdicts and the model's special cases"""
    s = golden("ecdsa")["sign"]
    sk, pk = int(s["sk"], 16), ec_from_image(bytes.fromhex(s["pk"]))
    dm, ds = bytes.fromhex(s["digest_message"]), bytes.fromhex(s["digest_small"])
    r, sg = sig_from_image(s["sig_message"])
    out = [(pk, (r, sg), dm, int(s["verify_message"])), (pk, sig_from_image(s["sig_small"]), dm, int(s["verify_small_sig_on_message"])),
           (pk, sig_from_image(s["sig_small"]), ds, int(s["verify_small"]))]
    out.append((pk, (r, 0), dm, 2))
    out.append((pk, (0, sg), dm, 0))
    # R = (h + r sk) / s G is infinity for h = -r sk: rejected whatever r and s are
    h = -r * sk % Q
    out.append((pk, (r, sg), h.to_bytes(32, "big"), 0))
    # h = r sk makes u1 G and u2 Q the same point, R = 2 r sk / s G; with s = 2 r sk / k and r = C(k G) that is k G: accepted
    k = 0x1234567 * sk % Q
    rk = conversion(ec_mul(k, G))
    s2 = 2 * rk * sk * pow(k, -1, Q) % Q
    h2 = (rk * sk % Q).to_bytes(32, "big")
    assert ecdsa_verify(pk, rk, s2, h2) and not ecdsa_verify(pk, rk, (s2 + 1) % Q, h2)
    out += [(pk, (rk, s2), h2, 1), (pk, (rk, (s2 + 1) % Q), h2, 0)]
    return tuple(out)


# ---- ec_mul -----------------------------------------------------------------------------------------------------------------
def test_mul_fixture_digits_and_grid_tails(scl, mul_cases):
    """k P for the fixture's points (5 G, a random multiple, a sum, infinity) and scalars (0, 1, 2, 15, 16, 17, 2^64, 2^255,
    q - 1, eight random) and digits 0 and 15 in windows 0, 1 and 63, tiled over counts around the block size; P given flat and
    under random projective coordinates; k = 0 and P = infinity give infinity"""
    assert sum(1 for p, k, w in mul_cases if w == INF) >= 17 + 3
    for n in COUNTS:
        c = tile(mul_cases, n)
        pts, ks = points_dev(scl, [p for p, _, _ in c]), scalars_dev(scl, [k for _, k, _ in c])
        assert images(scl, scl.ec_mul(pts, ks)) == [w for _, _, w in c], n
        assert images(scl, scl.ec_mul(rescale(scl, pts, n), ks)) == [w for _, _, w in c], n


def test_mul_lanes_differ_in_one_window(scl, mul_cases):
    """lane i multiplies by (i mod 16) * 16^5: sixteen different digits side by side in window 5 and zeros everywhere else --
    what a branch that is uniform over the wave would get wrong"""
    p = mul_cases[17][0]
    want = [ec_image(ec_mul(d << 20, p)) for d in range(16)]
    n = 130
    got = images(scl, scl.ec_mul(points_dev(scl, [p] * n), scalars_dev(scl, [(i % 16) << 20 for i in range(n)])))
    assert got == tile(want, n)


def test_mul_random_pairs_in_place(scl, gtable):
    """300 random (k, P) pairs, P = a G with Z != 1, against the model's (k a) G; dst == points"""
    rng = np.random.default_rng(31)
    rnd = lambda: int.from_bytes(rng.bytes(32), "big") % Q
    a, k = [rnd() for _ in range(300)], [rnd() for _ in range(300)]
    pts = rescale(scl, scl.ec_mul_base(gtable, scalars_dev(scl, a)), 32)
    assert scl.ec_mul(pts, scalars_dev(scl, k), out=pts) is pts
    assert images(scl, pts) == [ec_image(ec_mul(x * y % Q, G)) for x, y in zip(a, k)]


# ---- ecdsa_conversion -------------------------------------------------------------------------------------------------------
def test_conversion(scl):
    """the fixture's conversionFunc(R); off-curve coordinates with X = q + 5 -> 5, flat and under a non-unit Z (x >= q comes
    from no signature); X = p - 1 -> p - 1 - q; infinity -> 0"""
    sigs = golden("ecdsa")["signatures"]
    pts = points_dev(scl, [ec_from_image(bytes.fromhex(g["R"])) for g in sigs] + [None])
    want = [bytes.fromhex(g["conversion"]) for g in sigs] + [bytes(32)]
    assert scalar_images(scl, scl.ecdsa_conversion(pts)) == want
    assert scalar_images(scl, scl.ecdsa_conversion(rescale(scl, pts, 5))) == want
    z = 0xC0FFEE * R % P + 3
    syn = raw_points(scl, [(Q + 5, 1, 1), ((Q + 5) * z, 1, z), (P - 1, 1, 1), ((P - 1) * z, 9, z), (7, 1, 0)] * 13)
    assert scalar_images(scl, scl.ecdsa_conversion(syn)) == [v.to_bytes(32, "big") for v in (5, 5, P - 1 - Q, P - 1 - Q, 0)] * 13


# ---- ecdsa_sign -------------------------------------------------------------------------------------------------------------
def test_sign_reproduces_the_reference(scl, gtable, sign_cases):
    """the fixture's fourteen signatures from their nonces, a key per lane, tiled over the counts: (r, s) byte for byte"""
    for n in COUNTS:
        c = tile(sign_cases, n)
        status = scl.ew_status_buffer()
        sig = scl.ecdsa_sign(gtable, scalars_dev(scl, [x[0] for x in c]), scalars_dev(scl, [x[1] for x in c]),
                             digests_dev([x[2] for x in c]), status=status)
        assert sig_images(scl, sig) == [x[3] for x in c], n
        assert status.item() == 0


def test_sign_with_one_key_for_all_lanes(scl, gtable, sign_cases):
    """stride 0: the reference's two signatures are one key's; 65 lanes of them off one [1][4] key"""
    c = tile(sign_cases[:2], 65)
    assert c[0][0] == c[1][0]
    sig = scl.ecdsa_sign(gtable, scalars_dev(scl, [c[0][0]]), scalars_dev(scl, [x[1] for x in c]), digests_dev([x[2] for x in c]))
    assert sig_images(scl, sig) == [x[3] for x in c]


def test_sign_zero_nonce_raises_the_status_word(scl, gtable, sign_cases):
    """k = 0 in ONE lane of 65: (0, 0) there, the status word set, every other lane as without it"""
    c = tile(sign_cases, 65)
    nonces = [x[1] for x in c]
    nonces[37] = 0
    status = scl.ew_status_buffer()
    sig = scl.ecdsa_sign(gtable, scalars_dev(scl, [x[0] for x in c]), scalars_dev(scl, nonces), digests_dev([x[2] for x in c]), status=status)
    want = [x[3] for x in c]
    want[37] = bytes(64)
    assert sig_images(scl, sig) == want
    assert status.item() == 1
    assert scl.to_host(sig)[37].tolist() == [0] * 8


# ---- ecdsa_verify, ecdsa_verify_base ----------------------------------------------------------------------------------------
def test_verify_reproduces_every_verdict(scl, gtable, verify_cases):
    """every verdict of the fixture, honest and tampered lanes interleaved, and the model's special lanes (s = 0 -> 2 there only,
    r = 0, R = infinity, the doubling), a key per lane, tiled over the counts; then the keys under other projective coordinates"""
    for n in COUNTS:
        c = tile(verify_cases, n)
        pk, sig, dg = points_dev(scl, [x[0] for x in c]), sigs_dev(scl, [x[1] for x in c]), digests_dev([x[2] for x in c])
        assert scl.ecdsa_verify(gtable, pk, sig, dg).cpu().tolist() == [x[3] for x in c], n
        assert scl.ecdsa_verify(gtable, rescale(scl, pk, n), sig, dg).cpu().tolist() == [x[3] for x in c], n


def test_verify_one_key_and_the_key_table(scl, gtable):
    """one public key for all lanes (stride 0) and scl_hip_ecdsa_verify_base with that key's window table: the same verdicts,
    lane for lane, as the model's / the reference's; the key also under other coordinates"""
    cases = one_signer_cases()
    pk = points_dev(scl, [cases[0][0]])
    qtable = scl.ec_base_table(scl.to_host(pk)[0])
    for n in (1, 65, 300):
        c = tile(cases, n)
        sig, dg = sigs_dev(scl, [x[1] for x in c]), digests_dev([x[2] for x in c])
        want = [x[3] for x in c]
        assert scl.ecdsa_verify(gtable, pk, sig, dg).cpu().tolist() == want, n
        assert scl.ecdsa_verify(gtable, rescale(scl, pk, 3), sig, dg).cpu().tolist() == want, n
        assert scl.ecdsa_verify_base(gtable, qtable, sig, dg).cpu().tolist() == want, n


def test_verify_base_reproduces_every_fixture_verdict(scl, gtable, verify_cases):
    """the fixture's sixty lanes are twelve keys' five each -- honest, r + 1, s + 1, other digest under the key, and the honest
    signature under the OTHER key: verify_base with the key's table (and the other key's for the fifth lane) gives the
    fixture's verdicts, all digest lengths, and agrees with verify lane for lane; 24 tables"""
    for j in range(12):
        c = verify_cases[5 * j:5 * j + 5]
        assert [x[3] for x in c] == [1, 0, 0, 0, 0] and c[4][0] != c[0][0] and all(x[0] == c[0][0] for x in c[:4])
        for lanes in (c[:4], c[4:]):
            pk = points_dev(scl, [lanes[0][0]])
            qtable = scl.ec_base_table(scl.to_host(pk)[0])
            sig, dg = sigs_dev(scl, [x[1] for x in lanes]), digests_dev([x[2] for x in lanes])
            want = [x[3] for x in lanes]
            assert scl.ecdsa_verify_base(gtable, qtable, sig, dg).cpu().tolist() == want, j
            assert scl.ecdsa_verify(gtable, pk, sig, dg).cpu().tolist() == want, j


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_hash_sign_verify_on_the_device_and_in_a_graph(scl, gtable):
    """messages -> scl_hip_sha256 -> sign -> verify, nothing leaving the device: digests equal hashlib's, signatures the
    model's on two lanes, verdicts all 1; the same chain captured once into a graph and replayed on new messages gives the bytes
    of the plain calls"""
    n, mlen = 65, 40
    rng = np.random.default_rng(77)
    rnd = lambda: int.from_bytes(rng.bytes(32), "big") % (Q - 1) + 1
    sk, nonces = [rnd() for _ in range(n)], [rnd() for _ in range(n)]
    dsk, dk = scalars_dev(scl, sk), scalars_dev(scl, nonces)
    pk = scl.ec_mul_base(gtable, dsk)
    msgs = torch.from_numpy(rng.integers(0, 256, (n, mlen), dtype=np.uint8)).cuda()
    dg = scl.sha256(msgs)
    host = msgs.cpu().numpy()
    assert [bytes(r) for r in dg.cpu().numpy()] == [hashlib.sha256(host[i].tobytes()).digest() for i in range(n)]
    sig = scl.ecdsa_sign(gtable, dsk, dk, dg)
    for i in (0, 64):
        r, s = ecdsa_sign(sk[i], hashlib.sha256(host[i].tobytes()).digest(), nonces[i])
        assert sig_images(scl, sig[i:i + 1]) == [r.to_bytes(32, "big") + s.to_bytes(32, "big")]
    assert scl.ecdsa_verify(gtable, pk, sig, dg).cpu().tolist() == [1] * n

    dg2 = torch.empty(n, 32, dtype=torch.uint8, device="cuda")
    sig2 = torch.empty(n, 8, dtype=torch.int64, device="cuda")
    ok2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    scratch = scl.ec_mul_scratch(n)
    st, size = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_size_t

    def step():  # one chain on one stream: no parallel branches
        assert scl.lib.scl_hip_sha256(dg2.data_ptr(), msgs.data_ptr(), size(mlen), size(mlen), size(n), st()) == scl.OK
        scl.ecdsa_sign(gtable, dsk, dk, dg2, out=sig2)
        scl.ecdsa_verify(gtable, pk, sig2, dg2, scratch=scratch, out=ok2)

    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.synchronize()
    assert torch.equal(sig2, sig) and torch.equal(dg2, dg)
    msgs.copy_(torch.from_numpy(rng.integers(0, 256, (n, mlen), dtype=np.uint8)).cuda())
    ok2.zero_()
    sig2.zero_()
    g.replay()
    torch.cuda.synchronize()
    fresh = scl.sha256(msgs)
    assert torch.equal(dg2, fresh) and not torch.equal(fresh, dg)
    assert torch.equal(sig2, scl.ecdsa_sign(gtable, dsk, dk, fresh))
    assert ok2.cpu().tolist() == [1] * n


def test_cxx_batch_forms_agree_with_the_per_signature_forms(scl, tmp_path):
    """tests/cxx/test_ecdsa_api --device: hip::Ecdsa (include/scl_hip/hip/ecdsa.h) derives, signs, verifies (per-lane keys, one
    key, the key's table) and converts 65 signatures; results equal util::ECDSA's, signature by signature, planted errors and
    a zero nonce included"""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run(["timeout", "-k", "10", "300", mirror_binary("ecdsa"), cases, "--device"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device: 65 signatures" in r.stdout and f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout


def test_error_paths(scl, gtable):
    """NULL, a misaligned buffer and a stride that is neither 0 nor 1 return their codes with a message; n == 0 returns at once;
    the scratch size is 16 points a slot, whole blocks, capped; a short verdict buffer raises"""
    lib, N = scl.lib, 4
    size = C.c_size_t
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.scl_hip_ec_mul_scratch_bytes(size(1)) == lib.scl_hip_ec_mul_scratch_bytes(size(64)) == 64 * 16 * 96
    assert lib.scl_hip_ec_mul_scratch_bytes(size(65)) == 128 * 16 * 96
    assert lib.scl_hip_ec_mul_scratch_bytes(size(10 ** 9)) == lib.scl_hip_ec_mul_scratch_bytes(size(10 ** 8))
    pts, sc = scl.ec_empty(N + 1), scalars_dev(scl, [1, 2, 3, 4, 5])
    scratch, sig = scl.ec_mul_scratch(N), sigs_dev(scl, [(1, 1)] * N)
    dg, ok = digests_dev([b""] * N), torch.zeros(N, dtype=torch.uint8, device="cuda")
    assert lib.scl_hip_ec_mul(pts.data_ptr() + 8, pts.data_ptr(), sc.data_ptr(), scratch.data_ptr(), size(N), st) == scl.ERR_BAD_ARG
    assert b"16-byte aligned" in lib.scl_hip_last_error()
    assert lib.scl_hip_ec_mul(pts.data_ptr(), pts.data_ptr(), sc.data_ptr(), None, size(N), st) == scl.ERR_BAD_ARG
    assert b"NULL" in lib.scl_hip_last_error()
    assert lib.scl_hip_ecdsa_verify(ok.data_ptr(), sig.data_ptr(), dg.data_ptr(), pts.data_ptr(), size(2), gtable.data_ptr(),
                                    scratch.data_ptr(), size(N), st) == scl.ERR_BAD_ARG
    assert b"pk_stride" in lib.scl_hip_last_error()
    assert lib.scl_hip_ecdsa_sign(sig.data_ptr(), gtable.data_ptr(), sc.data_ptr(), size(3), sc.data_ptr(), dg.data_ptr(), None, size(N),
                                  st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ecdsa_verify_base(ok.data_ptr(), sig.data_ptr(), dg.data_ptr(), None, gtable.data_ptr(), size(N), st) == scl.ERR_BAD_ARG
    assert lib.scl_hip_ecdsa_conversion(sc.data_ptr(), pts.data_ptr() + 8, size(N), st) == scl.ERR_BAD_ARG
    for fn, nargs in ((lib.scl_hip_ec_mul, 4), (lib.scl_hip_ecdsa_conversion, 2)):
        assert fn(*([None] * nargs), size(0), st) == scl.OK
    assert lib.scl_hip_ecdsa_verify(None, None, None, None, size(0), None, None, size(0), st) == scl.OK
    assert lib.scl_hip_ecdsa_sign(None, None, None, size(0), None, None, None, size(0), st) == scl.OK
    assert lib.scl_hip_ecdsa_verify_base(None, None, None, None, None, size(0), st) == scl.OK
    assert scl.lib.scl_hip_abi_version() == 2
    # a verdict buffer of the caller's that is too short, or not bytes, is refused before a pointer crosses the boundary
    pk = scl.ec_empty(1)
    for bad in (ok[:N - 1], torch.zeros(N, dtype=torch.int32, device="cuda")):
        with pytest.raises(scl.SclError):
            scl.ecdsa_verify(gtable, pk, sig, dg, out=bad)
        with pytest.raises(scl.SclError):
            scl.ecdsa_verify_base(gtable, gtable, sig, dg, out=bad)
    torch.cuda.synchronize()
