"""ECDSA over secp256k1, the host half: the C++ mirror's util::ECDSA / util::Signature<ECDSA> (tests/cxx/test_ecdsa_api.cc) and
the functions under it (detail/secp256k1.hpp: rinv, ecdsa_conversion, pt_x_is, pt_mul_window) against what the REFERENCE computed
(tests/golden/golden_ecdsa.json), and the big-integer Python model of tests/secp256k1_model.py with its signing and
verification, which pins the same fixture by something that is neither the reference nor this code.  The model also checks the
kernels in tests/test_gpu_ecdsa.py.  Everything is exact."""
import hashlib
import subprocess

from cxx_support import mirror_binary
from secp256k1_model import (G, Q, conversion, digest_to_element, ec_from_image, ec_image, ec_mul, ecdsa_sign, ecdsa_verify, golden, h32,
                             sig_from_image, sig_image)
from secp256k1_model import write_ecdsa_cases as write_cases


def test_model_reproduces_the_reference_fixture():
    """every entry of the fixture through big-integer arithmetic: k P, the derived keys, every signature from its nonce byte
    for byte, conversionFunc, digestToElement at the six lengths, every honest verdict true and every tampered one false"""
    d = golden("ecdsa")
    ks = [int(k, 16) for k in d["scalars"]]
    assert ks[:9] == [0, 1, 2, 15, 16, 17, 2 ** 64, 2 ** 255, Q - 1] and len(ks) == 17
    pts = [ec_from_image(bytes.fromhex(m["P"])) for m in d["mul"]]
    assert pts[0] == ec_mul(5, G) and pts[3] is None and G not in pts
    for p, m in zip(pts, d["mul"]):
        assert [ec_image(ec_mul(k, p)).hex() for k in ks] == m["kP"]
    assert ec_image(ec_mul(int(d["derive"]["sk"], 16), G)).hex() == d["derive"]["pk"]
    s = d["sign"]
    sk, pk = int(s["sk"], 16), ec_from_image(bytes.fromhex(s["pk"]))
    assert pk == ec_mul(sk, G)
    dm, ds = bytes.fromhex(s["digest_message"]), bytes.fromhex(s["digest_small"])
    # update("message") of the reference takes the literal as a char[8] through its serializer: the terminating NUL is hashed
    assert dm == hashlib.sha256(b"message\0").digest() and ds == bytes([1, 2, 3])
    assert sig_image(*ecdsa_sign(sk, dm, int(s["nonce_message"], 16))) == s["sig_message"]
    assert sig_image(*ecdsa_sign(sk, ds, int(s["nonce_small"], 16))) == s["sig_small"]
    assert s["verify_message"] and ecdsa_verify(pk, *sig_from_image(s["sig_message"]), dm)
    assert s["verify_small"] and ecdsa_verify(pk, *sig_from_image(s["sig_small"]), ds)
    assert not s["verify_small_sig_on_message"] and not ecdsa_verify(pk, *sig_from_image(s["sig_small"]), dm)
    assert [len(g["digest"]) // 2 for g in d["signatures"]] == [0, 1, 31, 32, 33, 64] * 2
    for g in d["signatures"]:
        sk, pk, dg = int(g["sk"], 16), ec_from_image(bytes.fromhex(g["pk"])), bytes.fromhex(g["digest"])
        k, R = int(g["nonce"], 16), ec_from_image(bytes.fromhex(g["R"]))
        assert pk == ec_mul(sk, G) and R == ec_mul(k, G)
        assert h32(digest_to_element(dg)) == g["h"] and h32(conversion(R)) == g["conversion"]
        r, s_ = ecdsa_sign(sk, dg, k)
        assert sig_image(r, s_) == g["sig"]
        assert g["verify"] and ecdsa_verify(pk, r, s_, dg)
        assert not any(g["tampered"].values())
        other = bytes.fromhex(g["other_digest"])
        assert other == hashlib.sha256(dg).digest()
        assert not ecdsa_verify(pk, (r + 1) % Q, s_, dg) and not ecdsa_verify(pk, r, (s_ + 1) % Q, dg)
        assert not ecdsa_verify(pk, r, s_, other)
        assert not ecdsa_verify(ec_from_image(bytes.fromhex(g["other_pk"])), r, s_, dg)
        assert ec_from_image(bytes.fromhex(g["other_pk"])) == ec_mul(sk + 1, G)


def test_cxx_mirror_computes_what_the_reference_computed(tmp_path):
    """util::ECDSA of the mirror on every entry of the fixture -- Sign off the seed reproduces (r, s) byte for byte, Signature
    read / write round trips, digestToElement at the six lengths, verify of s = 0 throws --, pt_mul_window on the fixture's k P,
    rinv against pow(a, -1, q) for the edge scalars and 300 random ones (and rinv(0) = 0), ecdsa_conversion and pt_x_is on
    synthetic coordinates: X = (r + q) Z with r + q < p, X = r Z, X = (r + 1) Z, infinity, and r with r + q >= p"""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run([mirror_binary("ecdsa"), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout
