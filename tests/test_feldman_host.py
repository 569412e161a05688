"""Feldman VSS, the host half: the C++ mirror's math::EC<ec::Secp256k1> and ss::feldman* (tests/cxx/test_feldman_api.cc) against
what the REFERENCE computed (tests/golden/golden_feldman.json), and an independent Python model (tests/secp256k1_model.py) -- big-integer affine
secp256k1 and Lagrange interpolation over the group order -- that pins the same fixture by something that is neither the reference nor
this code.  The model also checks the kernels in tests/test_gpu_feldman.py."""
import subprocess

from cxx_support import ROOT, mirror_binary
from secp256k1_model import G, Q, ec_add, ec_from_image, ec_image, ec_mul, ec_neg, feldman_verify, golden, run_commitments, run_shares
from secp256k1_model import write_feldman_cases as write_cases


def test_model_reproduces_the_reference_fixture():
    """every entry of the fixture through big-integer affine arithmetic: multiples of G, the identities, the commitments and
    the verdicts (the three tampered inputs false)"""
    d = golden("feldman")
    assert ec_image(G).hex() == d["G"]
    ks = [int(m["k"], 16) for m in d["multiples"]]
    assert ks[:10] == [0, 1, 2, 3, 15, 16, 17, 2 ** 64, 2 ** 255, Q - 1] and len(ks) == 18
    for k, m in zip(ks, d["multiples"]):
        assert ec_image(ec_mul(k, G)).hex() == m["P"], hex(k)
    for i in d["identities"]:
        a, b = ec_from_image(bytes.fromhex(i["P"])), ec_from_image(bytes.fromhex(i["Q"]))
        assert ec_image(ec_add(a, b)).hex() == i["P+Q"]
        assert ec_image(ec_add(a, a)).hex() == i["P+P"] == i["2P"]
        assert ec_image(None).hex() == i["P-P"]
        assert ec_image(a).hex() == i["P+inf"]
        assert ec_image(ec_neg(a)).hex() == i["-P"]
        assert i["P+P==2P"] and i["sum==normalized_sum"] and i["P==Q"] == (a == b)
    assert [(r["t"], r["n"]) for r in d["runs"]] == [(0, 1), (1, 2), (3, 10), (4, 24)]
    for r in d["runs"] + d["hom_runs"]:
        t, n, shares, com = r["t"], r["n"], run_shares(r), run_commitments(r)
        assert com == [ec_mul(s, G) for s in [r["secret"]] + shares[:t]]
        assert r["verify_secret_at_0"] and feldman_verify(r["secret"], com, 0)
        # the model's own walk over the parties is kept short: both ends and one in the middle
        assert all(r["verify_party"]) and len(r["verify_party"]) == n
        for p in sorted({0, n // 2, n - 1}):
            assert feldman_verify(shares[p], com, p + 1)
        if t >= 1:
            assert not any(r["tampered"].values()) and len(r["tampered"]) == 3
            assert not feldman_verify((shares[n - 1] + 1) % Q, com, n)
            assert not feldman_verify(shares[n - 1], [G] + com[1:], n)
            assert not feldman_verify(shares[n - 1], com, n - 1)
    a, b = d["hom_runs"]
    com2 = [ec_add(x, y) for x, y in zip(run_commitments(a), run_commitments(b))]
    assert [ec_image(c).hex() for c in com2] == d["hom"]["commitments"]
    assert d["hom"]["verify_sum_at_0"] and feldman_verify(123 + 44, com2, 0)
    assert d["hom"]["verify_share_5_at_6"] and feldman_verify((run_shares(a)[5] + run_shares(b)[5]) % Q, com2, 6)


def test_cxx_mirror_computes_what_the_reference_computed(tmp_path):
    """both cases of the reference's test_feldman.cc, the uncompressed cases of its test_secp256k1.cc, and every entry of the
    fixture through math::EC and ss::feldman* of the mirror"""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run([mirror_binary("feldman"), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout


def test_number_scalars_and_compressed_images_do_not_compile(tmp_path):
    """what the mirror does not build is a compile error, not something else: write(dest, true) and a scalar that is not a
    ScalarField element, Vector<EC>::multiplyEntryWise; the same file with the two lines taken out compiles"""
    head = '#include "scl_hip/scl.h"\nusing EC = scl::math::EC<scl::math::ec::Secp256k1>;\nint main() {\n  unsigned char b[65];\n  EC g = EC::generator();\n'
    for body, ok in (("  g.write(b, false);\n", True), ("  g.write(b, true);\n", False), ("  bool c = false; g.write(b, c);\n", False),
                     ("  g = g * 3;\n", False),
                     ("  scl::math::Vector<EC> v{g}; v = v.add(v);\n", True), ("  scl::math::Vector<EC> v{g}; v = v.multiplyEntryWise(v);\n", False), ("  g = g * EC::Field(3);\n", False)):
        src = tmp_path / "probe.cc"
        src.write_text(head + body + "  return b[0] == 4 ? 0 : 1;\n}\n")
        r = subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wno-unknown-pragmas", f"-I{ROOT}/include", str(src)],
                           capture_output=True, text=True)
        assert (r.returncode == 0) == ok, body + r.stderr[-2000:]
