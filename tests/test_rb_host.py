"""Square roots and the random-bit finish, the host half: the Python model (tests/rb_support.py) pinned to what the REFERENCE's
math::details::sqrt produced over the secp256k1 prime (tests/golden/golden_rb.json), the model's own two routes held against each
other (inside the test of the host forms, not as a test of its own: alone it would say nothing about the library), and the stand-alone check of the host forms of detail/rb.hpp (tests/cxx/rb_host_check.cc) over all five prime fields --
Mont128 at 2^128 - 159 (s = 5) and at 2^127 - 1 (s = 1) -- against the fixture, the model and the identities, plain and under
the address and undefined-behaviour sanitizers.  Everything is exact.

THE FIXTURE'S ROOT IS NOT NORMALISED: the reference returns whichever root y^((p+1)/4) is, even or odd.  This project's canonical
root is the even one, so the reference's root r is replaced by p - r where r is odd before anything is compared."""
import json
import os
import subprocess

import rb_support as RBS
from cxx_support import SANITIZE, host_check, needed

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rb.json")
# (the program's name for the case, the tag, the modulus)
CASES = [("m61", RBS.M61, None), ("m127", RBS.M127, None), ("mont128_p0", RBS.MONT128, RBS.MONT_P0), ("mont128_p1", RBS.MONT128, RBS.MONT_P1),
         ("secp_scalar", RBS.SECP_SCALAR, None), ("secp_field", RBS.SECP_FIELD, None)]


def fixture():
    with open(GOLDEN) as fh:
        d = json.load(fh)["data"]
    assert d["field"] == "secp256k1_field" and len(d["cases"]) == 18
    return [(int(c["y"], 16), int(c["root"], 16)) for c in d["cases"]]          # FF::write is big-endian


def even(p, r):
    return p - r if r & 1 else r


def lines():
    """the cases file of rb_host_check: per field {0, 1, 4, p-1, p-4} and 64 seeded elements; the fixture under secp_field"""
    out = []
    for k, (name, f, mp) in enumerate(CASES):
        p = RBS.prime(f, mp or RBS.MONT_P0)
        values = [0, 1, 4, p - 1, p - 4] + RBS.seeded(p, 64, 1000 + k) + ([y for y, _ in fixture()] if f == RBS.SECP_FIELD else [])
        for a in values:
            root, status = RBS.model_sqrt(p, a)
            inv, _ = RBS.model_sqrt(p, a, RBS.INVERSE)
            out.append(f"{name} {a:x} {status} {root:x} {inv:x}")
    return out


def test_the_fixture_has_the_documented_shape():
    fx = fixture()
    assert fx[16] == (0, 0) and fx[17][0] == 1 and fx[17][1] in (1, RBS.SECP_P - 1)
    assert all(r * r % RBS.SECP_P == y for y, r in fx) and os.path.getsize(GOLDEN) < 8 * 1024
    assert any(r & 1 for _, r in fx) and any(not r & 1 for _, r in fx[:16]), "the reference returns roots of both parities"


def test_the_model_computes_the_fixtures_roots():
    """the reference's root, normalised to the even one, is the model's; the odd flag gives the other one"""
    p = RBS.SECP_P
    for y, r in fixture():
        want = (0, RBS.ZERO) if y == 0 else (even(p, r), RBS.OK_STATUS)
        assert RBS.model_sqrt(p, y) == want, hex(y)
        if y:
            assert RBS.model_sqrt(p, y, RBS.ODD_ROOT) == (p - even(p, r), RBS.OK_STATUS)


def model_self_check(name, f, mp):
    """the model against itself, before the host forms are held against it: the split p - 1 = 2^s q; Tonelli-Shanks gives a root
    wherever Euler's criterion says there is one (where p = 3 mod 4 it is held against pow); the root is even, its inverse is its
    inverse; about half of the seeded elements are residues; the bit of the even root is 1, of the odd root 0, of a flagged
    column 0"""
    p = RBS.prime(f, mp or RBS.MONT_P0)
    s, q = RBS.split(p)
    assert (p - 1) == q << s and q & 1 and s == {"m61": 1, "m127": 1, "mont128_p0": 5, "mont128_p1": 1, "secp_scalar": 6, "secp_field": 1}[name]
    values = [1, 4, p - 1, p - 4] + RBS.seeded(p, 64, 1000 + [c[0] for c in CASES].index(name))
    residues = 0
    for a in values:
        root, st = RBS.model_sqrt(p, a)
        assert st == (RBS.OK_STATUS if RBS.is_residue(p, a) else RBS.NONRESIDUE)
        if st:
            assert root == 0
            continue
        residues += 1
        t = RBS.tonelli_shanks(p, a)
        assert t * t % p == a and root in (t, p - t) and root % 2 == 0 and root * RBS.model_sqrt(p, a, RBS.INVERSE)[0] % p == 1
        b, status = RBS.model_bits(p, [a, a, 0], [[root, p - root, 5]])
        assert b == [[1, 0, 0]] and status == [0, 0, RBS.ZERO]
    assert 20 <= residues <= 52, residues
    assert RBS.model_sqrt(p, 0) == (0, RBS.ZERO) and RBS.model_sqrt(p, 0, RBS.INVERSE | RBS.ODD_ROOT) == (0, RBS.ZERO)


def test_the_host_forms_equal_the_fixture_the_model_and_the_identities(tmp_path):
    """rb_sqrt_one, rb_bit_factor, rb_bit_one and rb_make_params of detail/rb.hpp, every prime field, both Mont128 moduli; the
    model they are held against is checked against itself first (model_self_check)"""
    for case in CASES:
        model_self_check(*case)
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines()) + "\n")
    host_check(tmp_path, "rb_host_check.cc", "rb_host_check", ("-w", "-O2"), args=(str(cases),))


def test_the_host_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no read past the window table"""
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines()) + "\n")
    assert "runtime error" not in host_check(tmp_path, "rb_host_check.cc", "rb_host_check_san", ("-w",) + SANITIZE, args=(str(cases),))


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_mirrors_host_forms():
    """tests/cxx/test_rb_api.cc --host: math::sqrt and ss::randomBitFinish over the five prime fields -- root^2 == a, the even
    root's image is even, the odd root is its negative, a non-residue throws, the bit of the even root is 1 and of the odd root 0"""
    exe = RBS.rb_api_binary()
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    dynamic = needed(exe)
    assert "libscl_hip_rb.so" in dynamic and "libscl_hip.so" in dynamic
