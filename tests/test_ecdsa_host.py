"""ECDSA over secp256k1, the host half: the C++ mirror's util::ECDSA / util::Signature<ECDSA> (tests/cxx/test_ecdsa_api.cc) and
the functions under it (detail/secp256k1.hpp: rinv, ecdsa_conversion, pt_x_is, pt_mul_window) against what the REFERENCE computed
(tests/golden/golden_ecdsa.json), and the big-integer Python model of tests/test_feldman_host.py extended by signing and
verification, which pins the same fixture by something that is neither the reference nor this code.  The model also checks the
kernels in tests/test_gpu_ecdsa.py.  Everything is exact."""
import hashlib
import json
import os
import random
import subprocess

from test_feldman_host import G, P, Q, ec_add, ec_from_image, ec_image, ec_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_ecdsa.json")


# ---- the model (SEC 1, sections 4.1.3 and 4.1.4, without the range checks the reference does not make) -------------------------
def digest_row(digest: bytes) -> bytes:
    """the 32 bytes digestToElement reads: a short digest fills the FRONT of a zeroed buffer, a long one gives its first 32"""
    return digest[:32] + bytes(32 - min(len(digest), 32))


def digest_to_element(digest: bytes) -> int:
    return int.from_bytes(digest_row(digest), "big") % Q


def conversion(R) -> int:
    return 0 if R is None else R[0] % Q


def ecdsa_sign(sk: int, digest: bytes, k: int):
    r = conversion(ec_mul(k, G))
    return r, pow(k, -1, Q) * (digest_to_element(digest) + sk * r) % Q


def ecdsa_verify(pk, r: int, s: int, digest: bytes) -> bool:
    """s != 0 (the reference throws there)"""
    si = pow(s, -1, Q)
    R = ec_add(ec_mul(digest_to_element(digest) * si % Q, G), ec_mul(r * si % Q, pk))
    return R is not None and conversion(R) == r


def sig_image(r: int, s: int) -> str:
    return (r.to_bytes(32, "big") + s.to_bytes(32, "big")).hex()


def sig_from_image(h: str):
    b = bytes.fromhex(h)
    assert len(b) == 64
    return int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["data"]


def ecdsa_binary():
    """tests/cxx/test_ecdsa_api.cc compiled against the mirror (build() leaves it in place; rebuilt here when stale)"""
    src, exe = os.path.join(CXX, "test_ecdsa_api.cc"), os.path.join(CXX, "_build", "test_ecdsa_api")
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    newest = max(os.path.getmtime(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(newest, os.path.getmtime(src)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{lib}", "-lscl_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def h32(v: int) -> str:
    return v.to_bytes(32, "big").hex()


EDGE_SCALARS = [1, 2, 3, 15, 16, 17, 2 ** 64, 2 ** 127, 2 ** 128 - 1, 2 ** 128, 2 ** 255, Q - 2, Q - 1, (Q + 1) // 2]


def synthetic_cases():
    """conv / xis lines on coordinates no signature produces.  x(R) >= q has density 2^-128 among points, so the second
    comparison of pt_x_is (x = r + q, possible only for r < p - q) is reached this way alone"""
    rng = random.Random(7)
    lines = []
    z = rng.randrange(2, P)
    for Z in (1, z):
        lines.append(f"conv {h32((Q + 5) * Z % P)} {h32(Z)} {h32(5)}")           # X = q + 5 -> 5
        lines.append(f"conv {h32(5 * Z % P)} {h32(Z)} {h32(5)}")
        lines.append(f"conv {h32((Q - 1) * Z % P)} {h32(Z)} {h32(Q - 1)}")
        lines.append(f"conv {h32((P - 1) * Z % P)} {h32(Z)} {h32(P - 1 - Q)}")   # the largest x
        for r in (5, 0, P - Q - 1):                                               # r + q < p
            lines.append(f"xis {h32((r + Q) * Z % P)} {h32(Z)} {h32(r)} 1")      # X = (r + q) Z
            lines.append(f"xis {h32(r * Z % P)} {h32(Z)} {h32(r)} 1")            # X = r Z
            lines.append(f"xis {h32((r + 1) * Z % P)} {h32(Z)} {h32(r)} 0")      # X = (r + 1) Z
            lines.append(f"xis {h32((r + Q + 1) * Z % P)} {h32(Z)} {h32(r)} 0")
        for r in (P - Q, P - Q + 7, Q - 1):                                       # r + q >= p: x = r + q is not a coordinate
            lines.append(f"xis {h32(r * Z % P)} {h32(Z)} {h32(r)} 1")
            lines.append(f"xis {h32((r + Q) % P * Z % P)} {h32(Z)} {h32(r)} 0")  # (r + q) mod p is another x: no match
            lines.append(f"xis {h32((r + 1) * Z % P)} {h32(Z)} {h32(r)} 0")
    lines.append(f"conv {h32(7)} {h32(0)} {h32(0)}")                              # infinity -> 0
    lines.append(f"xis {h32(0)} {h32(0)} {h32(0)} 0")                             # infinity matches nothing, X = r Z = 0 or not
    lines.append(f"xis {h32(7)} {h32(0)} {h32(5)} 0")
    return lines


def write_cases(path):
    d = golden()
    lines = []
    for m in d["mul"]:
        lines += [f"mul {m['P']} {k} {kp}" for k, kp in zip(d["scalars"], m["kP"])]
    lines.append(f"derive {d['derive']['seed'].replace(' ', '+')} {d['derive']['sk']} {d['derive']['pk']}")
    s = d["sign"]
    lines.append(f"refsign {s['seed'].replace(' ', '+')} {s['sk']} {s['pk']} {s['digest_message']} {s['sig_message']} "
                 f"{s['digest_small']} {s['sig_small']}")
    lines.append(f"cross {s['pk']} {s['sig_small']} {s['digest_message']} 0")
    lines.append("prg ecdsa+fixture")
    for g in d["signatures"]:
        lines.append(" ".join(["sig", g["sk"], g["pk"], g["digest"] or "-", g["h"], g["R"], g["conversion"], g["sig"], g["other_digest"],
                               g["other_pk"]]))
    rng = random.Random(11)
    lines.append(f"rinv {h32(0)} {h32(0)}")
    for a in EDGE_SCALARS + [rng.randrange(1, Q) for _ in range(300)]:
        lines.append(f"rinv {h32(a)} {h32(pow(a, -1, Q))}")
    lines += synthetic_cases()
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return len(lines)


def test_model_reproduces_the_reference_fixture():
    """every entry of the fixture through big-integer arithmetic: k P, the derived keys, every signature from its nonce byte
    for byte, conversionFunc, digestToElement at the six lengths, every honest verdict true and every tampered one false"""
    d = golden()
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
    r = subprocess.run([ecdsa_binary(), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout
