"""The big-integer Python model of secp256k1 -- affine points, Lagrange interpolation over the group order -- with Feldman and
Pedersen verification and ECDSA signing and verification on top, and the readers of the three fixtures
(tests/golden/golden_{feldman,ecdsa,pedersen}.json) with the cases files they become for the C++ mirror's test programs.  The
model is neither the reference nor this code; tests/test_{feldman,ecdsa,pedersen}_host.py pin it to what the REFERENCE computed and
tests/test_gpu_{feldman,ecdsa,pedersen}.py compare the kernels against it.  Standard library only."""
import functools
import json
import os
import random

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the curve: y^2 = x^3 + 7 over P, affine, None = infinity (SEC 2, section 2.4.1) ---------------------------------------
P = 2 ** 256 - 2 ** 32 - 977
Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)


def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0] and (a[1] + b[1]) % P == 0:
        return None
    lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) if a == b else (b[1] - a[1]) * pow(b[0] - a[0], -1, P)
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def ec_neg(a):
    return None if a is None else (a[0], -a[1] % P)


def ec_mul(k, a):
    r = None
    for bit in bin(k % Q)[2:]:
        r = ec_add(r, r)
        if bit == "1":
            r = ec_add(r, a)
    return r


def ec_image(a) -> bytes:
    """Serializer<EC>: 0x04 | x | y, infinity 0x06 and zeros"""
    return b"\x06" + bytes(64) if a is None else b"\x04" + a[0].to_bytes(32, "big") + a[1].to_bytes(32, "big")


def ec_from_image(b: bytes):
    assert len(b) == 65 and b[0] in (4, 6), (len(b), b[:1])
    return None if b[0] & 2 else (int.from_bytes(b[1:33], "big"), int.from_bytes(b[33:], "big"))


def lagrange(nodes, x):
    """the basis over `nodes` at x, mod Q"""
    out = []
    for i, xi in enumerate(nodes):
        num = den = 1
        for j, xj in enumerate(nodes):
            if i != j:
                num, den = num * (x - xj) % Q, den * (xi - xj) % Q
        out.append(num * pow(den, -1, Q) % Q)
    return out


def golden(unit):
    """the `data` of tests/golden/golden_<unit>.json"""
    with open(os.path.join(GOLDEN_DIR, "golden_%s.json" % unit)) as fh:
        return json.load(fh)["data"]


def run_commitments(run):
    return [ec_from_image(bytes.fromhex(c)) for c in run["commitments"]]


# ---- Feldman -----------------------------------------------------------------------------------------------------------------
def feldman_verify(share: int, commitments, index: int) -> bool:
    lam = lagrange(range(len(commitments)), index)
    v = None
    for l, c in zip(lam, commitments):
        v = ec_add(v, ec_mul(l, c))
    return v == ec_mul(share, G)


def run_shares(run):
    raw = bytes.fromhex(run["shares"])
    assert len(raw) == 32 * run["n"], (len(raw), run["n"])
    return [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(run["n"])]


def write_feldman_cases(path):
    d = golden("feldman")
    lines = [f"G {d['G']}"]
    lines += [f"mul {m['k']} {m['P']}" for m in d["multiples"]]
    for i in d["identities"]:
        lines.append(" ".join(["id", i["P"], i["Q"], i["P+Q"], i["P+P"], i["2P"], i["P-P"], i["P+inf"], i["-P"], str(int(i["P==Q"]))]))
    for r in d["runs"]:
        lines += [f"prg {r['seed']}", f"run {r['secret']} {r['t']} {r['n']} {r['shares']} {','.join(r['commitments'])}"]
    # "Feldman hom": two sharings off ONE PRG, the second drawn after the first has advanced it (a space in a seed is a '+')
    firsts, seeds = [r["first_secret"] for r in d["hom_runs"]], {r["seed"] for r in d["hom_runs"]}
    assert firsts == [0, 1] and len(seeds) == 1, (firsts, seeds)
    lines.append("prg " + d["hom_runs"][0]["seed"].replace(" ", "+"))
    lines += [f"run {r['secret']} {r['t']} {r['n']} {r['shares']} {','.join(r['commitments'])}" for r in d["hom_runs"]]
    lines.append(f"hom {','.join(d['hom']['commitments'])}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return len(lines)


# ---- Pedersen ----------------------------------------------------------------------------------------------------------------
def pedersen_commitment(share: int, rand: int, h):
    return ec_add(ec_mul(share, G), ec_mul(rand, h))


def pedersen_verify(share: int, rand: int, commitments, index: int, h) -> bool:
    """pedersen.h:178-207 without its shortcut: at an index below commitments.size() the basis is a unit vector"""
    v = None
    for l, c in zip(lagrange(range(len(commitments)), index), commitments):
        v = ec_add(v, ec_mul(l, c))
    return v == pedersen_commitment(share, rand, h)


@functools.lru_cache(maxsize=None)
def pedersen_golden():
    return golden("pedersen")


def scalar_of(hex32: str) -> int:
    assert len(hex32) == 64, len(hex32)
    return int(hex32, 16)


def run_pairs(run):
    """[(share, randomness)] per party"""
    raw = run["shares"]
    assert len(raw) == 128 * run["n"], (len(raw), run["n"])
    return [(int(raw[128 * i:128 * i + 64], 16), int(raw[128 * i + 64:128 * i + 128], 16)) for i in range(run["n"])]


def every_run():
    d = pedersen_golden()
    return d["runs"] + [d["run5"]] + d["hom_runs"] + d["apply"]["sharings"]


def matrix_of(applied):
    raw, rows, cols = applied["matrix"], applied["rows"], applied["cols"]
    assert len(raw) == 64 * rows * cols, (len(raw), rows, cols)
    return [[int(raw[64 * (i * cols + k):64 * (i * cols + k + 1)], 16) for k in range(cols)] for i in range(rows)]


def write_pedersen_cases(path):
    """the fixture as lines for test_pedersen_api (its header has the grammar); a space in a seed is a '+'"""
    d = pedersen_golden()
    lines = [f"h {d['h']} {d['h_wrong']}"]

    def run_line(r):
        return (f"run {r['overload']} {r['secret']} {r['randomness']} {r['t']} {r['n']} {r['counter0']} {r['shares']} "
                f"{','.join(r['commitments'])}")

    for r in d["runs"] + [d["run5"]]:
        lines += ["prg " + r["seed"].replace(" ", "+"), run_line(r)]
    lines.append("prg " + d["hom_runs"][0]["seed"].replace(" ", "+"))
    lines += [run_line(r) for r in d["hom_runs"]]
    lines.append(f"hom {d['hom']['shares']} {','.join(d['hom']['commitments'])} {d['hom']['sum_secret']} {d['hom']['sum_randomness']}")
    lines.append("prg " + d["apply"]["sharings"][0]["seed"].replace(" ", "+"))
    for r in d["apply"]["sharings"]:
        lines += ["draw " + r["secret"], run_line(r)]
    for key in ("vandermonde", "identity"):
        a = d["apply"][key]
        for j, party in enumerate(a["out"]):
            for i, o in enumerate(party):
                lines.append(f"apply {key} {j} {i} {o['share']} {','.join(o['commitments'])}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return len(lines)


# ---- ECDSA (SEC 1, sections 4.1.3 and 4.1.4, without the range checks the reference does not make) ---------------------------
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
    assert len(b) == 64, len(b)
    return int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")


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


def write_ecdsa_cases(path):
    d = golden("ecdsa")
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
