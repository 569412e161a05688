"""Pedersen VSS, the host half: ss::pedersen* of the C++ mirror (tests/cxx/test_pedersen_api.cc) against what the REFERENCE
computed (tests/golden/golden_pedersen.json), and the big-integer Python model of tests/test_feldman_host.py, extended with
pedersen_verify, which pins the same fixture by something that is neither the reference nor this code.  The model also checks
the kernels in tests/test_gpu_pedersen.py."""
import functools
import json
import os
import subprocess

from test_feldman_host import CXX, G, Q, ROOT, ec_add, ec_from_image, ec_image, ec_mul, lagrange

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_pedersen.json")
TAMPERED = ["share_plus_1", "randomness_plus_1", "commitment_0_is_G", "last_share_at_index_n_minus_1", "h_is_43G"]


def pedersen_commitment(share: int, rand: int, h):
    return ec_add(ec_mul(share, G), ec_mul(rand, h))


def pedersen_verify(share: int, rand: int, commitments, index: int, h) -> bool:
    """pedersen.h:178-207 without its shortcut: at an index below commitments.size() the basis is a unit vector"""
    v = None
    for l, c in zip(lagrange(range(len(commitments)), index), commitments):
        v = ec_add(v, ec_mul(l, c))
    return v == pedersen_commitment(share, rand, h)


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["data"]


def scalar_of(hex32: str) -> int:
    assert len(hex32) == 64
    return int(hex32, 16)


def run_pairs(run):
    """[(share, randomness)] per party"""
    raw = run["shares"]
    assert len(raw) == 128 * run["n"]
    return [(int(raw[128 * i:128 * i + 64], 16), int(raw[128 * i + 64:128 * i + 128], 16)) for i in range(run["n"])]


def run_commitments(run):
    return [ec_from_image(bytes.fromhex(c)) for c in run["commitments"]]


def every_run():
    d = golden()
    return d["runs"] + [d["run5"]] + d["hom_runs"] + d["apply"]["sharings"]


def matrix_of(applied):
    raw, rows, cols = applied["matrix"], applied["rows"], applied["cols"]
    assert len(raw) == 64 * rows * cols
    return [[int(raw[64 * (i * cols + k):64 * (i * cols + k + 1)], 16) for k in range(cols)] for i in range(rows)]


def pedersen_binary():
    """tests/cxx/test_pedersen_api.cc compiled against the mirror (build() leaves it in place; rebuilt here when stale)"""
    src, exe = os.path.join(CXX, "test_pedersen_api.cc"), os.path.join(CXX, "_build", "test_pedersen_api")
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    newest = max(os.path.getmtime(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(newest, os.path.getmtime(src)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{lib}", "-lscl_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def write_cases(path):
    """the fixture as lines for test_pedersen_api (its header has the grammar); a space in a seed is a '+'"""
    d = golden()
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


def test_model_reproduces_the_reference_fixture():
    """every entry of the fixture through big-integer affine arithmetic: h, the commitments of every run, the verdicts (the
    five tampered inputs false), the sums of "Pedersen hom" and both outputs of ss::apply"""
    d = golden()
    h, h_wrong = ec_from_image(bytes.fromhex(d["h"])), ec_from_image(bytes.fromhex(d["h_wrong"]))
    assert ec_image(G).hex() == d["G"] and h == ec_mul(42, G) and h_wrong == ec_mul(43, G)
    assert [(r["t"], r["n"], r["overload"]) for r in d["runs"]] == [(0, 1, 6), (1, 2, 6), (3, 10, 6), (4, 24, 6)]
    assert all(scalar_of(r["secret"]) == 123 and scalar_of(r["randomness"]) == 42 for r in d["runs"])
    assert d["run5"]["overload"] == 5 and d["run5"]["counter0"] == 2 and [r["counter0"] for r in d["hom_runs"]] == [2, 24]
    for r in every_run():
        t, n, pairs, com = r["t"], r["n"], run_pairs(r), run_commitments(r)
        secret, rand = scalar_of(r["secret"]), scalar_of(r["randomness"])
        assert com == [pedersen_commitment(s, b, h) for s, b in [(secret, rand)] + pairs[:t]]
        assert r["verify_secret_at_0"] and pedersen_verify(secret, rand, com, 0, h)
        # the model's own walk over the parties is kept short: both ends and one in the middle
        assert all(r["verify_party"]) and len(r["verify_party"]) == n
        for p in sorted({0, n // 2, n - 1}):
            assert pedersen_verify(*pairs[p], com, p + 1, h)
        if t >= 1:
            assert sorted(r["tampered"]) == sorted(TAMPERED) and not any(r["tampered"].values())
            s, b = pairs[n - 1]
            assert not pedersen_verify((s + 1) % Q, b, com, n, h)
            assert not pedersen_verify(s, (b + 1) % Q, com, n, h)
            assert not pedersen_verify(s, b, [G] + com[1:], n, h)
            assert not pedersen_verify(s, b, com, n - 1, h)
            assert not pedersen_verify(s, b, com, n, h_wrong)
    a, b = d["hom_runs"]
    hom = d["hom"]
    com2 = [ec_add(x, y) for x, y in zip(run_commitments(a), run_commitments(b))]
    assert [ec_image(c).hex() for c in com2] == hom["commitments"]
    sums = [((x + u) % Q, (y + v) % Q) for (x, y), (u, v) in zip(run_pairs(a), run_pairs(b))]
    assert sums == run_pairs({"shares": hom["shares"], "n": 10})
    assert scalar_of(hom["sum_secret"]) == 123 + 44
    assert scalar_of(hom["sum_randomness"]) == (scalar_of(a["randomness"]) + scalar_of(b["randomness"])) % Q
    assert hom["verify_share_4_at_5"] and pedersen_verify(*sums[4], com2, 5, h)
    assert hom["verify_sum_at_0"] and pedersen_verify(167, scalar_of(hom["sum_randomness"]), com2, 0, h)
    # ss::apply: out[party j][row i] = sum_k M[i][k] * (party j's share of sharing k, and sharing k's commitments)
    ap = d["apply"]
    ins = [(run_pairs(r), run_commitments(r)) for r in ap["sharings"]]
    assert ap["n"] == 5 and ap["t"] == 2 and len(ins) == 5
    assert matrix_of(ap["vandermonde"]) == [[(i + 1) ** k for k in range(5)] for i in range(3)]
    assert matrix_of(ap["identity"]) == [[int(i == k) for k in range(5)] for i in range(5)]
    for key in ("vandermonde", "identity"):
        M = matrix_of(ap[key])
        want_com = []
        for row in M:
            acc = [None] * 3
            for m, (_, com) in zip(row, ins):
                acc = [ec_add(x, ec_mul(m, c)) for x, c in zip(acc, com)]
            want_com.append([ec_image(c).hex() for c in acc])
        for j, party in enumerate(ap[key]["out"]):
            for i, o in enumerate(party):
                share = tuple(sum(m * pairs[j][c] for m, (pairs, _) in zip(M[i], ins)) % Q for c in (0, 1))
                assert (scalar_of(o["share"][:64]), scalar_of(o["share"][64:])) == share and o["commitments"] == want_com[i]
                assert o["verify"]
        for j in (0, 4):
            o = ap[key]["out"][j][-1]
            com = [ec_from_image(bytes.fromhex(c)) for c in o["commitments"]]
            assert pedersen_verify(scalar_of(o["share"][:64]), scalar_of(o["share"][64:]), com, j + 1, h)


def test_cxx_mirror_computes_what_the_reference_computed(tmp_path):
    """all four cases of the reference's test_pedersen.cc and every entry of the fixture -- shares, commitments, apply outputs,
    verdicts -- through ss::pedersen* of the mirror"""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run([pedersen_binary(), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout
