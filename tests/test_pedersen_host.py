"""Pedersen VSS, the host half: ss::pedersen* of the C++ mirror (tests/cxx/test_pedersen_api.cc) against what the REFERENCE
computed (tests/golden/golden_pedersen.json), and the big-integer Python model of tests/secp256k1_model.py with its
pedersen_verify, which pins the same fixture by something that is neither the reference nor this code.  The model also checks
the kernels in tests/test_gpu_pedersen.py."""
import subprocess

from cxx_support import mirror_binary
from secp256k1_model import (G, Q, ec_add, ec_from_image, ec_image, ec_mul, every_run, matrix_of, pedersen_commitment, pedersen_verify, run_commitments,
                             run_pairs, scalar_of)
from secp256k1_model import pedersen_golden as golden
from secp256k1_model import write_pedersen_cases as write_cases

TAMPERED = ["share_plus_1", "randomness_plus_1", "commitment_0_is_G", "last_share_at_index_n_minus_1", "h_is_43G"]


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
    r = subprocess.run([mirror_binary("pedersen"), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n} cases" in r.stdout and " 0 failures" in r.stdout, r.stdout
