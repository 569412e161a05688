#!/usr/bin/env python3
"""Generate tests/golden/golden_pedersen.json from the REAL reference's ss::pedersenSecretShare / pedersenVerify / apply.

This script writes a small harness of its own against the reference's headers (EC, the Secp256k1 fields, pedersen.h, PRG),
compiles it with the translation units make_golden_feldman.py uses into a temporary directory OUTSIDE the repository, runs it
and keeps what it prints.  Points are their Serializer<EC> images (65 bytes, uncompressed), scalars their Serializer<FF> images
(32 bytes, big-endian), a share is its {share, randomness} pair (64 bytes), all in hex.  Nothing compiled is kept.  Run in the
build container only:

    python tests/golden/make_golden_pedersen.py

Contents, with h = 42 * G as in the reference's test/scl/ss/test_pedersen.cc: pedersenSecretShare runs for (t, n) in RUNS with
seed "Pedersen", secret 123 and randomness 42; one run through the 5-argument overload, which draws the randomness first; the
two sharings of "Pedersen hom" off one PRG and their sums; the five sharings of "Pedersen apply" (getShares(5, 2)) and what
ss::apply makes of every party's shares with vandermonde(3, 5) and with the identity.  Every run has the verdicts of
pedersenVerify at index 0 and for every party; for t >= 1 also five tampered inputs, all for the last party (index n > t, where
every commitment enters the sum): its share + 1, its randomness + 1, commitment 0 replaced by G, its share at index n - 1, and
h' = 43 * G.  Every one of them must be rejected, or this script fails.

`counter0` is added here, not by the harness: the PRG block at which the run's shamirSecretShare begins -- FF::random takes two
AES blocks (32 bytes), a sharing over Array<FF, 2> takes 4 (t + 1).
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCL_REFERENCE", "/root/reference")
GMP_SO = os.environ.get("GMP_SO", "/usr/lib/x86_64-linux-gnu/libgmp.so.10")
RUNS = [(0, 1), (1, 2), (3, 10), (4, 24)]
TUS = ["src/scl/math/fields/mersenne61.cc", "src/scl/math/fields/mersenne127.cc", "src/scl/util/prg.cc", "src/scl/util/str.cc",
       "src/scl/math/fields/secp256k1_scalar.cc", "src/scl/math/fields/secp256k1_field.cc", "src/scl/math/fields/ff_ops_gmp.cc",
       "src/scl/math/number.cc", "src/scl/math/curves/secp256k1_curve.cc"]
TAMPERED = ["share_plus_1", "randomness_plus_1", "commitment_0_is_G", "last_share_at_index_n_minus_1", "h_is_43G"]

HARNESS = r"""
#include <cstdio>
#include <string>
#include <vector>

#include "scl/math/array.h"
#include "scl/math/curves/secp256k1.h"
#include "scl/math/ec.h"
#include "scl/math/ff.h"
#include "scl/math/matrix.h"
#include "scl/math/vector.h"
#include "scl/serialization/serializer.h"
#include "scl/ss/pedersen.h"
#include "scl/ss/shamir.h"
#include "scl/util/prg.h"

using namespace scl;
using EC = math::EC<math::ec::Secp256k1>;
using FF = EC::ScalarField;
using Pair = math::Array<FF, 2>;

static const EC h = EC::generator() * FF(42);
static const EC h_wrong = EC::generator() * FF(43);

static void hex(const unsigned char* p, std::size_t n) {
  for (std::size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}
static void raw_pt(const EC& p) {
  unsigned char buf[65];
  hex(buf, seri::Serializer<EC>::write(p, buf));
}
static void raw_sc(const FF& s) {
  unsigned char buf[32];
  hex(buf, seri::Serializer<FF>::write(s, buf));
}
static void pt(const char* key, const EC& p, const char* tail = ",") {
  std::printf("\"%s\":\"", key);
  raw_pt(p);
  std::printf("\"%s", tail);
}
static void sc(const char* key, const FF& s, const char* tail = ",") {
  std::printf("\"%s\":\"", key);
  raw_sc(s);
  std::printf("\"%s", tail);
}
static void pairs(const char* key, const math::Vector<Pair>& v, const char* tail = ",") {
  std::printf("\"%s\":\"", key);
  for (std::size_t i = 0; i < v.size(); ++i) {
    raw_sc(v[i][0]);
    raw_sc(v[i][1]);
  }
  std::printf("\"%s", tail);
}
static void points(const char* key, const math::Vector<EC>& v, const char* tail = ",") {
  std::printf("\"%s\":[", key);
  for (std::size_t k = 0; k < v.size(); ++k) {
    std::printf("%s\"", k ? "," : "");
    raw_pt(v[k]);
    std::printf("\"");
  }
  std::printf("]%s", tail);
}
static const char* tf(bool b) { return b ? "true" : "false"; }

// one sharing with everything the tests compare; `overload` is 6 (randomness given) or 5 (drawn from the PRG first)
static ss::PedersenSharing<EC> run(util::PRG& prg, const char* seed, int overload, const FF& secret, const FF& given, std::size_t t,
                                   std::size_t n, const char* tail) {
  FF rand = given;
  ss::PedersenSharing<EC> sh;
  if (overload == 5) {
    auto copy = prg;  // the randomness the 5-argument overload is about to draw
    rand = FF::random(copy);
    sh = ss::pedersenSecretShare<EC>(secret, t, n, prg, h);
  } else {
    sh = ss::pedersenSecretShare<EC>(secret, t, n, prg, h, rand);
  }
  std::printf("{\"seed\":\"%s\",\"overload\":%d,\"t\":%zu,\"n\":%zu,", seed, overload, t, n);
  sc("secret", secret);
  sc("randomness", rand);
  pairs("shares", sh.shares);
  points("commitments", sh.commitments);
  std::printf("\"verify_secret_at_0\":%s,\"verify_party\":[", tf(ss::pedersenVerify<EC>(Pair{{secret, rand}}, sh.commitments, 0, h)));
  for (std::size_t p = 0; p < n; ++p) std::printf("%s%s", p ? "," : "", tf(ss::pedersenVerify(sh.getShare(p), p + 1, h)));
  std::printf("]");
  if (t >= 1) {
    std::vector<EC> c = sh.commitments.toStlVector();
    c[0] = EC::generator();
    const Pair last = sh.shares[n - 1];
    // at the last party's index n > t, where every commitment enters the sum (at an index k <= t the basis is a unit vector)
    std::printf(",\"tampered\":{\"share_plus_1\":%s,\"randomness_plus_1\":%s,\"commitment_0_is_G\":%s,"
                "\"last_share_at_index_n_minus_1\":%s,\"h_is_43G\":%s}",
                tf(ss::pedersenVerify<EC>(Pair{{last[0] + FF(1), last[1]}}, sh.commitments, n, h)),
                tf(ss::pedersenVerify<EC>(Pair{{last[0], last[1] + FF(1)}}, sh.commitments, n, h)),
                tf(ss::pedersenVerify<EC>(last, math::Vector<EC>{c}, n, h)),
                tf(ss::pedersenVerify<EC>(last, sh.commitments, n - 1, h)),
                tf(ss::pedersenVerify<EC>(last, sh.commitments, n, h_wrong)));
  }
  std::printf("}%s", tail);
  return sh;
}

// ss::apply over every party's shares: out[party][row] = {share pair, commitments}, and the verdict of each at party + 1
static void applied(const char* key, const std::vector<std::vector<ss::PedersenShare<EC>>>& in, const math::Matrix<FF>& m,
                    const char* tail) {
  std::printf("\"%s\":{\"rows\":%zu,\"cols\":%zu,\"matrix\":\"", key, m.rows(), m.cols());
  for (std::size_t i = 0; i < m.rows(); ++i)
    for (std::size_t k = 0; k < m.cols(); ++k) raw_sc(m(i, k));
  std::printf("\",\"out\":[");
  for (std::size_t j = 0; j < in.size(); ++j) {
    const auto out = ss::apply<EC>(in[j], m);
    std::printf("%s[", j ? "," : "");
    for (std::size_t i = 0; i < out.size(); ++i) {
      std::printf("%s{\"share\":\"", i ? "," : "");
      raw_sc(out[i].share[0]);
      raw_sc(out[i].share[1]);
      std::printf("\",");
      points("commitments", out[i].commitments);
      std::printf("\"verify\":%s}", tf(ss::pedersenVerify(out[i], j + 1, h)));
    }
    std::printf("]");
  }
  std::printf("]}%s", tail);
}

int main() {
  std::printf("{");
  pt("G", EC::generator());
  pt("h", h);
  pt("h_wrong", h_wrong);
  std::printf("\"runs\":[");
  const std::size_t tn[][2] = {RUNS};
  const std::size_t nruns = sizeof(tn) / sizeof(tn[0]);
  for (std::size_t i = 0; i < nruns; ++i) {
    auto prg = util::PRG::create("Pedersen");
    run(prg, "Pedersen", 6, FF(123), FF(42), tn[i][0], tn[i][1], i + 1 < nruns ? "," : "");
  }
  std::printf("],\"run5\":");
  {
    auto prg = util::PRG::create("Pedersen five");
    run(prg, "Pedersen five", 5, FF(123), FF(0), 3, 10, ",");
  }
  // ---- "Pedersen hom" (test/scl/ss/test_pedersen.cc:54-73): two sharings off one PRG, added
  std::printf("\"hom_runs\":[");
  {
    auto prg = util::PRG::create("Pedersen hom");
    const auto a = run(prg, "Pedersen hom", 5, FF(123), FF(0), 4, 10, ",");
    const auto b = run(prg, "Pedersen hom", 5, FF(44), FF(0), 4, 10, "");
    const auto s2 = a.shares.add(b.shares);
    const auto c2 = a.commitments.add(b.commitments);
    const auto sum = ss::shamirRecoverP(s2.subVector(5));
    std::printf("],\"hom\":{");
    pairs("shares", s2);
    points("commitments", c2);
    sc("sum_secret", sum[0]);
    sc("sum_randomness", sum[1]);
    std::printf("\"sum_secret_is_167\":%s,\"verify_share_4_at_5\":%s,\"verify_sum_at_0\":%s},", tf(sum[0] == FF(123) + FF(44)),
                tf(ss::pedersenVerify<EC>({s2[4], c2}, 5, h)), tf(ss::pedersenVerify<EC>({sum, c2}, 0, h)));
  }
  // ---- "Pedersen apply" / "Pedersen apply id" (test_pedersen.cc:75-136): getShares(5, 2)
  {
    const std::size_t n = 5, t = 2;
    auto prg = util::PRG::create("Pedersen apply");
    std::vector<std::vector<ss::PedersenShare<EC>>> shares(n);
    std::printf("\"apply\":{\"n\":%zu,\"t\":%zu,\"sharings\":[", n, t);
    for (std::size_t i = 0; i < n; ++i) {
      const auto secret = FF::random(prg);
      const auto shrs = run(prg, "Pedersen apply", 5, secret, FF(0), t, n, i + 1 < n ? "," : "");
      for (std::size_t j = 0; j < n; ++j) shares[j].emplace_back(shrs.getShare(j));
    }
    std::printf("],");
    applied("vandermonde", shares, math::Matrix<FF>::vandermonde(n - t, n), ",");
    applied("identity", shares, math::Matrix<FF>::identity(n), "}");
  }
  std::printf("}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_pedersen_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS.replace("{RUNS}", "{" + ", ".join("{%d, %d}" % r for r in RUNS) + "}"))
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    doc = {"generator": "tests/golden/make_golden_pedersen.py",
           "source": "the reference's ss::pedersenSecretShare / pedersenVerify / apply (include/scl/ss/pedersen.h) over "
                     "math::EC<math::ec::Secp256k1> with h = 42 G; points are Serializer<EC> images, scalars "
                     "Serializer<FF<Secp256k1Scalar>> images, a share is {share, randomness}, in hex",
           "data": json.loads(out)}
    d = doc["data"]

    def number(runs):
        """counter0 of each run's shamirSecretShare off one PRG, in order"""
        at = 0
        for r in runs:
            if r is None:
                at += 2  # a secret drawn with FF::random
                continue
            at += 2 if r["overload"] == 5 else 0
            r["counter0"] = at
            at += 4 * (r["t"] + 1)

    for r in d["runs"]:
        number([r])
    number([d["run5"]])
    number(d["hom_runs"])
    number([x for r in d["apply"]["sharings"] for x in (None, r)])
    every = d["runs"] + [d["run5"]] + d["hom_runs"] + d["apply"]["sharings"]
    for r in every:
        assert r["verify_secret_at_0"] and all(r["verify_party"]) and len(r["verify_party"]) == r["n"]
        if r["t"] >= 1:
            assert sorted(r["tampered"]) == sorted(TAMPERED) and not any(r["tampered"].values()), r["tampered"]
    assert [(r["t"], r["n"]) for r in d["runs"]] == RUNS
    assert d["hom"]["sum_secret_is_167"] and d["hom"]["verify_share_4_at_5"] and d["hom"]["verify_sum_at_0"]
    for key, rows in (("vandermonde", 3), ("identity", 5)):
        a = d["apply"][key]
        assert a["rows"] == rows and a["cols"] == 5 and len(a["out"]) == 5
        assert all(len(party) == rows and all(o["verify"] for o in party) for party in a["out"])
    for j, party in enumerate(d["apply"]["identity"]["out"]):  # "Pedersen apply id": the identity gives the inputs back
        for i, o in enumerate(party):
            r = d["apply"]["sharings"][i]
            assert o["share"] == r["shares"][128 * j:128 * j + 128] and o["commitments"] == r["commitments"]
    path = os.path.join(HERE, "golden_pedersen.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
