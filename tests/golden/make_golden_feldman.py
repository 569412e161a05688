#!/usr/bin/env python3
"""Generate tests/golden/golden_feldman.json from the REAL reference's math::EC<Secp256k1> and ss::feldmanSecretShare.

This script writes a small harness of its own against the reference's headers (EC, the Secp256k1 fields, feldman.h, PRG),
compiles it with the translation units the oracle's `make ref` uses plus src/scl/math/curves/secp256k1_curve.cc into a temporary
directory OUTSIDE the repository, runs it and keeps what it prints.  Points are their Serializer<EC> images (65 bytes,
uncompressed), scalars their Serializer<FF> images (32 bytes, big-endian), both in hex.  Nothing compiled is kept.  Run in the
build container only:

    python tests/golden/make_golden_feldman.py

Contents: base-point multiples k * G; point identities (P + Q, P + P, 2P, P - P, P + infinity, -P, equality with a copy under
other projective coordinates); feldmanSecretShare runs for (t, n) in RUNS with seed "feldman" and secret 123 and the two runs of
the reference's "Feldman hom" test, each with its shares, commitments and the verdicts of feldmanVerify at index 0 and for every
party; for t >= 1 also three tampered inputs, all for the last party (index n > t, where every commitment enters the sum): its
share off by one, commitment 0 replaced by G, its share at index n - 1.  With t = 0 the polynomial is constant and a right share
verifies at every index, so there is nothing to record.
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

HARNESS = r"""
#include <cstdio>
#include <string>
#include <vector>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ec.h"
#include "scl/math/ff.h"
#include "scl/math/vector.h"
#include "scl/serialization/serializer.h"
#include "scl/ss/feldman.h"
#include "scl/ss/shamir.h"
#include "scl/util/prg.h"

using namespace scl;
using EC = math::EC<math::ec::Secp256k1>;
using FF = EC::ScalarField;

static void hex(const unsigned char* p, std::size_t n) {
  for (std::size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}
static void pt(const char* key, const EC& p, const char* tail = ",") {
  unsigned char buf[65];
  const std::size_t n = seri::Serializer<EC>::write(p, buf);
  std::printf("\"%s\":\"", key);
  hex(buf, n);
  std::printf("\"%s", tail);
}
static void sc(const char* key, const FF& s, const char* tail = ",") {
  unsigned char buf[32];
  const std::size_t n = seri::Serializer<FF>::write(s, buf);
  std::printf("\"%s\":\"", key);
  hex(buf, n);
  std::printf("\"%s", tail);
}
static const char* tf(bool b) { return b ? "true" : "false"; }

static void run(util::PRG& prg, const char* seed, std::size_t first_secret, int secret, std::size_t t, std::size_t n, const char* tail) {
  const FF s(secret);
  const auto sh = ss::feldmanSecretShare<EC>(s, t, n, prg);
  std::printf("{\"seed\":\"%s\",\"first_secret\":%zu,\"secret\":%d,\"t\":%zu,\"n\":%zu,\"shares\":\"", seed, first_secret, secret, t, n);
  for (std::size_t i = 0; i < n; ++i) {
    unsigned char buf[32];
    seri::Serializer<FF>::write(sh.shares[i], buf);
    hex(buf, 32);
  }
  std::printf("\",\"commitments\":[");
  for (std::size_t k = 0; k <= t; ++k) {
    unsigned char buf[65];
    seri::Serializer<EC>::write(sh.commitments[k], buf);
    std::printf("%s\"", k ? "," : "");
    hex(buf, 65);
    std::printf("\"");
  }
  std::printf("],\"verify_secret_at_0\":%s,\"verify_party\":[", tf(ss::feldmanVerify<EC>(s, sh.commitments, 0)));
  for (std::size_t p = 0; p < n; ++p) std::printf("%s%s", p ? "," : "", tf(ss::feldmanVerify(sh.getShare(p), p + 1)));
  std::printf("]");
  if (t >= 1) {
    std::vector<EC> c = sh.commitments.toStlVector();
    c[0] = EC::generator();
    // at the last party's index n > t, where every commitment enters the sum (at an index k <= t the basis is a unit vector)
    std::printf(",\"tampered\":{\"share_off_by_one\":%s,\"commitment_0_is_G\":%s,\"last_share_at_index_n_minus_1\":%s}",
                tf(ss::feldmanVerify<EC>(sh.shares[n - 1] + FF(1), sh.commitments, n)),
                tf(ss::feldmanVerify<EC>(sh.shares[n - 1], math::Vector<EC>{c}, n)),
                tf(ss::feldmanVerify<EC>(sh.shares[n - 1], sh.commitments, n - 1)));
  }
  std::printf("}%s", tail);
}

int main() {
  const EC G = EC::generator();
  std::printf("{");
  pt("G", G);
  // ---- base-point multiples
  std::vector<FF> ks = {FF(0), FF(1), FF(2), FF(3), FF(15), FF(16), FF(17), FF::fromString("0000000000000000000000000000000000000000000000010000000000000000"),
                        FF::fromString("8000000000000000000000000000000000000000000000000000000000000000"), FF(0) - FF(1)};
  auto kprg = util::PRG::create("feldman-scalars");
  for (int i = 0; i < 8; ++i) ks.push_back(FF::random(kprg));
  std::printf("\"multiples\":[");
  std::vector<EC> ps;
  for (std::size_t i = 0; i < ks.size(); ++i) {
    ps.push_back(ks[i] * G);
    std::printf("%s{", i ? "," : "");
    sc("k", ks[i]);
    pt("P", ps.back(), "}");
  }
  // ---- identities over pairs of those points
  const std::size_t pairs[][2] = {{1, 2}, {10, 11}, {12, 9}, {13, 13}, {8, 14}, {0, 15}};
  std::printf("],\"identities\":[");
  for (std::size_t i = 0; i < sizeof(pairs) / sizeof(pairs[0]); ++i) {
    const EC P = ps[pairs[i][0]], Q = ps[pairs[i][1]];
    const EC sum = P + Q;  // projective coordinates with Z != 1 (unless an operand is infinity)
    EC flat = sum;
    flat.normalize();
    std::printf("%s{", i ? "," : "");
    pt("P", P);
    pt("Q", Q);
    pt("P+Q", sum);
    pt("P+P", P + P);
    pt("2P", P.doublePoint());
    pt("P-P", P - P);
    pt("P+inf", P + EC::zero());
    pt("-P", -P);
    std::printf("\"P+P==2P\":%s,\"sum==normalized_sum\":%s,\"P==Q\":%s}", tf(P + P == P.doublePoint()), tf(sum == flat), tf(P == Q));
  }
  // ---- feldmanSecretShare
  std::printf("],\"runs\":[");
  const std::size_t tn[][2] = {RUNS};
  const std::size_t nruns = sizeof(tn) / sizeof(tn[0]);
  for (std::size_t i = 0; i < nruns; ++i) {
    auto prg = util::PRG::create("feldman");
    run(prg, "feldman", 0, 123, tn[i][0], tn[i][1], i + 1 < nruns ? "," : "");
  }
  // ---- "Feldman hom" (test/scl/ss/test_feldman.cc:47-64): two sharings off one PRG, added
  std::printf("],\"hom_runs\":[");
  {
    auto prg = util::PRG::create("feldman hom");
    run(prg, "feldman hom", 0, 123, 4, 10, ",");
    run(prg, "feldman hom", 1, 44, 4, 10, "");
  }
  {
    auto prg = util::PRG::create("feldman hom");
    const auto a = ss::feldmanSecretShare<EC>(FF(123), 4, 10, prg);
    const auto b = ss::feldmanSecretShare<EC>(FF(44), 4, 10, prg);
    const auto s2 = a.shares.add(b.shares);
    const auto c2 = a.commitments.add(b.commitments);
    std::printf("],\"hom\":{\"commitments\":[");
    for (std::size_t k = 0; k < c2.size(); ++k) {
      unsigned char buf[65];
      seri::Serializer<EC>::write(c2[k], buf);
      std::printf("%s\"", k ? "," : "");
      hex(buf, 65);
      std::printf("\"");
    }
    std::printf("],\"verify_sum_at_0\":%s,\"verify_share_5_at_6\":%s}", tf(ss::feldmanVerify<EC>({FF(123) + FF(44), c2}, 0)),
                tf(ss::feldmanVerify<EC>({s2[5], c2}, 6)));
  }
  std::printf("}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_feldman_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS.replace("{RUNS}", "{" + ", ".join("{%d, %d}" % r for r in RUNS) + "}"))
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    doc = {"generator": "tests/golden/make_golden_feldman.py",
           "source": "the reference's math::EC<math::ec::Secp256k1> (include/scl/math/ec.h, src/scl/math/curves/secp256k1_curve.cc) "
                     "and ss::feldmanSecretShare / feldmanVerify (include/scl/ss/feldman.h); points are Serializer<EC> images, "
                     "scalars Serializer<FF<Secp256k1Scalar>> images, in hex",
           "data": json.loads(out)}
    d = doc["data"]
    for r in d["runs"] + d["hom_runs"]:
        assert r["verify_secret_at_0"] and all(r["verify_party"])
        assert not any(r.get("tampered", {}).values())
    assert d["hom"]["verify_sum_at_0"] and d["hom"]["verify_share_5_at_6"]
    path = os.path.join(HERE, "golden_feldman.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
