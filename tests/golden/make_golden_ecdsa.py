#!/usr/bin/env python3
"""Generate tests/golden/golden_ecdsa.json from the REAL reference's util::ECDSA and math::EC<Secp256k1>.

This script writes a small harness of its own against the reference's headers (sign.h, EC, the Secp256k1 fields, Sha256, PRG),
compiles it with the translation units make_golden_feldman.py uses plus src/scl/util/sha256.cc into a temporary directory
OUTSIDE the repository, runs it and keeps what it prints.  Points are their Serializer<EC> images (65 bytes, uncompressed),
scalars their FF::write images (32 bytes, big-endian), signatures their Signature::write images (64 bytes), digests their bytes,
all in hex.  Nothing compiled is kept.  Run in the build container only:

    python tests/golden/make_golden_ecdsa.py

Digests come from the reference's util::Sha256, not from Hash<256> (its SHA-3, which this project leaves out).  Contents:
  mul         k * P for three points P != G -- 5 G, a random multiple, and a sum left in projective coordinates with Z != 1 -- and
              k in {0, 1, 2, 15, 16, 17, 2^64, 2^255, q - 1} and eight from a seeded PRG; and k * infinity
  derive      the reference's "ECDSA derive" case: sk from the seed "ecdsa derive", pk
  sign        the reference's "ECDSA sign" case with Sha256: sk, pk, the two digests (of "message" as the reference's
              update() hashes the literal, a char[8] with its NUL; and the array {1, 2, 3}), the two signatures with their nonces (the PRG replayed beside the one Sign draws from), the three verdicts
  signatures  twelve more off the seed "ecdsa fixture", digests of 0, 1, 31, 32, 33 and 64 bytes twice over: sk, pk, nonce,
              R = nonce * G, conversionFunc(R), digestToElement(digest), the signature, its verdict, and the verdicts of four
              tamperings -- r + 1, s + 1, another digest (the Sha256 of this one), another key ((sk + 1) * G)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCL_REFERENCE", "/root/reference")
GMP_SO = os.environ.get("GMP_SO", "/usr/lib/x86_64-linux-gnu/libgmp.so.10")
TUS = ["src/scl/math/fields/mersenne61.cc", "src/scl/math/fields/mersenne127.cc", "src/scl/util/prg.cc", "src/scl/util/str.cc",
       "src/scl/math/fields/secp256k1_scalar.cc", "src/scl/math/fields/secp256k1_field.cc", "src/scl/math/fields/ff_ops_gmp.cc",
       "src/scl/math/number.cc", "src/scl/math/curves/secp256k1_curve.cc", "src/scl/util/sha256.cc"]

HARNESS = r"""
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ec.h"
#include "scl/math/ff.h"
#include "scl/serialization/serializer.h"
#include "scl/util/prg.h"
#include "scl/util/sha256.h"
#include "scl/util/sign.h"

using namespace scl;
using EC = math::EC<math::ec::Secp256k1>;
using FF = EC::ScalarField;
using Sig = util::Signature<util::ECDSA>;

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
  s.write(buf);
  std::printf("\"%s\":\"", key);
  hex(buf, 32);
  std::printf("\"%s", tail);
}
static void sg(const char* key, const Sig& s, const char* tail = ",") {
  unsigned char buf[64];
  s.write(buf);
  std::printf("\"%s\":\"", key);
  hex(buf, Sig::byteSize());
  std::printf("\"%s", tail);
}
template <typename D>
static void dg(const char* key, const D& d, const char* tail = ",") {
  std::printf("\"%s\":\"", key);
  hex(d.data(), d.size());
  std::printf("\"%s", tail);
}
static const char* tf(bool b) { return b ? "true" : "false"; }
static void must(bool b, const char* what) {
  if (!b) {
    std::fprintf(stderr, "harness: %s\n", what);
    std::exit(1);
  }
}

int main() {
  const EC G = EC::generator();
  std::printf("{");
  // ---- k * P
  std::vector<FF> ks = {FF(0), FF(1), FF(2), FF(15), FF(16), FF(17), FF::fromString("0000000000000000000000000000000000000000000000010000000000000000"),
                        FF::fromString("8000000000000000000000000000000000000000000000000000000000000000"), FF(0) - FF(1)};
  auto kprg = util::PRG::create("ecdsa-scalars");
  for (int i = 0; i < 8; ++i) ks.push_back(FF::random(kprg));
  const FF m = FF::random(kprg);
  const EC projective = (FF(2) * G + FF(3) * G) + m * G;  // left as the addition made it: Z != 1
  const EC points[] = {FF(5) * G, m * G, projective, EC::zero()};
  std::printf("\"scalars\":[");
  for (std::size_t i = 0; i < ks.size(); ++i) {
    unsigned char buf[32];
    ks[i].write(buf);
    std::printf("%s\"", i ? "," : "");
    hex(buf, 32);
    std::printf("\"");
  }
  std::printf("],\"mul\":[");
  for (std::size_t j = 0; j < 4; ++j) {
    std::printf("%s{", j ? "," : "");
    pt("P", points[j]);
    std::printf("\"kP\":[");
    for (std::size_t i = 0; i < ks.size(); ++i) {
      unsigned char buf[65];
      seri::Serializer<EC>::write(ks[i] * points[j], buf);
      std::printf("%s\"", i ? "," : "");
      hex(buf, 65);
      std::printf("\"");
    }
    std::printf("]}");
  }
  // ---- "ECDSA derive" (test/scl/util/test_ecdsa.cc:27-32)
  {
    auto prg = util::PRG::create("ecdsa derive");
    const auto sk = util::ECDSA::SecretKey::random(prg);
    const auto pk = util::ECDSA::derive(sk);
    must(pk == sk * G, "derive");
    std::printf("],\"derive\":{\"seed\":\"ecdsa derive\",");
    sc("sk", sk);
    pt("pk", pk, "}");
  }
  // ---- "ECDSA sign" (test_ecdsa.cc:34-48), Sha256 in Hash<256>'s place; `peek` runs beside prg and shows each nonce
  {
    auto prg = util::PRG::create("ecdsa sign"), peek = util::PRG::create("ecdsa sign");
    const auto dm = util::Sha256{}.update("message").finalize();
    const auto sk = util::ECDSA::SecretKey::random(prg);
    (void)FF::random(peek);
    const FF k0 = FF::random(peek);
    const auto sig = util::ECDSA::Sign(sk, dm, prg);
    const auto pk = util::ECDSA::derive(sk);
    const std::array<unsigned char, 3> small = {1, 2, 3};
    const FF k1 = FF::random(peek);
    const auto sig_small = util::ECDSA::Sign(sk, small, prg);
    must(sig.r == util::ECDSA::conversionFunc(k0 * G) && sig_small.r == util::ECDSA::conversionFunc(k1 * G), "nonce replay");
    std::printf(",\"sign\":{\"seed\":\"ecdsa sign\",");
    sc("sk", sk);
    pt("pk", pk);
    dg("digest_message", dm);
    dg("digest_small", small);
    sc("nonce_message", k0);
    sc("nonce_small", k1);
    sg("sig_message", sig);
    sg("sig_small", sig_small);
    std::printf("\"verify_message\":%s,\"verify_small\":%s,\"verify_small_sig_on_message\":%s}", tf(util::ECDSA::verify(pk, sig, dm)),
                tf(util::ECDSA::verify(pk, sig_small, small)), tf(util::ECDSA::verify(pk, sig_small, dm)));
  }
  // ---- twelve more
  {
    auto prg = util::PRG::create("ecdsa fixture"), peek = util::PRG::create("ecdsa fixture"), dprg = util::PRG::create("ecdsa digests");
    const std::size_t lens[] = {0, 1, 31, 32, 33, 64, 0, 1, 31, 32, 33, 64};
    std::printf(",\"signatures\":[");
    for (std::size_t i = 0; i < 12; ++i) {
      const FF sk = FF::random(prg);
      (void)FF::random(peek);
      std::vector<unsigned char> d(lens[i]);
      if (!d.empty()) dprg.next(d.data(), d.size());
      const FF k = FF::random(peek);
      const Sig sig = util::ECDSA::Sign(sk, d, prg);
      const EC pk = util::ECDSA::derive(sk), R = k * G;
      must(sig.r == util::ECDSA::conversionFunc(R), "nonce replay");
      const auto other = util::Sha256{}.update(d).finalize();
      std::printf("%s{", i ? "," : "");
      sc("sk", sk);
      pt("pk", pk);
      dg("digest", d);
      sc("h", util::ECDSA::digestToElement(d));
      sc("nonce", k);
      pt("R", R);
      sc("conversion", util::ECDSA::conversionFunc(R));
      sg("sig", sig);
      dg("other_digest", other);
      pt("other_pk", util::ECDSA::derive(sk + FF(1)));
      std::printf("\"verify\":%s,\"tampered\":{\"r_plus_1\":%s,\"s_plus_1\":%s,\"other_digest\":%s,\"other_key\":%s}}",
                  tf(util::ECDSA::verify(pk, sig, d)), tf(util::ECDSA::verify(pk, Sig{sig.r + FF(1), sig.s}, d)),
                  tf(util::ECDSA::verify(pk, Sig{sig.r, sig.s + FF(1)}, d)), tf(util::ECDSA::verify(pk, sig, other)),
                  tf(util::ECDSA::verify(util::ECDSA::derive(sk + FF(1)), sig, d)));
    }
    std::printf("]");
  }
  std::printf("}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_ecdsa_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    doc = {"generator": "tests/golden/make_golden_ecdsa.py",
           "source": "the reference's util::ECDSA / util::Signature<ECDSA> (include/scl/util/sign.h) over math::EC<math::ec::Secp256k1> "
                     "with util::Sha256 digests; points are Serializer<EC> images, scalars FF::write images, signatures "
                     "Signature::write images, in hex",
           "data": json.loads(out)}
    d = doc["data"]
    assert len(d["scalars"]) == 17 and [len(m["kP"]) for m in d["mul"]] == [17] * 4
    assert d["sign"]["verify_message"] and d["sign"]["verify_small"] and not d["sign"]["verify_small_sig_on_message"]
    assert len(d["signatures"]) == 12 and [len(s["digest"]) // 2 for s in d["signatures"]] == [0, 1, 31, 32, 33, 64] * 2
    for s in d["signatures"]:
        assert s["verify"] and not any(s["tampered"].values()) and len(s["tampered"]) == 4
    path = os.path.join(HERE, "golden_ecdsa.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
