#!/usr/bin/env python3
"""Generate tests/golden/golden_triples.json from the REAL reference: its trusted dealer of multiplication triples
(test/scl/protocol/triple.h:37-48) on its util::PRG, ss::additiveShare and ss::shamirSecretShare.

This script writes a small harness of its own against the reference's headers, compiles it with the reference's field and PRG
translation units into a temporary directory OUTSIDE the repository, runs it and keeps what it prints.  Elements are their
FF::write images (byteSize bytes, in hex).  Nothing compiled is kept.  Run in the build container only:

    python tests/golden/make_golden_triples.py

Contents:
  protocol  test/scl/protocol/test_protocol.cc:36-41 as written -- PRG::create(), xs, ys = additiveShare(42 / 11, 2, prg), ts =
            randomTriple2<Fp<61>>(prg), the reference's own function -- and what the two parties of BeaverMul::run compute from
            them (beaver.h:40-61): their e, d and z, and the sums; z0 + z1 = 462
  additive  Mersenne61, Mersenne127 and both secp256k1 fields: five consecutive triples among n in {2, 3, 5} parties off the seed
            "triples fixture" (randomTriple2 with its `2` replaced by n; at n = 2 the harness also runs randomTriple2 itself beside
            it and requires the same triples), and for n = 3 once more after a burn of three blocks, which pins counter0
  shamir    the same with shamirSecretShare(v, t, n, prg) in additiveShare's place at (n, t) in {(4,1), (10,3), (16,7), (20,9)};
            the burn run at (4,1)
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
       "src/scl/math/number.cc"]
SEED = "triples fixture"
ADDITIVE_N = [2, 3, 5]
SHAMIR_NT = [(4, 1), (10, 3), (16, 7), (20, 9)]
FIELDS = ["m61", "m127", "secp256k1_scalar", "secp256k1_field"]
COUNT = 5
BURN = 3

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ff.h"
#include "scl/math/fp.h"
#include "scl/protocol/triple.h"
#include "scl/ss/additive.h"
#include "scl/ss/shamir.h"
#include "scl/util/prg.h"

using namespace scl;

static const char* SEED = "triples fixture";
static void must(bool b, const char* what) {
  if (!b) {
    std::fprintf(stderr, "harness: %s\n", what);
    std::exit(1);
  }
}
template <typename T>
struct Tr {
  std::vector<T> a, b, c;  // party i's shares at [i]
};
template <typename T, typename SHARE>
static Tr<T> deal(util::PRG& prg, SHARE&& share) {  // triple.h:39-45 with `share` where additiveShare(., 2, prg) stands
  auto a = T::random(prg);
  auto b = T::random(prg);
  auto c = a * b;
  auto as = share(a);
  auto bs = share(b);
  auto cs = share(c);
  Tr<T> out;
  for (std::size_t i = 0; i < as.size(); ++i) {
    out.a.push_back(as[i]);
    out.b.push_back(bs[i]);
    out.c.push_back(cs[i]);
  }
  return out;
}
template <typename T>
static std::string image(const T& v) {  // the FF::write image, in hex
  unsigned char buf[64];
  v.write(buf);
  std::string s;
  char h[3];
  for (std::size_t i = 0; i < T::byteSize(); ++i) {
    std::snprintf(h, sizeof h, "%02x", buf[i]);
    s += h;
  }
  return s;
}
template <typename T>
static void elems(const char* key, const std::vector<T>& v, const char* tail) {
  std::printf("\"%s\":[", key);
  for (std::size_t i = 0; i < v.size(); ++i) std::printf("%s\"%s\"", i ? "," : "", image(v[i]).c_str());
  std::printf("]%s", tail);
}
static bool g_first = true;
template <typename T>
static void run(const char* field, std::size_t n, long t, std::size_t burn) {
  auto prg = util::PRG::create(SEED), twin = util::PRG::create(SEED);
  if (burn) {
    std::vector<unsigned char> buf(16 * burn);
    prg.next(buf.data(), buf.size());
    twin.next(buf.data(), buf.size());
  }
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,", g_first ? "" : ",", field, n);
  g_first = false;
  if (t >= 0) std::printf("\"t\":%ld,", t);
  std::printf("\"seed\":\"%s\",\"burn\":%zu,\"triples\":[", SEED, burn);
  for (int k = 0; k < 5; ++k) {
    const Tr<T> tr = t < 0 ? deal<T>(prg, [&](const T& v) { return ss::additiveShare(v, n, prg); })
                           : deal<T>(prg, [&](const T& v) { return ss::shamirSecretShare(v, (std::size_t)t, n, prg); });
    if (t < 0 && n == 2) {  // the reference's own function deals the same
      const auto ref = test::randomTriple2<T>(twin);
      for (std::size_t i = 0; i < 2; ++i) must(ref[i].a == tr.a[i] && ref[i].b == tr.b[i] && ref[i].c == tr.c[i], "randomTriple2");
    }
    T sa = T::zero(), sb = T::zero(), sc = T::zero();
    if (t < 0) {
      for (std::size_t i = 0; i < n; ++i) sa += tr.a[i], sb += tr.b[i], sc += tr.c[i];
    } else {
      sa = ss::shamirRecoverP(math::Vector<T>(tr.a));
      sb = ss::shamirRecoverP(math::Vector<T>(tr.b));
      sc = ss::shamirRecoverP(math::Vector<T>(tr.c));
    }
    must(sa * sb == sc, "c != a b");
    std::printf("%s{", k ? "," : "");
    elems("a", tr.a, ",");
    elems("b", tr.b, ",");
    elems("c", tr.c, "}");
  }
  std::printf("]}");
}
template <typename T>
static void additive_runs(const char* field) {
  for (std::size_t n : {2, 3, 5}) run<T>(field, n, -1, 0);
  run<T>(field, 3, -1, 3);
}
template <typename T>
static void shamir_runs(const char* field) {
  const std::size_t nt[4][2] = {{4, 1}, {10, 3}, {16, 7}, {20, 9}};
  for (auto& c : nt) run<T>(field, c[0], (long)c[1], 0);
  run<T>(field, 4, 1, 3);
}

int main() {
  using F61 = math::Fp<61>;
  using F127 = math::Fp<127>;
  using Scalar = math::FF<math::ff::Secp256k1Scalar>;
  using Field = math::FF<math::ff::Secp256k1Field>;
  std::printf("{");
  {  // test_protocol.cc:36-41, then BeaverMul::run for both parties (beaver.h:40-61)
    auto prg = util::PRG::create();
    auto x = F61(42);
    auto y = F61(11);
    auto xs = ss::additiveShare(x, 2, prg);
    auto ys = ss::additiveShare(y, 2, prg);
    auto ts = test::randomTriple2<F61>(prg);
    std::vector<F61> e, d, z, ta, tb, tc;
    for (int i = 0; i < 2; ++i) {
      e.push_back(xs[i] - ts[i].a);
      d.push_back(ys[i] - ts[i].b);
      ta.push_back(ts[i].a);
      tb.push_back(ts[i].b);
      tc.push_back(ts[i].c);
    }
    e.push_back(e[0] + e[1]);
    d.push_back(d[0] + d[1]);
    for (int i = 0; i < 2; ++i) {
      auto zi = e[2] * ts[i].b + d[2] * ts[i].a + ts[i].c;
      if (i == 0) zi += e[2] * d[2];
      z.push_back(zi);
    }
    z.push_back(z[0] + z[1]);
    must(z[2] == x * y && z[2] == F61(462), "Beaver multiplication protocol");
    std::printf("\"protocol\":{\"x\":\"%s\",\"y\":\"%s\",", image(x).c_str(), image(y).c_str());
    elems("xs", std::vector<F61>{xs[0], xs[1]}, ",");
    elems("ys", std::vector<F61>{ys[0], ys[1]}, ",");
    elems("a", ta, ",");
    elems("b", tb, ",");
    elems("c", tc, ",");
    elems("e", e, ",");
    elems("d", d, ",");
    elems("z", z, "}");
  }
  std::printf(",\"additive\":[");
  additive_runs<F61>("m61");
  additive_runs<F127>("m127");
  additive_runs<Scalar>("secp256k1_scalar");
  additive_runs<Field>("secp256k1_field");
  g_first = true;
  std::printf("],\"shamir\":[");
  shamir_runs<F61>("m61");
  shamir_runs<F127>("m127");
  shamir_runs<Scalar>("secp256k1_scalar");
  shamir_runs<Field>("secp256k1_field");
  std::printf("]}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_triples_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        # (-I test: the reference keeps triple.h under test/scl/protocol, beside the library's own scl/protocol headers)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", f"-I{REF}/test", "-idirafter",
                        "/opt/conda/include", "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    doc = {"generator": "tests/golden/make_golden_triples.py",
           "source": "the reference's test::randomTriple2 (test/scl/protocol/triple.h:37-48), ss::additiveShare, ss::shamirSecretShare "
                     "and util::PRG; elements are FF::write images (byteSize bytes, in hex)",
           "data": json.loads(out)}
    d = doc["data"]
    le = lambda v: v.to_bytes(8, "little").hex()
    assert d["protocol"]["z"][2] == le(462) and d["protocol"]["x"] == le(42) and d["protocol"]["y"] == le(11)
    assert [(r["field"], r["n"], r["burn"]) for r in d["additive"]] == [(f, n, b) for f in FIELDS for n, b in [(n, 0) for n in ADDITIVE_N] + [(3, BURN)]]
    assert [(r["field"], r["n"], r["t"], r["burn"]) for r in d["shamir"]] == \
        [(f, n, t, b) for f in FIELDS for n, t, b in [(n, t, 0) for n, t in SHAMIR_NT] + [(4, 1, BURN)]]
    for r in d["additive"] + d["shamir"]:
        assert r["seed"] == SEED and len(r["triples"]) == COUNT and all(len(tr[k]) == r["n"] for tr in r["triples"] for k in "abc")
    path = os.path.join(HERE, "golden_triples.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
