#!/usr/bin/env python3
"""Generate tests/golden/golden_ip.json from the REAL reference: inner products and one small matrix product of Shamir sharings
at ONE opening each, built from its ss::shamirSecretShare, ss::shamirRecoverP, math::innerProd, Matrix::multiply and util::PRG.

This script writes a small harness of its own against the reference's headers, compiles it with the reference's field and PRG
translation units into a temporary directory OUTSIDE the repository, runs it and keeps what it prints.  Elements are their
FF::write images (byteSize bytes, in hex).  Nothing compiled is kept.  Run in the build container only:

    python tests/golden/make_golden_ip.py

Contents (Mersenne61, Mersenne127 and the secp256k1 order):
  inner     (n, t) in {(4,1), (10,3)}, K in {1, 3, 5}.  The inputs come off ONE util::PRG seeded "ip inputs", term after term:
            x_k = FF::random, y_k = FF::random, shamirSecretShare(x_k, t, n), shamirSecretShare(y_k, t, n).  [R] is one dealer's
            double sharing off the PRG "ip dealer": r = FF::random, shamirSecretShare(r, t, n), shamirSecretShare(r, 2t, n).
            Recorded: the secrets x, y; every party's d = sum_k xs_k ys_k + R_2t; the opened d; every party's z = d - R_t; the
            recovered z, which the harness requires to equal math::innerProd of the secrets (the shares of x_k and y_k are not
            kept: d pins them)
  matrix    (4,1): X is 2 x 3, Y is 3 x 2.  Pair p = 0..5 off the PRG "ip matrix": X's entry p and Y's entry p (both row-major)
            and their sharings, in the order above.  [R] is four consecutive double sharings off "ip dealer", one per entry of
            the 2 x 2 result, row-major.  Recorded per result entry as above; the harness requires the recovered Z to equal
            Matrix::multiply of the secrets
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
FIELDS = ["m61", "m127", "secp256k1_scalar"]
NT = [(4, 1), (10, 3)]
KS = [1, 3, 5]
MATRIX = (2, 3, 2)

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ff.h"
#include "scl/math/fp.h"
#include "scl/math/matrix.h"
#include "scl/math/vector.h"
#include "scl/ss/shamir.h"
#include "scl/util/prg.h"

using namespace scl;

static void must(bool b, const char* what) {
  if (!b) {
    std::fprintf(stderr, "harness: %s\n", what);
    std::exit(1);
  }
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
template <typename T>
static std::vector<T> vec(const math::Vector<T>& v) {
  std::vector<T> out;
  for (std::size_t i = 0; i < v.size(); ++i) out.push_back(v[i]);
  return out;
}
template <typename T>
struct Double {
  T r;
  std::vector<T> lo, hi;
};
template <typename T>
static Double<T> deal(util::PRG& prg, std::size_t n, std::size_t t) {
  Double<T> d;
  d.r = T::random(prg);
  d.lo = vec(ss::shamirSecretShare(d.r, t, n, prg));
  d.hi = vec(ss::shamirSecretShare(d.r, 2 * t, n, prg));
  must(ss::shamirRecoverP(math::Vector<T>(d.lo)) == d.r && ss::shamirRecoverP(math::Vector<T>(d.hi)) == d.r, "both sharings recover r");
  return d;
}
template <typename T>
struct Inputs {
  std::vector<T> x, y;
  std::vector<std::vector<T>> xs, ys;  // [pair][party]
};
template <typename T>
static Inputs<T> inputs(const char* seed, std::size_t pairs, std::size_t n, std::size_t t) {
  auto prg = util::PRG::create(seed);
  Inputs<T> in;
  for (std::size_t k = 0; k < pairs; ++k) {
    const T x = T::random(prg);
    const T y = T::random(prg);
    in.xs.push_back(vec(ss::shamirSecretShare(x, t, n, prg)));
    in.ys.push_back(vec(ss::shamirSecretShare(y, t, n, prg)));
    in.x.push_back(x), in.y.push_back(y);
  }
  return in;
}
// one opening: d_j = sum over the listed (xi, yi) pairs of xs[xi][j] ys[yi][j] + hi[j]; z_j = open(d) - lo[j]
template <typename T>
static T one_opening(const Inputs<T>& in, const std::vector<std::size_t>& xi, const std::vector<std::size_t>& yi, const Double<T>& R,
                     std::size_t n, const char* tail) {
  std::vector<T> d, z;
  for (std::size_t j = 0; j < n; ++j) {
    T acc = R.hi[j];
    for (std::size_t k = 0; k < xi.size(); ++k) acc = acc + in.xs[xi[k]][j] * in.ys[yi[k]][j];
    d.push_back(acc);
  }
  const T opened = ss::shamirRecoverP(math::Vector<T>(d));
  for (std::size_t j = 0; j < n; ++j) z.push_back(opened - R.lo[j]);
  const T zz = ss::shamirRecoverP(math::Vector<T>(z));
  std::printf("{");
  elems("d_shares", d, ",");
  std::printf("\"d\":\"%s\",", image(opened).c_str());
  elems("z_shares", z, ",");
  std::printf("\"z\":\"%s\"}%s", image(zz).c_str(), tail);
  return zz;
}
template <typename T>
static void inner(const char* field, std::size_t n, std::size_t t, std::size_t K, bool first) {
  const Inputs<T> in = inputs<T>("ip inputs", K, n, t);
  auto dealer = util::PRG::create("ip dealer");
  const Double<T> R = deal<T>(dealer, n, t);
  std::printf("%s\n{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"K\":%zu,", first ? "" : ",", field, n, t, K);
  elems("x", in.x, ",");
  elems("y", in.y, ",");
  std::vector<std::size_t> idx;
  for (std::size_t k = 0; k < K; ++k) idx.push_back(k);
  std::printf("\"out\":");
  const T z = one_opening<T>(in, idx, idx, R, n, "}");
  must(z == math::innerProd<T>(in.x.begin(), in.x.end(), in.y.begin()), "z = innerProd(x, y)");
}
template <typename T>
static void matrix(const char* field, bool first) {
  const std::size_t n = 4, t = 1, a = 2, K = 3, b = 2;
  const Inputs<T> in = inputs<T>("ip matrix", a * K, n, t);  // a K = K b pairs: X's entry p and Y's entry p
  auto dealer = util::PRG::create("ip dealer");
  math::Matrix<T> X(a, K), Y(K, b);
  for (std::size_t p = 0; p < a * K; ++p) X(p / K, p % K) = in.x[p], Y(p / b, p % b) = in.y[p];
  const auto Z = X.multiply(Y);
  std::printf("%s\n{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"a\":%zu,\"K\":%zu,\"b\":%zu,", first ? "" : ",", field, n, t, a, K, b);
  elems("x", in.x, ",");
  elems("y", in.y, ",");
  std::printf("\"out\":[");
  for (std::size_t i = 0; i < a; ++i)
    for (std::size_t l = 0; l < b; ++l) {
      const Double<T> R = deal<T>(dealer, n, t);
      std::vector<std::size_t> xi, yi;
      for (std::size_t k = 0; k < K; ++k) xi.push_back(i * K + k), yi.push_back(k * b + l);
      const T z = one_opening<T>(in, xi, yi, R, n, (i + 1 == a && l + 1 == b) ? "" : ",");
      must(z == Z(i, l), "Z = X.multiply(Y)");
    }
  std::printf("]}");
}
template <typename T>
static void inners(const char* field, bool first) {
  const std::size_t nt[2][2] = {{4, 1}, {10, 3}};
  for (auto& c : nt)
    for (std::size_t K : {1, 3, 5}) {
      inner<T>(field, c[0], c[1], K, first);
      first = false;
    }
}

int main() {
  using F61 = math::Fp<61>;
  using F127 = math::Fp<127>;
  using Scalar = math::FF<math::ff::Secp256k1Scalar>;
  std::printf("{\"inner\":[");
  inners<F61>("m61", true);
  inners<F127>("m127", false);
  inners<Scalar>("secp256k1_scalar", false);
  std::printf("],\n\"matrix\":[");
  matrix<F61>("m61", true);
  matrix<F127>("m127", false);
  matrix<Scalar>("secp256k1_scalar", false);
  std::printf("]}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_ip_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    d = json.loads(out)
    assert [(r["field"], r["n"], r["t"], r["K"]) for r in d["inner"]] == [(f, n, t, K) for f in FIELDS for n, t in NT for K in KS]
    for r in d["inner"]:
        assert len(r["x"]) == len(r["y"]) == r["K"] and len(r["out"]["d_shares"]) == len(r["out"]["z_shares"]) == r["n"]
    assert [(r["field"], r["n"], r["t"], r["a"], r["K"], r["b"]) for r in d["matrix"]] == [(f, 4, 1) + MATRIX for f in FIELDS]
    for r in d["matrix"]:
        assert len(r["x"]) == len(r["y"]) == 6 and len(r["out"]) == 4 and all(len(o["d_shares"]) == 4 for o in r["out"])
    head = {"generator": "tests/golden/make_golden_ip.py",
            "source": "the reference's ss::shamirSecretShare, ss::shamirRecoverP, math::innerProd, Matrix::multiply and util::PRG; "
                      "elements are FF::write images (byteSize bytes, in hex)"}
    path = os.path.join(HERE, "golden_ip.json")
    with open(path, "w") as fh:       # the harness's own line structure: one run per line
        fh.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"data":' + out.strip() + "}\n")
    with open(path) as fh:
        assert json.load(fh)["data"] == d
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
