#!/usr/bin/env python3
"""Generate tests/golden/golden_hm.json from the REAL reference: double sharings dealt by its ss::shamirSecretShare on its
util::PRG, its Matrix::hyperInvertible and Matrix::multiply, and a Damgard-Nielsen multiplication built from them.

This script writes a small harness of its own against the reference's headers, compiles it with the reference's field and PRG
translation units into a temporary directory OUTSIDE the repository, runs it and keeps what it prints.  Elements are their
FF::write images (byteSize bytes, in hex).  Nothing compiled is kept.  Run in the build container only:

    python tests/golden/make_golden_hm.py

Contents:
  him       Matrix<FF>::hyperInvertible(m, n) for (m, n) in {(1,1), (3,4), (4,4), (7,10)}, row-major
  double    Mersenne61, Mersenne127 and both secp256k1 fields: five consecutive double sharings off the seed "hm fixture" --
            r = FF::random(prg), lo = shamirSecretShare(r, t, n, prg), hi = shamirSecretShare(r, 2t, n, prg) on ONE prg -- at
            (n, t) in {(3,1), (4,1), (7,3), (10,3), (9,4)}, and at (4,1) once more after a burn of three blocks, which pins
            counter0; the harness requires that both sharings recover r
  protocol  Mersenne61 at (4,1) and (10,3), secp256k1 order at (4,1): n dealers with the seeds "dealer 0".. deal three double
            sharings each; M = hyperInvertible(n-t, n) is applied with Matrix::multiply to the n x n matrix (dealer, party) of every
            sharing index s, at both degrees: R_lo / R_hi [k][s][party]; product p = 3k + s takes x, y = FF::random and their
            degree-t sharings from the PRG "hm inputs" (x, y, shares of x, shares of y, product after product; the shares are
            not kept: d pins them); every party's d = xs ys + R_hi, the opened d, every z = d - R_lo and the recovered z, which the harness requires to be x y
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
SEED = "hm fixture"
HIM = [(1, 1), (3, 4), (4, 4), (7, 10)]
DOUBLE_NT = [(3, 1), (4, 1), (7, 3), (10, 3), (9, 4)]
FIELDS = ["m61", "m127", "secp256k1_scalar", "secp256k1_field"]
PROTOCOL = [("m61", 4, 1), ("m61", 10, 3), ("secp256k1_scalar", 4, 1)]
COUNT = 5
BURN = 3
PER_DEALER = 3

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ff.h"
#include "scl/math/fp.h"
#include "scl/math/matrix.h"
#include "scl/ss/shamir.h"
#include "scl/util/prg.h"

using namespace scl;

static const char* SEED = "hm fixture";
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
static void him(const char* field, std::size_t m, std::size_t n, bool first) {
  const auto h = math::Matrix<T>::hyperInvertible(m, n);
  std::vector<T> flat;
  for (std::size_t i = 0; i < m; ++i)
    for (std::size_t j = 0; j < n; ++j) flat.push_back(h(i, j));
  std::printf("%s\n{\"field\":\"%s\",\"m\":%zu,\"n\":%zu,", first ? "" : ",", field, m, n);
  elems("rows", flat, "}");
}
template <typename T>
static void hims(const char* field, bool first) {
  const std::size_t mn[4][2] = {{1, 1}, {3, 4}, {4, 4}, {7, 10}};
  for (auto& c : mn) {
    him<T>(field, c[0], c[1], first);
    first = false;
  }
}
template <typename T>
static void double_run(const char* field, std::size_t n, std::size_t t, std::size_t burn, bool first) {
  auto prg = util::PRG::create(SEED);
  if (burn) {
    std::vector<unsigned char> buf(16 * burn);
    prg.next(buf.data(), buf.size());
  }
  std::printf("%s\n{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"seed\":\"%s\",\"burn\":%zu,\"sharings\":[", first ? "" : ",", field, n, t, SEED, burn);
  for (int k = 0; k < 5; ++k) {
    const T r = T::random(prg);
    const auto lo = ss::shamirSecretShare(r, t, n, prg);
    const auto hi = ss::shamirSecretShare(r, 2 * t, n, prg);
    must(ss::shamirRecoverP(lo) == r && ss::shamirRecoverP(hi) == r, "both sharings recover r");
    std::printf("%s{", k ? "," : "");
    elems("lo", vec(lo), ",");
    elems("hi", vec(hi), "}");
  }
  std::printf("]}");
}
template <typename T>
static void double_runs(const char* field, bool first) {
  const std::size_t nt[5][2] = {{3, 1}, {4, 1}, {7, 3}, {10, 3}, {9, 4}};
  for (auto& c : nt) {
    double_run<T>(field, c[0], c[1], 0, first);
    first = false;
  }
  double_run<T>(field, 4, 1, 3, false);
}
template <typename T>
static void protocol(const char* field, std::size_t n, std::size_t t, bool first) {
  const std::size_t S = 3, m = n - t;
  // lo[i][s][j]: dealer i, sharing s, party j
  std::vector<std::vector<std::vector<T>>> lo(n), hi(n);
  std::printf("%s\n{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"dealers\":[", first ? "" : ",", field, n, t);
  for (std::size_t i = 0; i < n; ++i) {
    const std::string seed = "dealer " + std::to_string(i);
    auto prg = util::PRG::create(seed);
    std::printf("%s{\"seed\":\"%s\",\"sharings\":[", i ? "," : "", seed.c_str());
    for (std::size_t s = 0; s < S; ++s) {
      const T r = T::random(prg);
      lo[i].push_back(vec(ss::shamirSecretShare(r, t, n, prg)));
      hi[i].push_back(vec(ss::shamirSecretShare(r, 2 * t, n, prg)));
      std::printf("%s{", s ? "," : "");
      elems("lo", lo[i][s], ",");
      elems("hi", hi[i][s], "}");
    }
    std::printf("]}");
  }
  const auto M = math::Matrix<T>::hyperInvertible(m, n);  // (an entry of `him`)
  std::printf("],");
  // Rlo[k][s][j]
  std::vector<std::vector<std::vector<T>>> Rlo(m, std::vector<std::vector<T>>(S)), Rhi = Rlo;
  for (std::size_t s = 0; s < S; ++s) {
    math::Matrix<T> X(n, n), Y(n, n);
    for (std::size_t i = 0; i < n; ++i)
      for (std::size_t j = 0; j < n; ++j) X(i, j) = lo[i][s][j], Y(i, j) = hi[i][s][j];
    const auto A = M.multiply(X), B = M.multiply(Y);
    for (std::size_t k = 0; k < m; ++k)
      for (std::size_t j = 0; j < n; ++j) Rlo[k][s].push_back(A(k, j)), Rhi[k][s].push_back(B(k, j));
  }
  auto dump3 = [&](const char* key, const std::vector<std::vector<std::vector<T>>>& R) {
    std::printf("\"%s\":[", key);
    for (std::size_t k = 0; k < R.size(); ++k) {
      std::printf("%s[", k ? "," : "");
      for (std::size_t s = 0; s < R[k].size(); ++s) {
        std::printf("%s{", s ? "," : "");
        elems("v", R[k][s], "}");
      }
      std::printf("]");
    }
    std::printf("],");
  };
  dump3("R_lo", Rlo);
  dump3("R_hi", Rhi);
  auto in = util::PRG::create("hm inputs");
  std::vector<T> xv, yv, dv, zv;
  std::printf("\"products\":[");
  for (std::size_t k = 0; k < m; ++k)
    for (std::size_t s = 0; s < S; ++s) {
      const T x = T::random(in);
      const T y = T::random(in);
      const auto xs = vec(ss::shamirSecretShare(x, t, n, in));
      const auto ys = vec(ss::shamirSecretShare(y, t, n, in));
      std::vector<T> d, z;
      for (std::size_t j = 0; j < n; ++j) d.push_back(xs[j] * ys[j] + Rhi[k][s][j]);
      const T opened = ss::shamirRecoverP(math::Vector<T>(d));
      for (std::size_t j = 0; j < n; ++j) z.push_back(opened - Rlo[k][s][j]);
      const T zz = ss::shamirRecoverP(math::Vector<T>(z));
      must(zz == x * y, "z = x y");
      must(ss::shamirRecoverP(math::Vector<T>(Rlo[k][s])) == ss::shamirRecoverP(math::Vector<T>(Rhi[k][s])), "extracted double sharing");
      std::printf("%s{", (k || s) ? "," : "");
      elems("d_shares", d, ",");
      elems("z_shares", z, "}");
      xv.push_back(x), yv.push_back(y), dv.push_back(opened), zv.push_back(zz);
    }
  std::printf("],");
  elems("x", xv, ",");
  elems("y", yv, ",");
  elems("d", dv, ",");
  elems("z", zv, "}");
}

int main() {
  using F61 = math::Fp<61>;
  using F127 = math::Fp<127>;
  using Scalar = math::FF<math::ff::Secp256k1Scalar>;
  using Field = math::FF<math::ff::Secp256k1Field>;
  std::printf("{\"him\":[");
  hims<F61>("m61", true);
  hims<F127>("m127", false);
  hims<Scalar>("secp256k1_scalar", false);
  hims<Field>("secp256k1_field", false);
  std::printf("],\n\"double\":[");
  double_runs<F61>("m61", true);
  double_runs<F127>("m127", false);
  double_runs<Scalar>("secp256k1_scalar", false);
  double_runs<Field>("secp256k1_field", false);
  std::printf("],\n\"protocol\":[");
  protocol<F61>("m61", 4, 1, true);
  protocol<F61>("m61", 10, 3, false);
  protocol<Scalar>("secp256k1_scalar", 4, 1, false);
  std::printf("]}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_hm_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    d = json.loads(out)
    assert [(r["field"], r["m"], r["n"]) for r in d["him"]] == [(f, m, n) for f in FIELDS for m, n in HIM]
    assert [(r["field"], r["n"], r["t"], r["burn"]) for r in d["double"]] == \
        [(f, n, t, b) for f in FIELDS for n, t, b in [(n, t, 0) for n, t in DOUBLE_NT] + [(4, 1, BURN)]]
    for r in d["double"]:
        assert r["seed"] == SEED and len(r["sharings"]) == COUNT and all(len(s[k]) == r["n"] for s in r["sharings"] for k in ("lo", "hi"))
    assert [(r["field"], r["n"], r["t"]) for r in d["protocol"]] == PROTOCOL
    for r in d["protocol"]:
        assert len(r["dealers"]) == r["n"] and len(r["products"]) == PER_DEALER * (r["n"] - r["t"]) == len(r["z"])
    head = {"generator": "tests/golden/make_golden_hm.py",
            "source": "the reference's ss::shamirSecretShare, ss::shamirRecoverP, Matrix::hyperInvertible, Matrix::multiply and util::PRG; "
                      "elements are FF::write images (byteSize bytes, in hex)"}
    path = os.path.join(HERE, "golden_hm.json")
    with open(path, "w") as fh:       # the harness's own line structure: one run per line
        fh.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"data":' + out.strip() + "}\n")
    with open(path) as fh:
        assert json.load(fh)["data"] == d
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
