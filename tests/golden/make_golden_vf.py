#!/usr/bin/env python3
"""Generate tests/golden/golden_vf.json from the REAL reference: random linear combinations of sharings along N (batch
verification), built from its Vector::random, math::innerProd, ss::shamirSecretShare, ss::shamirRecoverD / P and util::PRG.

This script writes a small harness of its own against the reference's headers, compiles it with the reference's field and PRG
translation units into a temporary directory OUTSIDE the repository, runs it and keeps what it prints.  Elements are their
FF::write images (byteSize bytes, in hex).  Nothing compiled is kept.  Run in the build container only:

    python tests/golden/make_golden_vf.py

Contents (Mersenne61, Mersenne127 and the secp256k1 order).  THE COIN everywhere: a util::PRG seeded "vf coin" from which
Vector::random(3) is drawn and discarded first, so that it stands at block counter0 = ceil(3 byteSize / 16) (recorded); then
one Vector::random(N) per repetition.
  combine   3 rows: x = three consecutive Vector::random(5) off the PRG "vf inputs", y three off "vf inputs y".  Per N in
            {1, 2, 5} the operands are the first N columns of every row (rows 5 apart: a stride above N) and the coin is drawn
            afresh as two Vector::random(N).  Recorded: x, y; per N counter0, plain[r][j] = innerProd(rho_j, x_r) and
            product[r][j] = innerProd(rho_j, x_r .* y_r) for j < 2 -- reps = 1 is column 0
  degree    (n, t) = (4, 1), N = 5.  secrets = Vector::random(5) off "vf secrets", shared one after the other with
            shamirSecretShare off ONE PRG "vf sharing"; reps = 1.  Recorded: the secrets, every party's combined share (it
            pins the shares), and shamirRecoverD(combined, 1..4, 3, 1, 0) -- the first two shares define the line, shares 3 and 4
            are checked -- which the harness requires to equal innerProd(rho, secrets).  Then party `party`'s share of column
            `column` is altered (+1): the harness requires the same call to throw "error detected during recovery"
  product   (4, 1), N = 5 triples: a, b = Vector::random(5) off "vf a" / "vf b", c = a .* b, shared off "vf share a" / "vf share
            b" / "vf share c".  Every party's v = innerProd(rho, a_i .* b_i) - innerProd(rho, c_i) is a degree-2 sharing of 0:
            the harness requires shamirRecoverP over all 4 shares to give 0.  With delta added to every party's share of c's
            column `column` it requires the recovered value to be -rho[column] * delta, which is not 0 (recorded as `off`)
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
NS = [1, 2, 5]
REPS = [1, 2]

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ff.h"
#include "scl/math/fp.h"
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
static void elems(const char* key, const math::Vector<T>& v, const char* tail) {
  std::printf("\"%s\":[", key);
  for (std::size_t i = 0; i < v.size(); ++i) std::printf("%s\"%s\"", i ? "," : "", image(v[i]).c_str());
  std::printf("]%s", tail);
}
template <typename T>
static void rows(const char* key, const std::vector<math::Vector<T>>& m, const char* tail) {
  std::printf("\"%s\":[", key);
  for (std::size_t r = 0; r < m.size(); ++r) {
    std::printf("%s[", r ? "," : "");
    for (std::size_t i = 0; i < m[r].size(); ++i) std::printf("%s\"%s\"", i ? "," : "", image(m[r][i]).c_str());
    std::printf("]");
  }
  std::printf("]%s", tail);
}
template <typename T>
static T dot(const math::Vector<T>& a, const math::Vector<T>& b) {
  return math::innerProd<T>(a.begin(), a.end(), b.begin());
}
// the coin: "vf coin" after Vector::random(3) was drawn and discarded; *counter0 = the blocks that took
template <typename T>
static util::PRG coin(std::size_t* counter0) {
  auto prg = util::PRG::create("vf coin");
  (void)math::Vector<T>::random(3, prg);
  *counter0 = (3 * T::byteSize() + 15) / 16;
  return prg;
}

template <typename T>
static void combine(const char* field, bool first) {
  const std::size_t NMAX = 5;
  auto px = util::PRG::create("vf inputs");
  auto py = util::PRG::create("vf inputs y");
  std::vector<math::Vector<T>> x, y;
  for (int r = 0; r < 3; ++r) x.push_back(math::Vector<T>::random(NMAX, px)), y.push_back(math::Vector<T>::random(NMAX, py));
  std::printf("%s\n{\"field\":\"%s\",", first ? "" : ",", field);
  rows("x", x, ",");
  rows("y", y, ",");
  std::printf("\"runs\":[");
  bool f1 = true;
  for (std::size_t N : {1, 2, 5}) {
    std::size_t counter0 = 0;
    auto pc = coin<T>(&counter0);
    std::vector<math::Vector<T>> rho, plain, product;
    for (std::size_t j = 0; j < 2; ++j) rho.push_back(math::Vector<T>::random(N, pc));
    for (int r = 0; r < 3; ++r) {
      const auto xr = x[r].subVector(0, N), yr = y[r].subVector(0, N);
      std::vector<T> p, q;
      for (std::size_t j = 0; j < 2; ++j) {
        p.push_back(dot(rho[j], xr));
        q.push_back(dot(rho[j], xr.multiplyEntryWise(yr)));
      }
      plain.push_back(math::Vector<T>(p)), product.push_back(math::Vector<T>(q));
    }
    std::printf("%s\n {\"N\":%zu,\"counter0\":%zu,", f1 ? "" : ",", N, counter0);
    f1 = false;
    rows("plain", plain, ",");
    rows("product", product, "}");
  }
  std::printf("]}");
}

template <typename T>
static void degree(const char* field, bool first) {
  const std::size_t n = 4, t = 1, N = 5, column = 3, party = 2;
  auto ps = util::PRG::create("vf secrets");
  const auto secrets = math::Vector<T>::random(N, ps);
  auto sharing = util::PRG::create("vf sharing");
  std::vector<math::Vector<T>> shares;  // [column][party]
  for (std::size_t s = 0; s < N; ++s) shares.push_back(ss::shamirSecretShare(secrets[s], t, n, sharing));
  std::size_t counter0 = 0;
  auto pc = coin<T>(&counter0);
  const auto rho = math::Vector<T>::random(N, pc);
  const auto alphas = math::Vector<T>::range(1, n + 1);
  auto fold = [&](const std::vector<math::Vector<T>>& sh) {
    std::vector<T> c;
    for (std::size_t i = 0; i < n; ++i) {
      std::vector<T> mine;
      for (std::size_t s = 0; s < N; ++s) mine.push_back(sh[s][i]);
      c.push_back(dot(rho, math::Vector<T>(mine)));
    }
    return math::Vector<T>(c);
  };
  const auto combined = fold(shares);
  const T opened = ss::shamirRecoverD(combined, alphas, n - t, t, T{});
  must(opened == dot(rho, secrets), "the combination opens to sum rho secret");
  auto bad = shares;
  bad[column][party] = bad[column][party] + T(1);
  const auto combined_bad = fold(bad);
  bool thrown = false;
  try {
    (void)ss::shamirRecoverD(combined_bad, alphas, n - t, t, T{});
  } catch (const std::logic_error& e) {
    thrown = std::string(e.what()) == "error detected during recovery";
  }
  must(thrown, "the altered share is detected");
  std::printf("%s\n{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"N\":%zu,\"counter0\":%zu,\"column\":%zu,\"party\":%zu,", first ? "" : ",", field, n, t, N,
              counter0, column, party);
  elems("secrets", secrets, ",");
  elems("combined", combined, ",");
  std::printf("\"opened\":\"%s\",", image(opened).c_str());
  elems("combined_bad", combined_bad, "}");
}

template <typename T>
static void product(const char* field, bool first) {
  const std::size_t n = 4, t = 1, N = 5, column = 1;
  auto pa = util::PRG::create("vf a");
  auto pb = util::PRG::create("vf b");
  const auto a = math::Vector<T>::random(N, pa), b = math::Vector<T>::random(N, pb);
  const auto c = a.multiplyEntryWise(b);
  auto sa = util::PRG::create("vf share a");
  auto sb = util::PRG::create("vf share b");
  auto sc = util::PRG::create("vf share c");
  std::vector<math::Vector<T>> as, bs, cs;  // [column][party]
  for (std::size_t s = 0; s < N; ++s) {
    as.push_back(ss::shamirSecretShare(a[s], t, n, sa));
    bs.push_back(ss::shamirSecretShare(b[s], t, n, sb));
    cs.push_back(ss::shamirSecretShare(c[s], t, n, sc));
  }
  std::size_t counter0 = 0;
  auto pc = coin<T>(&counter0);
  const auto rho = math::Vector<T>::random(N, pc);
  const T delta = T(5);
  auto fold = [&](bool off) {
    std::vector<T> v;
    for (std::size_t i = 0; i < n; ++i) {
      std::vector<T> ai, bi, ci;
      for (std::size_t s = 0; s < N; ++s) {
        ai.push_back(as[s][i]), bi.push_back(bs[s][i]);
        ci.push_back(off && s == column ? cs[s][i] + delta : cs[s][i]);
      }
      v.push_back(dot(rho, math::Vector<T>(ai).multiplyEntryWise(math::Vector<T>(bi))) - dot(rho, math::Vector<T>(ci)));
    }
    return math::Vector<T>(v);
  };
  const auto good = fold(false), bad = fold(true);
  must(ss::shamirRecoverP(good) == T{}, "the honest triples combine to a sharing of 0");
  const T off = ss::shamirRecoverP(bad);
  must(off == T{} - rho[column] * delta && !(off == T{}), "the altered triple combines to -rho delta, not 0");
  std::printf("%s\n{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"N\":%zu,\"counter0\":%zu,\"column\":%zu,\"delta\":\"%s\",", first ? "" : ",", field, n, t, N,
              counter0, column, image(delta).c_str());
  elems("a", a, ",");
  elems("b", b, ",");
  elems("v", good, ",");
  elems("v_bad", bad, ",");
  std::printf("\"off\":\"%s\"}", image(off).c_str());
}

int main() {
  using F61 = math::Fp<61>;
  using F127 = math::Fp<127>;
  using Scalar = math::FF<math::ff::Secp256k1Scalar>;
  std::printf("{\"combine\":[");
  combine<F61>("m61", true);
  combine<F127>("m127", false);
  combine<Scalar>("secp256k1_scalar", false);
  std::printf("],\n\"degree\":[");
  degree<F61>("m61", true);
  degree<F127>("m127", false);
  degree<Scalar>("secp256k1_scalar", false);
  std::printf("],\n\"product\":[");
  product<F61>("m61", true);
  product<F127>("m127", false);
  product<Scalar>("secp256k1_scalar", false);
  std::printf("]}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_vf_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    d = json.loads(out)
    assert [r["field"] for r in d["combine"]] == FIELDS
    for r in d["combine"]:
        assert len(r["x"]) == len(r["y"]) == 3 and all(len(v) == max(NS) for v in r["x"] + r["y"]) and [q["N"] for q in r["runs"]] == NS
        for q in r["runs"]:
            assert q["counter0"] > 0 and len(q["plain"]) == len(q["product"]) == 3 and all(len(v) == max(REPS) for v in q["plain"] + q["product"])
    assert [r["field"] for r in d["degree"]] == [r["field"] for r in d["product"]] == FIELDS
    head = {"generator": "tests/golden/make_golden_vf.py",
            "source": "the reference's Vector::random, math::innerProd, ss::shamirSecretShare, ss::shamirRecoverD / P and util::PRG; "
                      "elements are FF::write images (byteSize bytes, in hex)"}
    path = os.path.join(HERE, "golden_vf.json")
    with open(path, "w") as fh:       # the harness's own line structure: one run per line
        fh.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"data":' + out.strip() + "}\n")
    with open(path) as fh:
        assert json.load(fh)["data"] == d
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
