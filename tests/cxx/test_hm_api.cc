// tests/cxx/test_hm_api.cc -- honest-majority multiplication in the C++ mirror: ss::doubleShare (include/scl_hip/ss/double_share.h),
// Matrix::hyperInvertible and the per-element forms of include/scl_hip/detail/hm.hpp on the host, hip::dealDoubleSharings,
// hip::applyMatrix, hip::mulMask and hip::mulFinish (include/scl_hip/hip/hm.h) on the GPU.
//
//   test_hm_api --host   the contents of tests/golden/golden_hm.json (the same seeds, burns and shapes), printed in the fixture's
//                        layout -- tests/test_hm_host.py compares the two: the matrices by Matrix::hyperInvertible, the double
//                        sharings by ss::doubleShare, and the protocol runs with the extraction through hm_mac_step, every d share
//                        through hm_mask_one and every z share through hm_finish_one, on the elements' limbs.  Needs no GPU; also
//                        built with -fsanitize=address,undefined.
//   test_hm_api --gpu    N double sharings dealt on the device equal N per-secret calls on one PRG, element for element, and the
//                        PRG ends at the same counter; deal x n -> extract at both degrees -> mask -> finish -> recover multiplies.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/detail/hm.hpp>
#include <scl_hip/hip/hm.h>
#include <scl_hip/ss/double_share.h>

#include "check.hpp"

using namespace scl;

static const char* SEED = "hm fixture";

template <typename T>
static void hims(const char* field, bool first) {
  const std::size_t mn[4][2] = {{1, 1}, {3, 4}, {4, 4}, {7, 10}};
  for (auto& c : mn) {
    const auto h = hip::hyperInvertible<T>(c[0], c[1]);
    std::vector<T> flat;
    for (std::size_t i = 0; i < c[0]; ++i)
      for (std::size_t j = 0; j < c[1]; ++j) flat.push_back(h(i, j));
    std::printf("%s{\"field\":\"%s\",\"m\":%zu,\"n\":%zu,", first ? "" : ",", field, c[0], c[1]);
    elems("rows", flat, "}");
    first = false;
  }
}

template <typename T>
static void double_run(const char* field, std::size_t n, std::size_t t, std::size_t burn, bool first) {
  auto prg = util::PRG::create(SEED);
  if (burn) (void)prg.next(16 * burn);
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"seed\":\"%s\",\"burn\":%zu,\"sharings\":[", first ? "" : ",", field, n, t, SEED, burn);
  for (int k = 0; k < 5; ++k) {
    const std::uint64_t before = prg.counter();
    const auto ds = ss::doubleShare<T>(t, n, prg);
    REQUIRE(ds.lo.size() == n && ds.hi.size() == n && prg.counter() - before == hip::doubleBlocks<T>(n, t));
    REQUIRE(ss::shamirRecoverP(math::Vector<T>(ds.lo)) == ss::shamirRecoverP(math::Vector<T>(ds.hi)));
    std::printf("%s{", k ? "," : "");
    elems("lo", ds.lo, ",");
    elems("hi", ds.hi, "}");
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

template <typename T, class F>
static void protocol(const char* field, std::size_t n, std::size_t t, bool first) {
  const typename F::Ctx ctx{};
  const std::size_t S = 3, m = n - t;
  std::vector<std::vector<ss::DoubleSharing<T>>> deals(n);  // [dealer][sharing]
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"dealers\":[", first ? "" : ",", field, n, t);
  for (std::size_t i = 0; i < n; ++i) {
    const std::string seed = "dealer " + std::to_string(i);
    auto prg = util::PRG::create(seed);
    std::printf("%s{\"seed\":\"%s\",\"sharings\":[", i ? "," : "", seed.c_str());
    for (std::size_t s = 0; s < S; ++s) {
      deals[i].push_back(ss::doubleShare<T>(t, n, prg));
      std::printf("%s{", s ? "," : "");
      elems("lo", deals[i][s].lo, ",");
      elems("hi", deals[i][s].hi, "}");
    }
    std::printf("]}");
  }
  const auto M = hip::hyperInvertible<T>(m, n);
  std::printf("],");
  // the extraction, party by party: row k of M against the n shares party j received, by the inner step of apply
  std::vector<std::vector<std::vector<T>>> Rlo(m, std::vector<std::vector<T>>(S)), Rhi = Rlo;
  for (std::size_t k = 0; k < m; ++k)
    for (std::size_t s = 0; s < S; ++s)
      for (std::size_t j = 0; j < n; ++j) {
        typename F::Acc lo = F::acc_zero(), hi = F::acc_zero();
        int tl = 0, th = 0;
        for (std::size_t i = 0; i < n; ++i) {
          sclhip::hm_mac_step<F>(ctx, lo, tl, limbs<T, F>(M(k, i)), limbs<T, F>(deals[i][s].lo[j]));
          sclhip::hm_mac_step<F>(ctx, hi, th, limbs<T, F>(M(k, i)), limbs<T, F>(deals[i][s].hi[j]));
        }
        Rlo[k][s].push_back(element<T, F>(F::acc_fold(ctx, lo)));
        Rhi[k][s].push_back(element<T, F>(F::acc_fold(ctx, hi)));
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
  const auto lambda = math::computeLagrangeBasis(math::Vector<T>::range(1, n + 1), T{});
  std::vector<T> xv, yv, dv, zv;
  std::printf("\"products\":[");
  for (std::size_t k = 0; k < m; ++k)
    for (std::size_t s = 0; s < S; ++s) {
      const T x = T::random(in);
      const T y = T::random(in);
      const auto xs = ss::shamirSecretShare(x, t, n, in), ys = ss::shamirSecretShare(y, t, n, in);
      std::vector<T> d, z;
      typename F::Acc open = F::acc_zero();
      int terms = 0;
      for (std::size_t j = 0; j < n; ++j) {
        const auto dj = sclhip::hm_mask_one<F>(ctx, limbs<T, F>(xs[j]), limbs<T, F>(ys[j]), limbs<T, F>(Rhi[k][s][j]));
        d.push_back(element<T, F>(dj));
        sclhip::hm_mac_step<F>(ctx, open, terms, limbs<T, F>(lambda[j]), dj);
      }
      const auto opened = F::acc_fold(ctx, open);
      for (std::size_t j = 0; j < n; ++j) z.push_back(element<T, F>(sclhip::hm_finish_one<F>(ctx, opened, limbs<T, F>(Rlo[k][s][j]))));
      const T zz = ss::shamirRecoverP(math::Vector<T>(z));
      REQUIRE(zz == x * y);
      REQUIRE(element<T, F>(opened) == ss::shamirRecoverP(math::Vector<T>(d)));
      std::printf("%s{", (k || s) ? "," : "");
      elems("d_shares", d, ",");
      elems("z_shares", z, "}");
      xv.push_back(x), yv.push_back(y), dv.push_back(element<T, F>(opened)), zv.push_back(zz);
    }
  std::printf("],");
  elems("x", xv, ",");
  elems("y", yv, ",");
  elems("d", dv, ",");
  elems("z", zv, "}");
}

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;
using Field = math::FF<math::ff::Secp256k1Field>;

static int host() {
  std::printf("{\"him\":[");
  hims<F61>("m61", true);
  hims<F127>("m127", false);
  hims<Scalar>("secp256k1_scalar", false);
  hims<Field>("secp256k1_field", false);
  std::printf("],\"double\":[");
  double_runs<F61>("m61", true);
  double_runs<F127>("m127", false);
  double_runs<Scalar>("secp256k1_scalar", false);
  double_runs<Field>("secp256k1_field", false);
  std::printf("],\"protocol\":[");
  protocol<F61, sclhip::M61>("m61", 4, 1, true);
  protocol<F61, sclhip::M61>("m61", 10, 3, false);
  protocol<Scalar, sclhip::Secp256k1Scalar>("secp256k1_scalar", 4, 1, false);
  std::printf("]}\n");
  return summary(stderr);
}

// ---- on the device -----------------------------------------------------------------------------------------------------------
template <typename T>
static void device_equals_host(const char* name, std::size_t N, std::size_t n, std::size_t t) {
  auto dprg = util::PRG::create(std::string("hm gpu ") + name), hprg = util::PRG::create(std::string("hm gpu ") + name);
  (void)dprg.next(32);  // both start two blocks in
  (void)hprg.next(32);
  const auto dev = hip::dealDoubleSharings<T>(N, t, n, dprg);
  bool same = dev.lo.parties() == n && dev.hi.parties() == n && dev.lo.secrets() == N;
  for (std::size_t s = 0; same && s < N; ++s) {
    const auto ds = ss::doubleShare<T>(t, n, hprg);
    same = dev.lo.sharesOf(s) == ds.lo && dev.hi.sharesOf(s) == ds.hi;
  }
  REQUIRE(same);
  REQUIRE(dprg.counter() == hprg.counter());
  std::printf("%s: %zu double sharings, n = %zu, t = %zu, equal the per-secret calls\n", name, N, n, t);
}

// one party's view is enough to multiply inside one process: party j's input to the extraction is row j of every dealer's
// matrices, so the n x n products are taken party by party with the batch-of-one form of hip::applyMatrix
template <typename T>
static void multiply(const char* name, std::size_t N, std::size_t n, std::size_t t) {
  const std::size_t m = n - t, L = hip::DeviceVector<T>::LIMBS;
  std::vector<hip::DoubleSharings<T>> deals;
  for (std::size_t i = 0; i < n; ++i) {
    auto prg = util::PRG::create(std::string("hm dealer ") + name + std::to_string(i));
    deals.push_back(hip::dealDoubleSharings<T>(N, t, n, prg));
  }
  const auto M = hip::uploadMatrix(hip::hyperInvertible<T>(m, n));
  // R[j]: the m x N extracted shares of party j; product p = k N + s
  hip::ShareMatrix<T> rlo(n, m * N), rhi(n, m * N);
  for (std::size_t j = 0; j < n; ++j)
    for (int deg = 0; deg < 2; ++deg) {
      hip::ShareMatrix<T> in(n, N);  // row i = what dealer i sent party j
      for (std::size_t i = 0; i < n; ++i)
        hip::check(scl_hip_stream_copy(in.data() + i * N * L, (deg ? deals[i].hi : deals[i].lo).row(j), N * L * 8, nullptr));
      const auto out = hip::applyMatrix(M, m, in);
      hip::check(scl_hip_stream_copy((deg ? rhi : rlo).data() + j * m * N * L, out.data(), m * N * L * 8, nullptr));
      hip::check(scl_hip_stream_sync(nullptr));
    }
  const std::size_t P = m * N;
  auto sprg = util::PRG::create(std::string("hm secrets ") + name), prg = util::PRG::create(std::string("hm shares ") + name);
  std::vector<T> x, y, want;
  for (std::size_t p = 0; p < P; ++p) {
    x.push_back(T::random(sprg));
    y.push_back(T::random(sprg));
    want.push_back(x[p] * y[p]);
  }
  const hip::ShareMatrix<T> xs = ss::shamirSecretShare(hip::DeviceVector<T>(x), t, n, prg), ys = ss::shamirSecretShare(hip::DeviceVector<T>(y), t, n, prg);
  const auto d = hip::mulMask(xs, ys, rhi);
  const hip::ShareMatrix<T> z = hip::mulFinish(d, rlo);
  const auto got = ss::shamirRecoverP(z).toHost();
  bool same = got.size() == P;
  for (std::size_t p = 0; same && p < P; ++p) same = got[p] == want[p];
  REQUIRE(same);
  std::printf("%s: deal x %zu, extract, mask, finish, recover multiplies %zu secrets (n = %zu, t = %zu)\n", name, n, P, n, t);
}

static int gpu() {
  device_equals_host<F61>("Mersenne61", 67, 10, 3);
  device_equals_host<F127>("Mersenne127", 33, 7, 3);
  device_equals_host<Scalar>("secp256k1_order", 33, 4, 1);  // two-pass: the scratch is the call's own
  device_equals_host<F61>("Mersenne61", 33, 9, 4);           // two-pass
  multiply<F61>("Mersenne61", 38, 10, 3);  // (scl_hip_stream_copy moves 16-byte units: an even N for one-limb rows)
  multiply<Scalar>("secp256k1_order", 9, 4, 1);
  return summary();
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--host")) return host();
  if (argc == 2 && !std::strcmp(argv[1], "--gpu")) {
    try {
      return gpu();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "FAILED: %s\n", e.what());
      return 1;
    }
  }
  std::fprintf(stderr, "usage: test_hm_api --host | --gpu\n");
  return 2;
}
