// tests/cxx/test_ip_api.cc -- inner and matrix products of Shamir sharings at one opening in the C++ mirror: the per-element form of
// include/scl_hip/detail/ip.hpp on the host, hip::dotMask and hip::matmulMask (include/scl_hip/hip/ip.h) on the GPU.
//
//   test_ip_api --host   the contents of tests/golden/golden_ip.json (the same seeds and shapes), printed in the fixture's layout
//                        -- tests/test_ip_host.py compares the two: the inputs by ss::shamirSecretShare on one util::PRG, [R] by
//                        ss::doubleShare, every d share through ip_dot_one, the open through hm_mac_step and every z share through
//                        hm_finish_one, on the elements' limbs.  Needs no GPU.
//   test_ip_api --gpu    hip::dotMask and hip::matmulMask equal ip_dot_one on the host, element for element, with and without
//                        the addend (65 terms pass Mersenne61's bound); share -> dotMask -> hip::mulFinish -> recover is the
//                        inner product of the secrets.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/detail/ip.hpp>
#include <scl_hip/hip/hm.h>
#include <scl_hip/hip/ip.h>
#include <scl_hip/ss/double_share.h>

#include "check.hpp"

using namespace scl;

template <typename T>
struct Inputs {
  std::vector<T> x, y;
  std::vector<math::Vector<T>> xs, ys;  // [pair][party]
};
template <typename T>
static Inputs<T> inputs(const char* seed, std::size_t pairs, std::size_t n, std::size_t t) {
  auto prg = util::PRG::create(seed);
  Inputs<T> in;
  for (std::size_t k = 0; k < pairs; ++k) {
    const T x = T::random(prg);
    const T y = T::random(prg);
    in.xs.push_back(ss::shamirSecretShare(x, t, n, prg));
    in.ys.push_back(ss::shamirSecretShare(y, t, n, prg));
    in.x.push_back(x), in.y.push_back(y);
  }
  return in;
}

// one opening: d_j = sum over the listed pairs of xs[xi][j] ys[yi][j] + hi[j] by ip_dot_one; z_j = open(d) - lo[j]
template <typename T, class F>
static T one_opening(const Inputs<T>& in, const std::vector<std::size_t>& xi, const std::vector<std::size_t>& yi, const ss::DoubleSharing<T>& R,
                     std::size_t n, const char* tail) {
  const typename F::Ctx ctx{};
  const auto lambda = math::computeLagrangeBasis(math::Vector<T>::range(1, n + 1), T{});
  std::vector<T> d, z;
  typename F::Acc open = F::acc_zero();
  int terms = 0;
  for (std::size_t j = 0; j < n; ++j) {
    std::vector<typename F::E> xv, yv;
    for (std::size_t k = 0; k < xi.size(); ++k) xv.push_back(limbs<T, F>(in.xs[xi[k]][j])), yv.push_back(limbs<T, F>(in.ys[yi[k]][j]));
    const typename F::E r2 = limbs<T, F>(R.hi[j]);
    const auto dj = sclhip::ip_dot_one<F>(ctx, xv.data(), 1, yv.data(), 1, xv.size(), &r2);
    d.push_back(element<T, F>(dj));
    sclhip::hm_mac_step<F>(ctx, open, terms, limbs<T, F>(lambda[j]), dj);
  }
  const auto opened = F::acc_fold(ctx, open);
  for (std::size_t j = 0; j < n; ++j) z.push_back(element<T, F>(sclhip::hm_finish_one<F>(ctx, opened, limbs<T, F>(R.lo[j]))));
  const T zz = ss::shamirRecoverP(math::Vector<T>(z));
  REQUIRE(element<T, F>(opened) == ss::shamirRecoverP(math::Vector<T>(d)));
  std::printf("{");
  elems("d_shares", d, ",");
  std::printf("\"d\":\"%s\",", image(element<T, F>(opened)).c_str());
  elems("z_shares", z, ",");
  std::printf("\"z\":\"%s\"}%s", image(zz).c_str(), tail);
  return zz;
}

template <typename T, class F>
static void inner(const char* field, std::size_t n, std::size_t t, std::size_t K, bool first) {
  const Inputs<T> in = inputs<T>("ip inputs", K, n, t);
  auto dealer = util::PRG::create("ip dealer");
  const auto R = ss::doubleShare<T>(t, n, dealer);
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"K\":%zu,", first ? "" : ",", field, n, t, K);
  elems("x", in.x, ",");
  elems("y", in.y, ",");
  std::vector<std::size_t> idx;
  for (std::size_t k = 0; k < K; ++k) idx.push_back(k);
  std::printf("\"out\":");
  const T z = one_opening<T, F>(in, idx, idx, R, n, "}");
  T want{};
  for (std::size_t k = 0; k < K; ++k) want = want + in.x[k] * in.y[k];
  REQUIRE(z == want);
}
template <typename T, class F>
static void inners(const char* field, bool first) {
  const std::size_t nt[2][2] = {{4, 1}, {10, 3}};
  for (auto& c : nt)
    for (std::size_t K : {1, 3, 5}) {
      inner<T, F>(field, c[0], c[1], K, first);
      first = false;
    }
}
template <typename T, class F>
static void matrix(const char* field, bool first) {
  const std::size_t n = 4, t = 1, a = 2, K = 3, b = 2;
  const Inputs<T> in = inputs<T>("ip matrix", a * K, n, t);  // pair p: X's entry p and Y's entry p, both row-major
  auto dealer = util::PRG::create("ip dealer");
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"a\":%zu,\"K\":%zu,\"b\":%zu,", first ? "" : ",", field, n, t, a, K, b);
  elems("x", in.x, ",");
  elems("y", in.y, ",");
  std::printf("\"out\":[");
  for (std::size_t i = 0; i < a; ++i)
    for (std::size_t l = 0; l < b; ++l) {
      const auto R = ss::doubleShare<T>(t, n, dealer);
      std::vector<std::size_t> xi, yi;
      T want{};
      for (std::size_t k = 0; k < K; ++k) {
        xi.push_back(i * K + k), yi.push_back(k * b + l);
        want = want + in.x[i * K + k] * in.y[k * b + l];
      }
      const T z = one_opening<T, F>(in, xi, yi, R, n, (i + 1 == a && l + 1 == b) ? "" : ",");
      REQUIRE(z == want);
    }
  std::printf("]}");
}

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;

static int host() {
  std::printf("{\"inner\":[");
  inners<F61, sclhip::M61>("m61", true);
  inners<F127, sclhip::M127>("m127", false);
  inners<Scalar, sclhip::Secp256k1Scalar>("secp256k1_scalar", false);
  std::printf("],\"matrix\":[");
  matrix<F61, sclhip::M61>("m61", true);
  matrix<F127, sclhip::M127>("m127", false);
  matrix<Scalar, sclhip::Secp256k1Scalar>("secp256k1_scalar", false);
  std::printf("]}\n");
  return summary(stderr);
}

// ---- on the device -----------------------------------------------------------------------------------------------------------
template <typename T, class F>
static std::vector<typename F::E> download(const hip::ShareMatrix<T>& m) {
  constexpr std::size_t L = hip::DeviceVector<T>::LIMBS;
  std::vector<std::uint64_t> w(m.parties() * m.secrets() * L);
  hip::check(scl_hip_memcpy_d2h(w.data(), m.data(), w.size() * 8, nullptr));
  hip::check(scl_hip_stream_sync(nullptr));
  std::vector<typename F::E> out;
  for (std::size_t i = 0; i < m.parties() * m.secrets(); ++i) out.push_back(F::ld(w.data() + i * L));
  return out;
}

// `count` sharings of N secrets each, one after another in one matrix of count * n rows; the secrets are returned too
template <typename T>
static hip::ShareMatrix<T> share_rows(const std::string& seed, std::size_t count, std::size_t N, std::size_t n, std::size_t t,
                                      std::vector<std::vector<T>>* secrets) {
  constexpr std::size_t L = hip::DeviceVector<T>::LIMBS;
  auto sprg = util::PRG::create(seed + " secrets"), prg = util::PRG::create(seed + " shares");
  hip::ShareMatrix<T> all(count * n, N);
  for (std::size_t k = 0; k < count; ++k) {
    std::vector<T> s;
    for (std::size_t i = 0; i < N; ++i) s.push_back(T::random(sprg));
    const hip::ShareMatrix<T> sh = ss::shamirSecretShare(hip::DeviceVector<T>(s), t, n, prg);
    hip::check(scl_hip_stream_copy(all.data() + k * n * N * L, sh.data(), n * N * L * 8, nullptr));  // (16-byte units: an even N)
    hip::check(scl_hip_stream_sync(nullptr));
    secrets->push_back(s);
  }
  return all;
}

template <typename T, class F>
static void dot(const char* name, std::size_t terms, std::size_t N, std::size_t n, std::size_t t) {
  const typename F::Ctx ctx{};
  std::vector<std::vector<T>> x, y;
  const auto xs = share_rows<T>(std::string("ip gpu x ") + name, terms, N, n, t, &x), ys = share_rows<T>(std::string("ip gpu y ") + name, terms, N, n, t, &y);
  auto dealer = util::PRG::create(std::string("ip gpu dealer ") + name);
  const auto R = hip::dealDoubleSharings<T>(N, t, n, dealer);
  const auto hx = download<T, F>(xs), hy = download<T, F>(ys), hr = download<T, F>(R.hi);
  for (const hip::ShareMatrix<T>* r2 : {static_cast<const hip::ShareMatrix<T>*>(nullptr), &R.hi}) {
    const auto d = hip::dotMask(xs, ys, terms, r2);
    const auto hd = download<T, F>(d);
    bool same = d.parties() == n && d.secrets() == N;
    for (std::size_t j = 0; same && j < n; ++j)
      for (std::size_t s = 0; same && s < N; ++s)
        same = F::eq(hd[j * N + s], sclhip::ip_dot_one<F>(ctx, &hx[j * N + s], n * N, &hy[j * N + s], n * N, terms, r2 ? &hr[j * N + s] : nullptr));
    REQUIRE(same);
  }
  // the protocol: [z] = open([d]) - [R]_t recovers the inner products of the secrets
  const hip::ShareMatrix<T> z = hip::mulFinish(hip::dotMask(xs, ys, terms, &R.hi), R.lo);
  const auto got = ss::shamirRecoverP(z).toHost();
  bool same = got.size() == N;
  for (std::size_t s = 0; same && s < N; ++s) {
    T want{};
    for (std::size_t k = 0; k < terms; ++k) want = want + x[k][s] * y[k][s];
    same = got[s] == want;
  }
  REQUIRE(same);
  std::printf("%s: %zu terms, %zu inner products, n = %zu, t = %zu: dotMask equals the host form; share, dotMask, mulFinish, recover\n", name, terms,
              N, n, t);
}

// X, Y and [R] as the sharings of share_rows and of a dealer, read party-major: one process holds every party, and which
// element is called whose does not matter to the local step
template <typename T, class F>
static void matmul(const char* name, std::size_t a, std::size_t K, std::size_t b, std::size_t N, std::size_t n) {
  const typename F::Ctx ctx{};
  std::vector<std::vector<T>> unused;
  const auto X = share_rows<T>(std::string("ip gpu X ") + name, a * K, N, n, 1, &unused), Y = share_rows<T>(std::string("ip gpu Y ") + name, K * b, N, n, 1, &unused);
  const auto R = share_rows<T>(std::string("ip gpu R ") + name, a * b, N, n, 1, &unused);
  const auto hX = download<T, F>(X), hY = download<T, F>(Y), hR = download<T, F>(R);
  for (const hip::ShareMatrix<T>* r2 : {static_cast<const hip::ShareMatrix<T>*>(nullptr), &R}) {
    const auto D = hip::matmulMask(X, Y, a, K, b, r2);
    const auto hD = download<T, F>(D);
    bool same = D.parties() == n * a * b && D.secrets() == N;
    for (std::size_t j = 0; same && j < n; ++j)
      for (std::size_t i = 0; same && i < a; ++i)
        for (std::size_t l = 0; same && l < b; ++l)
          for (std::size_t s = 0; same && s < N; ++s) {
            const std::size_t e = ((j * a + i) * b + l) * N + s;
            same = F::eq(hD[e], sclhip::ip_dot_one<F>(ctx, &hX[((j * a + i) * K) * N + s], N, &hY[(j * K * b + l) * N + s], b * N, K, r2 ? &hR[e] : nullptr));
          }
    REQUIRE(same);
  }
  const auto tile = hip::matmulTile<T>();
  REQUIRE(tile.first > 0 && tile.second > 0);
  std::printf("%s: %zu x %zu by %zu x %zu, %zu instances, %zu parties (tile %d x %d): matmulMask equals the host form\n", name, a, K, K, b, N, n,
              tile.first, tile.second);
}

static int gpu() {
  dot<F61, sclhip::M61>("Mersenne61", 3, 38, 10, 3);
  dot<F61, sclhip::M61>("Mersenne61", 65, 38, 4, 1);  // past the accumulator's 64 terms
  dot<F127, sclhip::M127>("Mersenne127", 8, 33, 7, 3);
  dot<Scalar, sclhip::Secp256k1Scalar>("secp256k1_order", 5, 9, 4, 1);
  matmul<F61, sclhip::M61>("Mersenne61", 5, 7, 3, 38, 4);
  matmul<F61, sclhip::M61>("Mersenne61", 1, 65, 1, 38, 4);  // the inner-product route
  matmul<F127, sclhip::M127>("Mersenne127", 3, 4, 5, 33, 3);
  matmul<Scalar, sclhip::Secp256k1Scalar>("secp256k1_order", 3, 3, 3, 9, 4);
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
  std::fprintf(stderr, "usage: test_ip_api --host | --gpu\n");
  return 2;
}
