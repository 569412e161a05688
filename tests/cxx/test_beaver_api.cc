// tests/cxx/test_beaver_api.cc -- hip::beaverMask / hip::beaverFinish (include/scl_hip/hip/beaver.h) end to end on the GPU.
//
//   test_beaver_api
//
// Shamir (n, t) = (5, 2) over FF<Secp256k1Scalar> and over Fp<61>: N secrets x, y and a triple (a, b, c = a b) shared with
// ss::shamirSecretShare, every party masked in one launch, e and d opened, every party finished in one launch (a constant is
// its own Shamir sharing: all parties add e d), ss::shamirRecoverP(z) == x y element by element.  Then the shape of the
// reference's own test (two parties, additive shares, party 0 adds e d): each party masks its own shares into a packet (e then
// d), the packets are summed, each party finishes alone, the sum of the two results is x y.  Needs a GPU.
#include <cstdio>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/hip/beaver.h>

#include "check.hpp"

using namespace scl;

template <typename T>
static std::vector<T> randoms(std::size_t N, util::PRG& prg) {
  std::vector<T> v;
  for (std::size_t s = 0; s < N; ++s) v.push_back(T::random(prg));
  return v;
}

template <typename T>
static std::vector<T> products(const std::vector<T>& x, const std::vector<T>& y) {
  std::vector<T> v;
  for (std::size_t s = 0; s < x.size(); ++s) v.push_back(x[s] * y[s]);
  return v;
}

template <typename T>
static void shamir_round_trip(const char* name, std::size_t N) {
  const std::size_t n = 5, t = 2;
  auto sprg = util::PRG::create(std::string("beaver secrets ") + name), prg = util::PRG::create(std::string("beaver shares ") + name);
  const auto x = randoms<T>(N, sprg), y = randoms<T>(N, sprg), a = randoms<T>(N, sprg), b = randoms<T>(N, sprg);
  const auto c = products(a, b), want = products(x, y);
  auto share = [&](const std::vector<T>& v) { return ss::shamirSecretShare(hip::DeviceVector<T>(v), t, n, prg); };
  const hip::ShareMatrix<T> xs = share(x), ys = share(y);
  const hip::Triple<hip::ShareMatrix<T>> triple{share(a), share(b), share(c)};
  const auto masked = hip::beaverMask(xs, ys, triple);
  REQUIRE(masked.parties() == n && masked.secrets() == N);
  const auto opened = hip::beaverOpenShamir(masked);
  const auto ed = opened.ed.toHost();
  bool same = ed.size() == 2 * N;
  for (std::size_t s = 0; same && s < N; ++s) same = ed[s] == x[s] - a[s] && ed[N + s] == y[s] - b[s];
  REQUIRE(same);
  const hip::ShareMatrix<T> z = hip::beaverFinish(opened, triple, n);
  const auto got = ss::shamirRecoverP(z).toHost();
  REQUIRE(got.size() == N);
  same = got.size() == N;
  for (std::size_t s = 0; same && s < N; ++s) same = got[s] == want[s];
  REQUIRE(same);
  // t + 1 = 3 parties' rows of z already determine the product (z has degree t)
  const auto some = z.sharesOf(N - 1);
  REQUIRE(ss::shamirRecoverP(math::Vector<T>(std::vector<T>(some.begin(), some.begin() + 3))) == want[N - 1]);
  std::printf("%s: Shamir (%zu, %zu) multiplication of %zu secrets\n", name, n, t, N);
}

// BeaverMul::run for both parties of the reference's test, N multiplications at once
template <typename T>
static void two_party_additive(const char* name, std::size_t N) {
  auto sprg = util::PRG::create(std::string("beaver2 secrets ") + name), prg = util::PRG::create(std::string("beaver2 shares ") + name);
  const auto x = randoms<T>(N, sprg), y = randoms<T>(N, sprg), a = randoms<T>(N, sprg), b = randoms<T>(N, sprg);
  const auto c = products(a, b), want = products(x, y);
  auto share = [&](const std::vector<T>& v) { return ss::additiveShare(hip::DeviceVector<T>(v), 2, prg); };
  const hip::ShareMatrix<T> xs = share(x), ys = share(y), as = share(a), bs = share(b), cs = share(c);
  auto row = [&](const hip::ShareMatrix<T>& m, std::size_t i) {  // party i's shares as a vector of its own
    std::vector<T> v;
    for (std::size_t s = 0; s < N; ++s) v.push_back(m.sharesOf(s)[i]);
    return hip::DeviceVector<T>(v);
  };
  std::vector<hip::Triple<hip::DeviceVector<T>>> triples;
  std::vector<hip::OpenedMask<T>> packets;
  for (std::size_t i = 0; i < 2; ++i) {
    triples.push_back(hip::Triple<hip::DeviceVector<T>>{row(as, i), row(bs, i), row(cs, i)});
    packets.push_back(hip::beaverMask(row(xs, i), row(ys, i), triples[i]));
  }
  hip::OpenedMask<T> opened{hip::DeviceVector<T>(2 * N)};
  hip::add(opened.ed, packets[0].ed, packets[1].ed);    // e = e0 + e1, d = d0 + d1
  const auto z0 = hip::beaverFinish(opened, triples[0], true).toHost();   // only party 0 adds constants
  const auto z1 = hip::beaverFinish(opened, triples[1], false).toHost();
  bool same = z0.size() == N && z1.size() == N;
  for (std::size_t s = 0; same && s < N; ++s) same = z0[s] + z1[s] == want[s];
  REQUIRE(same);
  // the same two rows from the all-parties call with ed_parties = 1
  const hip::Triple<hip::ShareMatrix<T>> all{share(a), share(b), share(c)};
  const auto zs = ss::additiveRecover(hip::beaverFinish(hip::beaverOpenAdditive(hip::beaverMask(xs, ys, all)), all, 1)).toHost();
  same = zs.size() == N;
  for (std::size_t s = 0; same && s < N; ++s) same = zs[s] == want[s];
  REQUIRE(same);
  std::printf("%s: two-party additive multiplication of %zu secrets\n", name, N);
}

int main() {
  using Scalar = math::FF<math::ff::Secp256k1Scalar>;
  using F61 = math::Fp<61>;
  shamir_round_trip<Scalar>("secp256k1_order", 257);
  shamir_round_trip<F61>("Mersenne61", 4099);
  two_party_additive<F61>("Mersenne61", 257);
  two_party_additive<Scalar>("secp256k1_order", 65);
  return summary();
}
