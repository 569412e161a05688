// tests/cxx/test_triples_api.cc -- the triple dealer of the C++ mirror: ss::randomTripleAdditive / ss::randomTripleShamir
// (include/scl_hip/ss/triples.h) on the host and hip::dealTriplesAdditive / hip::dealTriplesShamir (include/scl_hip/hip/triples.h)
// on the GPU.
//
//   test_triples_api --host   the runs of tests/golden/golden_triples.json (the same seeds, burns and shapes) by the per-secret
//                             calls, printed in the fixture's layout -- tests/test_triples_host.py compares the two -- and the
//                             reference's "Beaver multiplication protocol" (test/scl/protocol/test_protocol.cc:36-78) restated
//                             over the mirror: xs, ys, ts as written there, both parties' arithmetic of beaver.h:40-61,
//                             z0 + z1 == x * y == 462.  Needs no GPU; also built with -fsanitize=address,undefined.
//   test_triples_api --gpu    N triples dealt on the device equal N per-secret calls on one PRG, element for element, and the
//                             PRG ends at the same counter; deal -> mask -> open -> finish -> recover multiplies.  Needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/hip/beaver.h>
#include <scl_hip/hip/triples.h>
#include <scl_hip/ss/triples.h>

#include "check.hpp"

using namespace scl;

static const char* SEED = "triples fixture";

template <typename T>
static std::vector<T> column(const std::vector<hip::Triple<T>>& tr, int which) {
  std::vector<T> v;
  for (const auto& p : tr) v.push_back(which == 0 ? p.a : which == 1 ? p.b : p.c);
  return v;
}

static bool g_first = true;
template <typename T>
static void run(const char* field, std::size_t n, long t, std::size_t burn) {
  auto prg = util::PRG::create(SEED);
  if (burn) (void)prg.next(16 * burn);
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,", g_first ? "" : ",", field, n);
  g_first = false;
  if (t >= 0) std::printf("\"t\":%ld,", t);
  std::printf("\"seed\":\"%s\",\"burn\":%zu,\"triples\":[", SEED, burn);
  for (int k = 0; k < 5; ++k) {
    const std::uint64_t before = prg.counter();
    const auto tr = t < 0 ? ss::randomTripleAdditive<T>(n, prg) : ss::randomTripleShamir<T>((std::size_t)t, n, prg);
    REQUIRE(tr.size() == n && prg.counter() - before == hip::tripleBlocks<T>(t >= 0, n, t < 0 ? 0 : (std::size_t)t));
    const auto a = column(tr, 0), b = column(tr, 1), c = column(tr, 2);
    if (t < 0) REQUIRE(math::Vector<T>(a).sum() * math::Vector<T>(b).sum() == math::Vector<T>(c).sum());
    else REQUIRE(ss::shamirRecoverP(math::Vector<T>(a)) * ss::shamirRecoverP(math::Vector<T>(b)) == ss::shamirRecoverP(math::Vector<T>(c)));
    std::printf("%s{", k ? "," : "");
    elems("a", a, ",");
    elems("b", b, ",");
    elems("c", c, "}");
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

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;
using Field = math::FF<math::ff::Secp256k1Field>;

static int host() {
  std::printf("{");
  {  // "Beaver multiplication protocol": test_protocol.cc:36-41, then BeaverMul::run for both parties (beaver.h:40-61)
    auto prg = util::PRG::create();
    const auto x = F61(42), y = F61(11);
    const auto xs = ss::additiveShare(x, 2, prg), ys = ss::additiveShare(y, 2, prg);
    const auto ts = ss::randomTripleAdditive<F61>(2, prg);
    std::vector<F61> e, d, z;
    for (int i = 0; i < 2; ++i) {
      e.push_back(xs[i] - ts[i].a);  // [e] = [x] - [a]
      d.push_back(ys[i] - ts[i].b);  // [d] = [y] - [b]
    }
    e.push_back(e[0] + e[1]);
    d.push_back(d[0] + d[1]);
    for (int i = 0; i < 2; ++i) {
      auto zi = e[2] * ts[i].b + d[2] * ts[i].a + ts[i].c;
      if (i == 0) zi += e[2] * d[2];  // only party 0 adds constants
      z.push_back(zi);
    }
    z.push_back(z[0] + z[1]);
    REQUIRE(z[2] == x * y);
    REQUIRE(z[2] == F61(462));
    std::printf("\"protocol\":{\"x\":\"%s\",\"y\":\"%s\",", image(x).c_str(), image(y).c_str());
    elems("xs", std::vector<F61>{xs[0], xs[1]}, ",");
    elems("ys", std::vector<F61>{ys[0], ys[1]}, ",");
    elems("a", column(ts, 0), ",");
    elems("b", column(ts, 1), ",");
    elems("c", column(ts, 2), ",");
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
  return summary(stderr);
}

// ---- on the device -----------------------------------------------------------------------------------------------------------
template <typename T>
static bool same_as_host(const hip::Triple<hip::ShareMatrix<T>>& dev, std::size_t N, std::size_t n, long t, util::PRG& prg) {
  bool same = dev.a.parties() == n && dev.a.secrets() == N;
  for (std::size_t s = 0; same && s < N; ++s) {
    const auto tr = t < 0 ? ss::randomTripleAdditive<T>(n, prg) : ss::randomTripleShamir<T>((std::size_t)t, n, prg);
    same = dev.a.sharesOf(s) == column(tr, 0) && dev.b.sharesOf(s) == column(tr, 1) && dev.c.sharesOf(s) == column(tr, 2);
  }
  return same;
}

template <typename T>
static void device_equals_host(const char* name, std::size_t N, std::size_t n, long t) {
  auto dprg = util::PRG::create(std::string("triples gpu ") + name), hprg = util::PRG::create(std::string("triples gpu ") + name);
  (void)dprg.next(32);  // both start two blocks in
  (void)hprg.next(32);
  const auto dev = t < 0 ? hip::dealTriplesAdditive<T>(N, n, dprg) : hip::dealTriplesShamir<T>(N, (std::size_t)t, n, dprg);
  REQUIRE(same_as_host(dev, N, n, t, hprg));
  REQUIRE(dprg.counter() == hprg.counter());
  std::printf("%s: %zu %s triples, n = %zu%s%s, equal the per-secret calls\n", name, N, t < 0 ? "additive" : "Shamir", n, t < 0 ? "" : ", t = ",
              t < 0 ? "" : std::to_string(t).c_str());
}

template <typename T>
static void multiply(const char* name, std::size_t N, std::size_t n, long t) {
  auto sprg = util::PRG::create(std::string("triples secrets ") + name), prg = util::PRG::create(std::string("triples shares ") + name);
  std::vector<T> x, y, want;
  for (std::size_t s = 0; s < N; ++s) {
    x.push_back(T::random(sprg));
    y.push_back(T::random(sprg));
    want.push_back(x[s] * y[s]);
  }
  auto share = [&](const std::vector<T>& v) {
    return t < 0 ? ss::additiveShare(hip::DeviceVector<T>(v), n, prg) : ss::shamirSecretShare(hip::DeviceVector<T>(v), (std::size_t)t, n, prg);
  };
  const hip::ShareMatrix<T> xs = share(x), ys = share(y);
  const auto triple = t < 0 ? hip::dealTriplesAdditive<T>(N, n, prg) : hip::dealTriplesShamir<T>(N, (std::size_t)t, n, prg);
  const auto masked = hip::beaverMask(xs, ys, triple);
  const auto opened = t < 0 ? hip::beaverOpenAdditive(masked) : hip::beaverOpenShamir(masked);
  const hip::ShareMatrix<T> z = hip::beaverFinish(opened, triple, t < 0 ? 1 : n);
  const auto got = (t < 0 ? ss::additiveRecover(z) : ss::shamirRecoverP(z)).toHost();
  bool same = got.size() == N;
  for (std::size_t s = 0; same && s < N; ++s) same = got[s] == want[s];
  REQUIRE(same);
  std::printf("%s: deal, mask, open, finish, recover multiplies %zu secrets (%s, n = %zu)\n", name, N, t < 0 ? "additive" : "Shamir", n);
}

static int gpu() {
  device_equals_host<F61>("Mersenne61", 67, 3, -1);
  device_equals_host<Scalar>("secp256k1_order", 33, 2, -1);
  device_equals_host<F61>("Mersenne61", 67, 10, 3);
  device_equals_host<F127>("Mersenne127", 33, 16, 7);
  device_equals_host<Scalar>("secp256k1_order", 33, 4, 1);  // two-pass: the scratch is the call's own
  device_equals_host<F61>("Mersenne61", 33, 20, 9);          // two-pass
  multiply<F61>("Mersenne61", 257, 2, -1);
  multiply<F61>("Mersenne61", 257, 10, 3);
  multiply<Scalar>("secp256k1_order", 65, 5, 2);
  return summary();
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--host")) return host();
  if (argc == 2 && !std::strcmp(argv[1], "--gpu")) return gpu();
  std::fprintf(stderr, "usage: test_triples_api --host | --gpu\n");
  return 2;
}
