// tests/cxx/test_cmp_api.cc -- exact comparison in the C++ mirror: ss::cmpOpen, ss::bitLtLeaves, ss::combine, ss::mod2m,
// ss::truncExact and ss::ltz (include/scl_hip/ss/compare.h) on the host, hip::cmpFirstMask, hip::cmpLevelMask and hip::cmpFinish
// (include/scl_hip/hip/cmp.h) on the GPU.
//
//   test_cmp_api --host   over the five prime fields, n = 4 parties, t = 1: shares of x and of true random bits are masked party by
//                         party (ss::truncMask), c is opened from two shares, every party makes its leaves, each level's products
//                         are masked with a degree-2 sharing, opened from three shares and reduced by the degree-1 sharing, and
//                         every party finishes: the shares reconstruct x mod 2^w, floor(x / 2^w) and [x < 0] exactly -- (k, w, B) =
//                         (24, 9, 32) and (24, 23, 32), both signs and the ends of x, low bits all zero and all one among the
//                         cases, and w = 65 past a limb for the wide fields; a c beyond 2^(B+1) is reported.  Needs no GPU.
//   test_cmp_api --gpu    the three device calls equal the host forms word for word, status bytes included, with a column whose c
//                         is out of range among the inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/hip/cmp.h>
#include <scl_hip/ss/compare.h>
#include <scl_hip/ss/trunc.h>

#include "check.hpp"

using namespace scl;

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using M128 = math::FF<math::ff::Mont128>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;
using Field = math::FF<math::ff::Secp256k1Field>;

constexpr std::size_t PARTIES = 4;

static std::uint64_t g_state = 0xA4093822299F31D0ull;
static std::uint64_t next() {  // splitmix64: the bits and the values of the host cases
  std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename T>
static std::vector<T> randoms(const std::string& seed, std::size_t N) {
  auto prg = util::PRG::create(seed);
  const auto v = math::Vector<T>::random(N, prg);
  std::vector<T> out;
  for (std::size_t i = 0; i < N; ++i) out.push_back(v[i]);
  return out;
}

template <typename T>
static T signedInt(long v) {  // |v| < 2^31
  return v < 0 ? T{} - T((int)-v) : T((int)v);
}

// the sharing secret + a i + b i^2 at the nodes 1..PARTIES (b = 0: degree 1)
template <typename T>
static std::vector<T> share(const T& secret, const T& a, const T& b = T{}) {
  std::vector<T> out;
  for (std::size_t i = 1; i <= PARTIES; ++i) out.push_back(secret + a * T((int)i) + b * T((int)(i * i)));
  return out;
}

// the bases at 0 of the nodes 1, 2 (degree 1) and 1, 2, 3 (degree 2)
template <typename T>
static T open2(const std::vector<T>& s) {
  return T(2) * s[0] - s[1];
}
template <typename T>
static T open3(const std::vector<T>& s) {
  return T(3) * s[0] - T(3) * s[1] + s[2];
}

// the whole protocol on the host -> the reconstructed result; what: sclhip::CMP_MOD, CMP_TRUNC or CMP_LTZ
template <typename T>
static T compare(const std::string& seed, const T& x, const std::vector<int>& bits, std::size_t k, std::size_t w, int what, int* status) {
  const std::size_t B = bits.size();
  const auto coef = randoms<T>(seed, B + 1 + 6 * sclhip::cmp_planes(w));
  std::size_t used = B + 1;
  const auto xs = share(x, coef[B]);
  std::vector<std::vector<T>> bs(PARTIES);  // [party][bit]
  for (std::size_t i = 0; i < B; ++i) {
    const auto s = share(T(bits[i]), coef[i]);
    for (std::size_t p = 0; p < PARTIES; ++p) bs[p].push_back(s[p]);
  }
  std::vector<T> c, rlow;
  for (std::size_t p = 0; p < PARTIES; ++p) {
    const auto m = ss::truncMask(xs[p], bs[p], k, w);
    c.push_back(m.c);
    rlow.push_back(m.rlow);
  }
  const auto co = ss::cmpOpen(open2(c), w, B);
  if (status) *status = co.status;
  std::vector<std::vector<ss::CmpNode<T>>> nodes(PARTIES);  // [party][node]
  for (std::size_t p = 0; p < PARTIES; ++p) nodes[p] = ss::bitLtLeaves(co, std::vector<T>(bs[p].begin(), bs[p].begin() + w));
  std::size_t levels = 0;
  do {
    const std::size_t cnt = nodes[0].size(), out = (cnt + 1) / 2;
    std::vector<std::vector<ss::CmpNode<T>>> after(PARTIES, std::vector<ss::CmpNode<T>>(out));
    for (std::size_t j = 0; j < out; ++j) {
      // one double sharing per plane: [R]_1 and [R]_2 of the same value
      const auto lo_lt = share(coef[used], coef[used + 1]), hi_lt = share(coef[used], coef[used + 2], coef[used + 3]);
      const auto lo_eq = share(coef[used + 4], coef[used + 5]), hi_eq = share(coef[used + 4], coef[used + 1], coef[used + 2]);
      used += 6;
      std::vector<T> dlt, deq;
      for (std::size_t p = 0; p < PARTIES; ++p) {
        const auto hi = 2 * j + 1 < cnt ? nodes[p][2 * j + 1] : ss::cmpIdentity<T>();
        const auto d = ss::combine(hi, nodes[p][2 * j], ss::CmpNode<T>{hi_lt[p], hi_eq[p]});
        dlt.push_back(d.lt);
        deq.push_back(d.eq);
      }
      REQUIRE(dlt[3] - T(3) * dlt[2] + T(3) * dlt[1] - dlt[0] == T{});  // four shares of a degree-2 sharing
      const T olt = open3(dlt), oeq = open3(deq);
      for (std::size_t p = 0; p < PARTIES; ++p) after[p][j] = ss::CmpNode<T>{olt - lo_lt[p], oeq - lo_eq[p]};
    }
    nodes = after;
    ++levels;
  } while (nodes[0].size() > 1);
  REQUIRE(levels == sclhip::cmp_levels(w));
  std::vector<T> y;
  for (std::size_t p = 0; p < PARTIES; ++p) {
    const T lt = nodes[p][0].lt;
    y.push_back(what == sclhip::CMP_MOD ? ss::mod2m(co, lt, rlow[p], w) : what == sclhip::CMP_TRUNC ? ss::truncExact(co, lt, rlow[p], xs[p], w)
                                                                                                    : ss::ltz(co, lt, rlow[p], xs[p], w));
  }
  REQUIRE(y[2] - y[1] == y[1] - y[0] && y[3] - y[2] == y[1] - y[0]);  // the finished shares lie on one line
  return open2(y);
}

template <typename T>
static void host_field(const char* name, std::size_t top) {
  const std::size_t k = 24, B = 32;
  long below = 0;
  for (int rep = 0; rep < 24; ++rep) {
    const std::size_t w = rep % 2 ? 23 : 9;
    std::vector<int> bits;
    for (std::size_t i = 0; i < B; ++i) bits.push_back((int)(next() >> 63));
    if (rep / 2 % 4 == 1) std::fill(bits.begin(), bits.begin() + w, 0);  // r' = 0
    if (rep / 2 % 4 == 2) std::fill(bits.begin(), bits.begin() + w, 1);  // r' = 2^w - 1
    long xs = (long)(next() >> 41) - (1l << 22);                         // in [-2^22, 2^22), within [-2^23, 2^23)
    const long corners[] = {-(1l << 23), (1l << 23) - 1, -1, 0, 1, 512};
    if (rep < 12) xs = corners[rep / 2];                                 // (0, -2^23 and 512: x mod 2^9 = 0, that is c' == r')
    const std::string seed = std::string("cmp host ") + name + std::to_string(rep);
    int st = -1;
    REQUIRE(compare<T>(seed, signedInt<T>(xs), bits, k, w, sclhip::CMP_TRUNC, &st) == signedInt<T>(xs >> w) && st == 0);
    REQUIRE(compare<T>(seed + "m", signedInt<T>(xs), bits, k, w, sclhip::CMP_MOD, &st) == signedInt<T>(xs & ((1l << w) - 1)) && st == 0);
    if (w == k - 1) REQUIRE(compare<T>(seed + "z", signedInt<T>(xs), bits, k, w, sclhip::CMP_LTZ, &st) == T(xs < 0 ? 1 : 0) && st == 0);
    below += xs < 0;
  }
  REQUIRE(below > 4 && below < 20);
  // w past the first limb (the wide fields), and the smallest shapes
  for (int sign = 0; sign < 2; ++sign) {
    if (top > 70) {
      std::vector<int> bits;
      for (std::size_t i = 0; i < top; ++i) bits.push_back((int)((i * 7 + sign) % 3 == 0));
      int st = -1;
      const T y = compare<T>(std::string("cmp host top ") + name, signedInt<T>(sign ? -12345 : 12345), bits, top, 65, sclhip::CMP_TRUNC, &st);
      REQUIRE(st == 0 && y == (sign ? T{} - T(1) : T{}));
    }
    for (std::size_t w = 1; w <= 3; ++w) {
      int st = -1;
      const long xs = sign ? -5 : 6;
      REQUIRE(compare<T>(std::string("cmp host small ") + name, signedInt<T>(xs), {1, 0, 1, 1, 0, 1}, 5, w, sclhip::CMP_TRUNC, &st) == signedInt<T>(xs >> w));
    }
  }
  // a c at 2^(B+1) is out of range: status 1, c' = 0 and a zero share; 2^(B+1) - 1 is not
  T edge = T(1);
  for (std::size_t i = 0; i < B + 1; ++i) edge = edge + edge;
  const auto bad = ss::cmpOpen(edge, 9, B), good = ss::cmpOpen(edge - T(1), 9, B);
  REQUIRE(bad.status == 1 && bad.cmod == T{} && good.status == 0 && good.cmod == T(511));
  REQUIRE(ss::truncExact(bad, T(1), T(7), T(5), 9) == T{} && ss::mod2m(good, T{}, T(11), 9) == T(500));
  bool refused = false;
  try {
    (void)ss::cmpOpen(T(1), 9, top + 1);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  REQUIRE(refused);
  std::printf("%s: 24 exact truncations and residues at (k, B) = (24, 32), w = 9 and 23, %ld negative\n", name, below);
}

static int host() {
  host_field<F61>("Mersenne61", 59);
  host_field<F127>("Mersenne127", 125);
  host_field<M128>("Mont128", 126);
  host_field<Scalar>("secp256k1_order", 254);
  host_field<Field>("secp256k1_field", 254);
  return summary();
}

template <typename T>
static bool same_words(const T& a, const T& b) {
  std::uint64_t x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
  a.toLimbs(x);
  b.toLimbs(y);
  return !std::memcmp(x, y, sizeof x);
}

template <typename T>
static hip::ShareMatrix<T> upload(const std::vector<std::vector<T>>& rows) {
  constexpr std::size_t L = hip::ShareMatrix<T>::LIMBS;
  const std::size_t N = rows[0].size();
  hip::ShareMatrix<T> out(rows.size(), N);
  for (std::size_t i = 0; i < rows.size(); ++i) {
    std::vector<std::uint64_t> limbs(N * L);
    for (std::size_t s = 0; s < N; ++s) rows[i][s].toLimbs(limbs.data() + s * L);
    hip::check(scl_hip_memcpy_h2d(out.data() + i * out.stride() * L, limbs.data(), limbs.size() * 8, nullptr));
  }
  hip::check(scl_hip_stream_sync(nullptr));
  return out;
}

template <typename T>
static std::vector<std::vector<T>> matrix(const std::string& seed, std::size_t cols) {
  const auto v = randoms<T>(seed, PARTIES * cols);
  std::vector<std::vector<T>> out(PARTIES);
  for (std::size_t p = 0; p < PARTIES; ++p) out[p].assign(v.begin() + p * cols, v.begin() + (p + 1) * cols);
  return out;
}

template <typename T>
static void gpu_field(const char* name, std::size_t N, std::size_t w, std::size_t B) {
  const std::string tag = std::string(name) + std::to_string(w);
  // c: shares of values below 2^31, column 1 out of range (a uniform element); everything else uniform elements
  const auto coef = randoms<T>("cmp gpu coef " + tag, N + 1);
  std::vector<std::vector<T>> c(PARTIES, std::vector<T>(N));
  for (std::size_t s = 0; s < N; ++s) {
    const auto cs = share(s == 1 ? coef[N] : T((int)(s * 2654435761u % 2147483647u)), coef[s]);
    for (std::size_t p = 0; p < PARTIES; ++p) c[p][s] = cs[p];
  }
  const std::size_t cnt = (w + 1) / 2, P1 = 2 * cnt, P2 = 2 * ((cnt + 1) / 2);
  const auto bits = matrix<T>("cmp gpu bits " + tag, B * N), r2a = matrix<T>("cmp gpu r2a " + tag, P1 * N), r2b = matrix<T>("cmp gpu r2b " + tag, P2 * N);
  const auto lt = matrix<T>("cmp gpu lt " + tag, N), rlow = matrix<T>("cmp gpu rlow " + tag, N), x = matrix<T>("cmp gpu x " + tag, N);
  const auto first = hip::cmpFirstMask(upload(c), std::vector<T>{T(2), T{} - T(1)}, upload(bits), upload(r2a), w, B);
  const auto second = hip::cmpLevelMask(first.d, upload(r2b), cnt);
  const auto ltd = upload(lt), rlowd = upload(rlow), xd = upload(x);
  const hip::ShareMatrix<T> done[3] = {hip::cmpFinish(ltd, first, rlowd, xd, w, SCL_CMP_MOD), hip::cmpFinish(ltd, first, rlowd, xd, w, SCL_CMP_TRUNC),
                                       hip::cmpFinish(ltd, first, rlowd, xd, w, SCL_CMP_LTZ)};
  const auto cmod = first.cmod.toHost();
  bool ok = first.flagged.size() == N, flagged = false;
  for (std::size_t s = 0; ok && s < N; ++s) {
    std::vector<T> col;
    for (std::size_t p = 0; p < PARTIES; ++p) col.push_back(c[p][s]);
    const auto co = ss::cmpOpen(open2(col), w, B);
    ok = same_words(cmod[s], co.cmod) && first.flagged[s] == co.status;
    flagged = flagged || co.status == 1;
    for (std::size_t p = 0; ok && p < PARTIES; ++p) {
      std::vector<T> mine;
      for (std::size_t i = 0; i < w; ++i) mine.push_back(bits[p][i * N + s]);
      const auto leaves = ss::bitLtLeaves(co, mine);
      std::vector<ss::CmpNode<T>> nodes;
      for (std::size_t j = 0; ok && j < cnt; ++j) {
        const auto hi = 2 * j + 1 < w ? leaves[2 * j + 1] : ss::cmpIdentity<T>();
        nodes.push_back(ss::combine(hi, leaves[2 * j], ss::CmpNode<T>{r2a[p][2 * j * N + s], r2a[p][(2 * j + 1) * N + s]}));
        ok = same_words(first.d.sharesOf(2 * j * N + s)[p], nodes[j].lt) && same_words(first.d.sharesOf((2 * j + 1) * N + s)[p], nodes[j].eq);
      }
      for (std::size_t j = 0; ok && j < (cnt + 1) / 2; ++j) {
        const auto hi = 2 * j + 1 < cnt ? nodes[2 * j + 1] : ss::cmpIdentity<T>();
        const auto d = ss::combine(hi, nodes[2 * j], ss::CmpNode<T>{r2b[p][2 * j * N + s], r2b[p][(2 * j + 1) * N + s]});
        ok = same_words(second.sharesOf(2 * j * N + s)[p], d.lt) && same_words(second.sharesOf((2 * j + 1) * N + s)[p], d.eq);
      }
      ok = ok && same_words(done[0].sharesOf(s)[p], ss::mod2m(co, lt[p][s], rlow[p][s], w)) &&
           same_words(done[1].sharesOf(s)[p], ss::truncExact(co, lt[p][s], rlow[p][s], x[p][s], w)) &&
           same_words(done[2].sharesOf(s)[p], ss::ltz(co, lt[p][s], rlow[p][s], x[p][s], w));
    }
  }
  REQUIRE(ok);
  if (B + 24 < 8 * T::byteSize()) REQUIRE(flagged);  // a uniform c lands beyond 2^(B+1) unless B is near the top
  std::printf("%s: N = %zu, (w, B) = (%zu, %zu): hip::cmpFirstMask, hip::cmpLevelMask and hip::cmpFinish equal the host forms\n", name, N, w, B);
}

static int gpu() {
  gpu_field<F61>("Mersenne61", 129, 9, 32);
  gpu_field<F61>("Mersenne61", 34, 31, 32);
  gpu_field<F127>("Mersenne127", 17, 31, 80);
  gpu_field<M128>("Mont128", 17, 31, 100);
  gpu_field<Scalar>("secp256k1_order", 9, 31, 200);
  gpu_field<Field>("secp256k1_field", 9, 7, 40);
  bool refused = false;
  try {
    const hip::ShareMatrix<F61> c(PARTIES, 4), bits(PARTIES, 8), r2(PARTIES, 8);
    (void)hip::cmpFirstMask(c, std::vector<F61>{F61(2), F61{} - F61(1)}, bits, r2, 2, 2);  // w >= B
  } catch (const std::exception&) {
    refused = true;
  }
  REQUIRE(refused);
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
  std::fprintf(stderr, "usage: test_cmp_api --host | --gpu\n");
  return 2;
}
