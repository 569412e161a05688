// tests/cxx/test_fx_api.cc -- probabilistic truncation in the C++ mirror: ss::composeBits, ss::truncMask and ss::truncFinish
// (include/scl_hip/ss/trunc.h) on the host, hip::composeBits, hip::truncMask and hip::truncFinish (include/scl_hip/hip/fx.h) on
// the GPU.
//
//   test_fx_api --host   over the five prime fields, n = 4 parties and degree-1 sharings: shares of x and of true random bits are
//                        masked party by party, c is opened from two shares, every party finishes, and the shares reconstruct
//                        floor((x + 2^(k-1)) / 2^shift) + carry - 2^(k-1-shift) exactly (k = 24, shift = 9, B = 32, both signs of
//                        x) and floor(x / 2^65) or that plus one at B = k = |p| - 2 (the shift past a limb); composeBits of bits
//                        is the integer they spell; a c beyond 2^(B+1) is reported.  Needs no GPU.
//   test_fx_api --gpu    the three device calls equal the host forms word for word, status bytes included, with a column whose x is
//                        out of range among the inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/hip/fx.h>
#include <scl_hip/ss/trunc.h>

#include "check.hpp"

using namespace scl;

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using M128 = math::FF<math::ff::Mont128>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;
using Field = math::FF<math::ff::Secp256k1Field>;

constexpr std::size_t PARTIES = 4;

static std::uint64_t g_state = 0x452821E638D01377ull;
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

// the degree-1 sharing secret + a i at the nodes 1..PARTIES
template <typename T>
static std::vector<T> share(const T& secret, const T& a) {
  std::vector<T> out;
  for (std::size_t i = 1; i <= PARTIES; ++i) out.push_back(secret + a * T((int)i));
  return out;
}

// the basis of the nodes 1, 2 at 0: 2, -1
template <typename T>
static std::vector<T> lambda2() {
  return {T(2), T{} - T(1)};
}

template <typename T>
static T open2(const std::vector<T>& shares) {
  const auto lam = lambda2<T>();
  return lam[0] * shares[0] + lam[1] * shares[1];
}

// x truncated by the whole protocol on the host -> the reconstructed y
template <typename T>
static T truncate(const std::string& seed, const T& x, const std::vector<int>& bits, std::size_t k, std::size_t shift, int* status) {
  const std::size_t B = bits.size();
  const auto coef = randoms<T>(seed, B + 1);
  const auto xs = share(x, coef[B]);
  std::vector<std::vector<T>> bs(PARTIES);  // [party][bit]
  for (std::size_t i = 0; i < B; ++i) {
    const auto s = share(T(bits[i]), coef[i]);
    for (std::size_t p = 0; p < PARTIES; ++p) bs[p].push_back(s[p]);
  }
  std::vector<T> c, rlow;
  for (std::size_t p = 0; p < PARTIES; ++p) {
    const auto m = ss::truncMask(xs[p], bs[p], k, shift);
    c.push_back(m.c);
    rlow.push_back(m.rlow);
  }
  const T opened = open2(c);
  std::vector<T> y;
  for (std::size_t p = 0; p < PARTIES; ++p) y.push_back(ss::truncFinish(opened, xs[p], rlow[p], shift, B, status));
  const T first = open2(y);
  REQUIRE(y[2] - y[1] == y[1] - y[0] && y[3] - y[2] == y[1] - y[0]);  // the finished shares lie on one line
  return first;
}

template <typename T>
static void host_field(const char* name, std::size_t top) {
  const std::size_t k = 24, shift = 9, B = 32;
  long carries = 0;
  for (int rep = 0; rep < 24; ++rep) {
    std::vector<int> bits;
    for (std::size_t i = 0; i < B; ++i) bits.push_back((int)(next() >> 63));
    long xs = (long)(next() >> 41) - (1l << 22);  // in [-2^22, 2^22), within [-2^23, 2^23)
    if (rep == 0) xs = -(1l << 23);
    if (rep == 1) xs = (1l << 23) - 1;
    if (rep == 2) xs = -1;
    long rlow = 0;
    for (std::size_t i = 0; i < shift; ++i) rlow |= (long)bits[i] << i;
    const long u = xs + (1l << (k - 1));
    const long carry = ((u & ((1l << shift) - 1)) + rlow) >> shift;
    carries += carry;
    int st = -1;
    const T y = truncate<T>(std::string("fx host ") + name + std::to_string(rep), signedInt<T>(xs), bits, k, shift, &st);
    REQUIRE(st == 0 && y == signedInt<T>((u >> shift) + carry - (1l << (k - 1 - shift))));
    // composeBits spells the integer (here its low 24 bits, so that it fits an int)
    std::vector<T> plain;
    long spelled = 0;
    for (std::size_t i = 0; i < 24; ++i) {
      plain.push_back(T(bits[i]));
      spelled |= (long)bits[i] << i;
    }
    REQUIRE(ss::composeBits(plain) == T((int)spelled));
  }
  REQUIRE(carries > 2 && carries < 22);
  // B = k = |p| - 2, the shift past the first limb: a small x truncates to 0 or 1, a small negative one to -1 or 0
  for (int sign = 0; sign < 2; ++sign) {
    std::vector<int> bits;
    for (std::size_t i = 0; i < top; ++i) bits.push_back((int)((i * 7 + sign) % 3 == 0));
    int st = -1;
    const std::size_t sh = top > 70 ? 65 : 33;
    const T y = truncate<T>(std::string("fx host top ") + name, signedInt<T>(sign ? -12345 : 12345), bits, top, sh, &st);
    const T floor = sign ? T{} - T(1) : T{};
    REQUIRE(st == 0 && (y == floor || y == floor + T(1)));
  }
  // a c at 2^(B+1) is out of range: status 1 and a zero share; 2^(B+1) - 1 is not
  T edge = T(1);
  for (std::size_t i = 0; i < B + 1; ++i) edge = edge + edge;
  int st = -1;
  REQUIRE(ss::truncFinish(edge, T(5), T(7), shift, B, &st) == T{} && st == 1);
  (void)ss::truncFinish(edge - T(1), T(5), T(7), shift, B, &st);
  REQUIRE(st == 0);
  bool refused = false;
  try {
    (void)ss::truncMask(T(1), std::vector<T>(top + 1, T(1)), 4, 2);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  REQUIRE(refused);
  std::printf("%s: 24 truncations at (B, k, shift) = (32, 24, 9), %ld carries; two at B = k = %zu\n", name, carries, top);
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
static void gpu_field(const char* name, std::size_t N, std::size_t B, std::size_t k, std::size_t shift) {
  // x: shares of small signed values, column 1 out of range (a uniform element); bits: shares of bits, plane i at columns [i N, ..)
  const auto coef = randoms<T>(std::string("fx gpu coef ") + name, (B + 1) * N);
  const auto wild = randoms<T>(std::string("fx gpu wild ") + name, 1);
  std::vector<std::vector<T>> x(PARTIES, std::vector<T>(N)), bits(PARTIES, std::vector<T>(B * N));
  for (std::size_t s = 0; s < N; ++s) {
    const auto xs = share(s == 1 ? wild[0] : signedInt<T>((long)(s * 2654435761u % 2001) - 1000), coef[B * N + s]);
    for (std::size_t p = 0; p < PARTIES; ++p) x[p][s] = xs[p];
    for (std::size_t i = 0; i < B; ++i) {
      const auto b = share(T((int)((s * 31 + i * 17 + (s ^ i)) % 2)), coef[i * N + s]);
      for (std::size_t p = 0; p < PARTIES; ++p) bits[p][i * N + s] = b[p];
    }
  }
  const auto xd = upload(x), bd = upload(bits);
  const auto composed = hip::composeBits(bd, B);
  const auto masked = hip::truncMask(xd, bd, k, shift);
  const auto done = hip::truncFinish(masked.c, lambda2<T>(), xd, masked.rlow, shift, B);
  bool ok = done.status.size() == N, flagged = false;
  for (std::size_t s = 0; ok && s < N; ++s) {
    const auto r = composed.sharesOf(s), c = masked.c.sharesOf(s), lo = masked.rlow.sharesOf(s), y = done.shares.sharesOf(s);
    std::vector<T> hc;
    for (std::size_t p = 0; ok && p < PARTIES; ++p) {
      std::vector<T> mine;
      for (std::size_t i = 0; i < B; ++i) mine.push_back(bits[p][i * N + s]);
      const auto m = ss::truncMask(x[p][s], mine, k, shift);
      ok = same_words(r[p], ss::composeBits(mine)) && same_words(c[p], m.c) && same_words(lo[p], m.rlow);
      hc.push_back(m.c);
    }
    const T opened = open2(hc);
    for (std::size_t p = 0; ok && p < PARTIES; ++p) {
      int st = -1;
      ok = same_words(y[p], ss::truncFinish(opened, x[p][s], lo[p], shift, B, &st)) && done.status[s] == st;
      flagged = flagged || st == 1;
    }
  }
  REQUIRE(ok);
  if (B + 24 < 8 * T::byteSize()) REQUIRE(flagged);  // a uniform x lands beyond 2^(B+1) unless B is near the top
  std::printf("%s: N = %zu, (B, k, shift) = (%zu, %zu, %zu): hip::composeBits, hip::truncMask and hip::truncFinish equal the host forms\n", name, N, B, k,
              shift);
}

static int gpu() {
  gpu_field<F61>("Mersenne61", 257, 32, 24, 9);
  gpu_field<F61>("Mersenne61", 66, 59, 59, 58);
  gpu_field<F127>("Mersenne127", 65, 125, 80, 65);
  gpu_field<M128>("Mont128", 65, 100, 80, 64);
  gpu_field<Scalar>("secp256k1_order", 33, 254, 200, 129);
  gpu_field<Field>("secp256k1_field", 33, 40, 24, 9);
  bool refused = false;
  try {
    const hip::ShareMatrix<F61> x(PARTIES, 4), bits(PARTIES, 8);
    (void)hip::truncMask(x, bits, 2, 2);
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
  std::fprintf(stderr, "usage: test_fx_api --host | --gpu\n");
  return 2;
}
