// tests/cxx/check.hpp -- what the stand-alone test programs of this directory share.  One of two halves, chosen by the including
// file:
//
//   * the test_X_api.cc programs (the default): REQUIRE with its counters and the closing summary; the FF::write image of an
//     element in hex, a JSON array of such images, hex -> bytes, a line's fields, and the way between an element of the mirror and
//     the limbs the per-element forms of include/scl_hip/detail/ work on.
//   * the X_host_check.cc programs, which #define CHECK_SEED to the constant their splitmix64 generator starts from (each keeps its
//     own, so each keeps its own operands) after including their detail/ header: check() with its counters and the closing
//     summary, the generator, and Gen<F> -- a uniform canonical element, the extreme ones and the largest one of every field struct
//     of detail/field.hpp.
#ifndef SCL_TESTS_CXX_CHECK_HPP
#define SCL_TESTS_CXX_CHECK_HPP

#include <cstdint>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#ifndef CHECK_SEED
// ---------------------------------------------------------------------------------------------------- the API test programs
static int g_fail = 0, g_checks = 0;
#define REQUIRE(...)                                                              \
  do {                                                                            \
    ++g_checks;                                                                   \
    if (!(__VA_ARGS__)) {                                                         \
      ++g_fail;                                                                   \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
    }                                                                             \
  } while (0)

/// "<checks> checks, <failures> failures" on `to`; -> the program's exit status
inline int summary(std::FILE* to = stdout) {
  std::fprintf(to, "%d checks, %d failures\n", g_checks, g_fail);
  return g_fail != 0;
}

template <typename T>
std::string image(const T& v) {  // the FF::write image, in hex
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
template <class V>  // std::vector<T> or math::Vector<T>
void elems(const char* key, const V& v, const char* tail) {
  std::printf("\"%s\":[", key);
  for (std::size_t i = 0; i < v.size(); ++i) std::printf("%s\"%s\"", i ? "," : "", image(v[i]).c_str());
  std::printf("]%s", tail);
}

inline std::vector<unsigned char> unhex(const std::string& s) {  // "-" is the empty string
  std::vector<unsigned char> out;
  if (s == "-") return out;
  for (std::size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((unsigned char)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}
inline std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::stringstream ss(s);
  for (std::string item; std::getline(ss, item, sep);) out.push_back(item);
  return out;
}

// the elements' limbs, for the per-element forms of include/scl_hip/detail/
template <typename T, class F>
typename F::E limbs(const T& v) {
  std::uint64_t w[4] = {0, 0, 0, 0};
  v.toLimbs(w);
  return F::ld(w);
}
template <typename T, class F>
T element(const typename F::E& e) {
  std::uint64_t w[4] = {0, 0, 0, 0};
  F::st(w, e);
  return T::fromLimbs(w);
}

#else
// ---------------------------------------------------------------------------------------------------- the host checks
using namespace sclhip;

static long g_bad = 0, g_checks = 0;
inline void check(bool ok, const char* what, const char* op, long at) {
  ++g_checks;
  if (!ok) {
    if (g_bad < 20) std::printf("MISMATCH %s %s case %ld\n", what, op, at);
    ++g_bad;
  }
}
/// "<checks> checks, <mismatches> mismatches" -> the program's exit status
inline int summary() {
  std::printf("%ld checks, %ld mismatches\n", g_checks, g_bad);
  return g_bad != 0;
}

static u64 g_state = CHECK_SEED;
inline u64 next64() {  // splitmix64
  u64 z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline u128 next128() {
  const u64 lo = next64();
  return ((u128)next64() << 64) | lo;
}

// per field: rnd -- a uniform canonical element; pool -- the extreme ones; top -- the largest one, pool[2]
template <class F>
struct Gen;
template <>
struct Gen<M61> {
  static u64 rnd(const M61::Ctx&) { return next64() % M61::P; }
  static std::vector<u64> pool(const M61::Ctx&) {
    const u64 p = M61::P;
    return {0, 1, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2};
  }
  static u64 top(const M61::Ctx&) { return M61::P - 1; }
};
template <>
struct Gen<M127> {
  static u128 rnd(const M127::Ctx&) { return next128() % M127::P(); }
  static std::vector<u128> pool(const M127::Ctx&) {
    const u128 p = M127::P();
    return {0, 1, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2};
  }
  static u128 top(const M127::Ctx&) { return M127::P() - 1; }
};
template <>
struct Gen<Mont128> {
  static u128 rnd(const Mont128::Ctx& c) { return next128() % c.p; }
  static std::vector<u128> pool(const Mont128::Ctx& c) {
    const u128 p = c.p;
    return {0, 1, p - 1, p - 2, (p - 1) / 2, (p - 1) / 2 + 1, c.one};
  }
  static u128 top(const Mont128::Ctx& c) { return c.p - 1; }
};
template <>
struct Gen<Gf128> {
  static u128 rnd(const Gf128::Ctx&) { return next128(); }
  static std::vector<u128> pool(const Gf128::Ctx&) {
    const u128 ones = ~(u128)0;
    return {0, 1, ones, ones - 1, ones >> 1, (u128)1 << 127};
  }
  static u128 top(const Gf128::Ctx&) { return ~(u128)0; }
};
template <class PRM>
struct Gen<Mont256<PRM>> {
  typedef Mont256<PRM> F;
  static typename F::E rnd(const typename F::Ctx&) {
    typename F::E r = F::make(next64(), next64(), next64(), next64());
    if (F::geq_p(r)) F::sub_n(r, r, F::prime());  // both primes exceed 2^255: one subtraction lands below p
    return r;
  }
  static std::vector<typename F::E> pool(const typename F::Ctx& c) {
    const typename F::E p = F::prime(), one = F::make(1, 0, 0, 0), two = F::make(2, 0, 0, 0);
    typename F::E pm1, pm2, half, half1;
    F::sub_n(pm1, p, one);
    F::sub_n(pm2, p, two);
    half = F::make((pm1.w[0] >> 1) | (pm1.w[1] << 63), (pm1.w[1] >> 1) | (pm1.w[2] << 63), (pm1.w[2] >> 1) | (pm1.w[3] << 63),
                   pm1.w[3] >> 1);
    F::add_n(half1, half, one);
    return {F::zero(), one, pm1, pm2, half, half1, F::one(c)};
  }
  static typename F::E top(const typename F::Ctx&) {
    typename F::E r;
    F::sub_n(r, F::prime(), F::make(1, 0, 0, 0));
    return r;
  }
};
template <typename W, int L, int T>
struct Gen<Z2kRing<W, L, T>> {
  typedef Z2kRing<W, L, T> F;
  static W rnd(const typename F::Ctx& c) { return (W)next128() & c.mask; }
  static std::vector<W> pool(const typename F::Ctx& c) {
    const W top = (W)1 << (c.K - 1);
    return {0, (W)1 & c.mask, c.mask, (W)(c.mask - 1) & c.mask, top, (W)(top - 1)};
  }
};
#endif

#endif
