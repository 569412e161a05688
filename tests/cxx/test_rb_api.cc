// tests/cxx/test_rb_api.cc -- random shared bits in the C++ mirror: math::sqrt and ss::randomBitFinish
// (include/scl_hip/ss/random_bit.h) on the host, hip::sqrt and hip::bitsFinish (include/scl_hip/hip/rb.h) on the GPU.
//
//   test_rb_api --host   math::sqrt over the five prime fields: root^2 == a, the root's FF::write image is even (its low byte:
//                        the image is big-endian for the Montgomery fields, little-endian for the Mersenne ones), the odd root
//                        is its negative, 0 has the root 0, a non-residue throws std::logic_error; ss::randomBitFinish of the
//                        even root of u is a share of 1, of the odd root a share of 0, and reports a zero or a non-square u.
//                        Needs no GPU.
//   test_rb_api --gpu    hip::sqrt under the four flag combinations and hip::bitsFinish equal the host forms word for word, status
//                        bytes included, with zeros and non-residues among the inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/hip/rb.h>
#include <scl_hip/ss/random_bit.h>

#include "check.hpp"

using namespace scl;

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using M128 = math::FF<math::ff::Mont128>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;
using Field = math::FF<math::ff::Secp256k1Field>;

// the host form with the device's conventions: (value written, status)
template <typename T>
static T root_or_status(const T& a, unsigned flags, int* status) {
  *status = a == T{} ? 1 : 0;
  try {
    const T r = math::sqrt(a, (flags & SCL_RB_ODD_ROOT) != 0);
    return (flags & SCL_RB_INVERSE) && !(a == T{}) ? r.inverse() : r;
  } catch (const std::logic_error&) {
    *status = 2;
    return T{};
  }
}

template <typename T>
static bool is_odd(const T& v) {  // of the integer FF::write serialises
  unsigned char buf[64];
  v.write(buf);
  constexpr bool big_endian = T::byteSize() == 32 || T::Field::TAG == SCL_MONT128;
  return (buf[big_endian ? T::byteSize() - 1 : 0] & 1) != 0;
}

template <typename T>
static std::vector<T> inputs(const std::string& seed, std::size_t N) {
  auto prg = util::PRG::create(seed);
  const auto v = math::Vector<T>::random(N, prg);
  std::vector<T> out;
  for (std::size_t i = 0; i < N; ++i) out.push_back(v[i]);
  return out;
}

template <typename T>
static void host_field(const char* name) {
  std::size_t residues = 0, others = 0;
  auto values = inputs<T>(std::string("rb host ") + name, 64);
  values.push_back(T(1));
  values.push_back(T(4));
  for (const T& a : values) {
    int st = -1;
    const T even = root_or_status(a, 0, &st);
    if (st == 2) {
      ++others;
      int bst = 0;
      REQUIRE(ss::randomBitFinish(a, a, &bst) == T{} && bst == 2);
      continue;
    }
    ++residues;
    const T odd = math::sqrt(a, true);
    REQUIRE(even * even == a && odd * odd == a && !is_odd(even) && is_odd(odd) && even + odd == T{});
    int bst = -1;
    REQUIRE(ss::randomBitFinish(a, even, &bst) == T::one() && bst == 0);
    REQUIRE(ss::randomBitFinish(a, odd) == T{});
  }
  REQUIRE(residues > 16 && others > 16);
  int st = -1;
  REQUIRE(math::sqrt(T{}) == T{} && ss::randomBitFinish(T{}, T(5), &st) == T{} && st == 1);
  REQUIRE(math::sqrt(T(4)) == T(2) && math::sqrt(T(4), true) == T{} - T(2));
  std::printf("%s: %zu residues, %zu non-residues\n", name, residues, others);
}

static int host() {
  host_field<F61>("Mersenne61");
  host_field<F127>("Mersenne127");
  host_field<M128>("Mont128");
  host_field<Scalar>("secp256k1_order");
  host_field<Field>("secp256k1_field");
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
static void gpu_field(const char* name, std::size_t N, std::size_t rows) {
  auto a = inputs<T>(std::string("rb gpu a ") + name, N);
  a[0] = a[N / 2] = a[N - 1] = T{};
  const hip::DeviceVector<T> ad(a);
  for (unsigned flags = 0; flags < 4; ++flags) {
    const auto got = hip::sqrt(ad, flags);
    const auto values = got.values.toHost();
    bool ok = values.size() == N && got.status.size() == N;
    for (std::size_t i = 0; ok && i < N; ++i) {
      int st = -1;
      const T want = root_or_status(a[i], flags, &st);
      ok = same_words(values[i], want) && got.status[i] == st;
    }
    REQUIRE(ok);
  }
  // u: squares, a zero and a non-residue among them; r: rows of uniform shares, the first two ARE the two roots in column 1
  auto u = inputs<T>(std::string("rb gpu u ") + name, N);
  T nonresidue{};
  for (const T& v : a) {
    int st = -1;
    (void)root_or_status(v, 0, &st);
    if (st == 2) nonresidue = v;
  }
  REQUIRE(!(nonresidue == T{}));
  for (T& v : u) v = v * v;
  u[0] = T{};
  u[N - 1] = nonresidue;
  std::vector<std::vector<T>> r;
  for (std::size_t i = 0; i < rows; ++i) r.push_back(inputs<T>(std::string("rb gpu r ") + name + std::to_string(i), N));
  r[0][1] = math::sqrt(u[1]);
  r[1][1] = math::sqrt(u[1], true);
  hip::ShareMatrix<T> rd(rows, N);
  for (std::size_t i = 0; i < rows; ++i) {
    std::vector<std::uint64_t> limbs(N * hip::ShareMatrix<T>::LIMBS);
    for (std::size_t s = 0; s < N; ++s) r[i][s].toLimbs(limbs.data() + s * hip::ShareMatrix<T>::LIMBS);
    hip::check(scl_hip_memcpy_h2d(rd.data() + i * rd.stride() * hip::ShareMatrix<T>::LIMBS, limbs.data(), limbs.size() * 8, nullptr));
  }
  hip::check(scl_hip_stream_sync(nullptr));
  const auto bits = hip::bitsFinish(hip::DeviceVector<T>(u), rd);
  bool ok = bits.status.size() == N && bits.status[0] == 1 && bits.status[N - 1] == 2;
  for (std::size_t s = 0; ok && s < N; ++s) {
    const auto column = bits.shares.sharesOf(s);
    for (std::size_t i = 0; ok && i < rows; ++i) {
      int st = -1;
      ok = same_words(column[i], ss::randomBitFinish(u[s], r[i][s], &st)) && bits.status[s] == st;
    }
    if (s == 1) ok = ok && column[0] == T::one() && column[1] == T{};
  }
  REQUIRE(ok);
  std::printf("%s: N = %zu, %zu rows: hip::sqrt (four flag combinations) and hip::bitsFinish equal the host forms\n", name, N, rows);
}

static int gpu() {
  gpu_field<F61>("Mersenne61", 257, 3);
  gpu_field<F61>("Mersenne61", 66, 17);
  gpu_field<F127>("Mersenne127", 65, 3);
  gpu_field<M128>("Mont128", 65, 3);
  gpu_field<Scalar>("secp256k1_order", 65, 2);
  gpu_field<Field>("secp256k1_field", 65, 2);
  bool refused = false;
  try {
    (void)hip::sqrt(hip::DeviceVector<F61>(std::vector<F61>(4, F61(9))), 4u);
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
  std::fprintf(stderr, "usage: test_rb_api --host | --gpu\n");
  return 2;
}
