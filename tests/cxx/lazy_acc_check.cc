// tests/cxx/lazy_acc_check.cc -- every field's lazy accumulator (detail/field.hpp) driven with maximal raw residues for exactly
// the number of terms it claims, against the sum built by double-and-add on the field's own reduced add.  Each accumulator sums
// products (or elements) unreduced up to a bound derived by hand: F::ACC_TERMS for mac / acc_add / acc_fold, F::K_TERMS for
// kmac / kacc_fold over a prepared constant.  Uniform operands sit a factor of about four below those bounds; p - 1, all-ones
// limbs and the largest any-word inputs of kmac reach them.  Where ACC_TERMS is 2^30 (Mersenne127, GF(2^128), Z2k) the run stops
// at 2^24 terms: the accumulator widths leave those fields far more room than that, and 2^30 host terms would take minutes.
// Then M61's and M127's muladd_small_lazy chained at the edges of their stated input ranges.  Host only; built and run by
// tests/test_cxx_api.py.
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "scl_hip/detail/field.hpp"
using namespace sclhip;

static long g_bad = 0, g_checks = 0;
static void check(bool ok, const char* what, long terms) {
  ++g_checks;
  if (!ok) {
    if (g_bad < 20) std::printf("MISMATCH %s at %ld terms\n", what, terms);
    ++g_bad;
  }
}

// x + x + ... (k terms) with the field's reduced add
template <class F>
static typename F::E times(const typename F::Ctx& c, long k, typename F::E x) {
  typename F::E r = F::zero();
  while (k) {
    if (k & 1) r = F::add(c, r, x);
    x = F::add(c, x, x);
    k >>= 1;
  }
  return r;
}

template <class F>
static void acc_case(const typename F::Ctx& c, const char* name, typename F::E a, typename F::E b, long terms) {
  typename F::Acc m = F::acc_zero(), s = F::acc_zero();
  for (long i = 0; i < terms; ++i) {
    F::mac(c, m, a, b);
    F::acc_add(c, s, a);
  }
  char what[96];
  std::snprintf(what, sizeof what, "%s mac", name);
  check(F::eq(F::acc_fold(c, m), times<F>(c, terms, F::mul(c, a, b))), what, terms);
  std::snprintf(what, sizeof what, "%s acc_add", name);
  check(F::eq(F::acc_fold(c, s), times<F>(c, terms, a)), what, terms);
}

template <class F>
static void kacc_case(const typename F::Ctx& c, const char* name, typename F::E k, typename F::E x, typename F::E x_canon) {
  const typename F::KC kc = F::kc_make(c, k);
  typename F::KAcc acc = F::kacc_zero();
  for (long i = 0; i < (long)F::K_TERMS; ++i) F::kmac(c, acc, kc, x);
  char what[96];
  std::snprintf(what, sizeof what, "%s kmac", name);
  check(F::eq(F::kacc_fold(c, acc), times<F>(c, F::K_TERMS, F::mul(c, k, x_canon))), what, F::K_TERMS);
}

static long cap24(long terms) { return terms > (1L << 24) ? (1L << 24) : terms; }

int main() {
  const u64 ONES = ~0ull;
  {  // Mersenne61: a u128 of 64 products < 2^122 each; kmac: three 64-bit columns of 1024 terms, x any 64-bit word
    M61::Ctx c;
    const u64 p = M61::P;
    const u64 vals[] = {p - 1, p - 2, 0x007F7F7F7F7F7F80ull, 0x1F7F7F7F7F7F7F7Full, (1ull << 61) - 2};
    for (u64 a : vals)
      for (u64 b : vals) acc_case<M61>(c, "M61", a, b, M61::ACC_TERMS);
    // constants whose 21-bit limbs (of c and of c 2^32 mod p) are all ones, and words x = 2^64 - 1
    const u64 inv32 = M61::inv(c, 1ull << 32);
    const u64 ks[] = {p - 1, (1ull << 42) - 1, M61::mul(c, (1ull << 42) - 1, inv32), (1ull << 61) - 2};
    for (u64 k : ks)
      for (u64 x : {ONES, p - 1, ONES - 1, (u64)p}) kacc_case<M61>(c, "M61", k, x, M61::from_le_word(c, x));
  }
  {  // Mersenne127: mul_lazy < 2^128 summed into 128 + 64 bits; kmac: six columns of 256 terms, x any 128-bit word
    M127::Ctx c;
    const u128 p = M127::P(), ones = ~(u128)0;
    const u128 vals[] = {p - 1, p - 2, ((u128)1 << 127) - ((u128)1 << 64), ((u128)ONES << 64 >> 1) | ONES};
    for (u128 a : vals) {
      acc_case<M127>(c, "M127", a, p - 1, cap24(M127::ACC_TERMS));
      acc_case<M127>(c, "M127", a, a, 4096);
    }
    for (u128 k : {p - 1, ((u128)1 << 110) - 1, p - 2})
      for (u128 x : {ones, p - 1, p, ones - 1}) kacc_case<M127>(c, "M127", k, x, M127::from_le_word(c, x));
  }
  {  // Mont128: the product columns of LazyCols<4> folded by five words ("any K <= 2^32"), at ACC_TERMS = 2^24
    const u128 R159 = ~(u128)0 - 158;
    const u128 primes[] = {R159, ((u128)1 << 127) - 1, ((u128)0xc381e88f38c0c8fdull << 64) | 0x8712b8bc076f3787ull,
                           ~(u128)0 /* odd, not prime: the fold's arithmetic only */};
    for (u128 p : primes) {
      const Mont128::Ctx c = Mont128::make_ctx(p);
      const u128 low_ones = (((p >> 64) - 1) << 64) | ONES;
      acc_case<Mont128>(c, "Mont128", p - 1, p - 1, Mont128::ACC_TERMS);
      acc_case<Mont128>(c, "Mont128", p - 1, low_ones, 1 << 20);
      acc_case<Mont128>(c, "Mont128", low_ones, low_ones, 1 << 20);
    }
  }
  {  // secp256k1 order and field: LazyCols<8>, ACC_TERMS = 2^24
    const Secp256k1Scalar::Ctx c{};
    typedef Secp256k1Scalar S;
    const S::E pm1 = S::make(S::P(0) - 1, S::P(1), S::P(2), S::P(3));
    acc_case<S>(c, "secp256k1 order", pm1, pm1, S::ACC_TERMS);
    typedef Secp256k1Field Fq;
    const Fq::Ctx d{};
    const Fq::E qm1 = Fq::make(Fq::P(0) - 1, Fq::P(1), Fq::P(2), Fq::P(3));
    const Fq::E top = Fq::make(0, ONES, ONES, ONES);
    acc_case<Fq>(d, "secp256k1 field", qm1, qm1, Fq::ACC_TERMS);
    acc_case<Fq>(d, "secp256k1 field", top, qm1, 1 << 20);
  }
  {  // GF(2^128): an xor accumulator, 2^24 of 2^30 terms
    Gf128::Ctx c;
    const u128 ones = ~(u128)0;
    acc_case<Gf128>(c, "GF(2^128)", ones, ones, (1 << 24) + 1);
    acc_case<Gf128>(c, "GF(2^128)", (u128)1 << 127, ones ^ 1, 1 << 20);
  }
  {  // Z2k: wrapping words, 2^24 of 2^30 terms
    const Z2k64::Ctx c64 = Z2k64::make_ctx(64), c61 = Z2k64::make_ctx(61);
    acc_case<Z2k64>(c64, "Z2k<64>", ONES, ONES, 1 << 24);
    acc_case<Z2k64>(c61, "Z2k<61>", (1ull << 61) - 1, (1ull << 60), 1 << 24);
    const Z2k128::Ctx c128 = Z2k128::make_ctx(128), c127 = Z2k128::make_ctx(127);
    acc_case<Z2k128>(c128, "Z2k<128>", ~(u128)0, ~(u128)0, 1 << 24);
    acc_case<Z2k128>(c127, "Z2k<127>", ((u128)1 << 127) - 1, ((u128)1 << 126), 1 << 22);
  }
  {  // muladd_small_lazy chained at its stated input range.  M61: y, c < 2^62 in, < 2^61 + 4 out
    M61::Ctx c;
    const u64 p = M61::P;
    for (u32 x : {0xFFFFFFFFu, 0x80000000u, 1u, 0u}) {
      u64 y = (1ull << 62) - 1, want = y % p;
      const u64 add = (1ull << 62) - 1, add_mod = add % p;
      for (int i = 0; i < 1000; ++i) {
        y = M61::muladd_small_lazy(y, x, add);
        want = (u64)(((u128)want * x + add_mod) % p);
        check(y < (1ull << 61) + 4 && y % p == want, "M61 muladd_small_lazy", i + 1);
      }
      check(M61::canon(y) == want, "M61 muladd_small canon", 1000);
    }
  }
  {  // M127: y any u128, c < 2^127 in; < 2^127 + 2^34 out
    M127::Ctx c;
    const u128 p = M127::P();
    for (u32 x : {0xFFFFFFFFu, 0x80000001u, 1u, 0u}) {
      u128 y = ~(u128)0;
      u128 want = M127::from_le_word(c, y);
      const u128 add = ((u128)1 << 127) - 1;
      for (int i = 0; i < 1000; ++i) {
        y = M127::muladd_small_lazy(y, x, add);
        want = M127::add(c, M127::mul(c, want, (u128)x), add % p);
        check(y < ((u128)1 << 127) + ((u128)1 << 34) && M127::canon(y) == want, "M127 muladd_small_lazy", i + 1);
        if (i == 500) y = ~(u128)0 - (y & 1), want = M127::from_le_word(c, y);   // back to the top of the input range
      }
    }
  }
  std::printf("%ld checks, %ld mismatches\n", g_checks, g_bad);
  return g_bad != 0;
}
