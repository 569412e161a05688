// tests/cxx/beaver_host_check.cc -- beaver_finish_one / beaver_mask_one (detail/beaver.hpp: two products on the lazy accumulator,
// one reduction) against the same value built from the field's own reduced mul / add, one operation at a time.  Every field struct
// of detail/field.hpp and the ring widths given on the command line (tests/test_beaver_host.py passes extremes.RING_BITS); Mont128
// at its default prime 2^128 - 159 and at a second full-width prime.  Per field: the five operands crossed over {0, 1, p - 1,
// p - 2, (p - 1) / 2, (p + 1) / 2} (all-ones, all-ones - 1 and the two halves for GF(2^128) and the rings) -- which holds all
// five at p - 1, at 0 and at 1, and b + d wrapping to 0 (p - 1 and 1; the halves), to p - 1 (p - 2 and 1; twice (p - 1) / 2) and
// to p - 2 (twice p - 1) --, both values of add_ed, and 10^5 uniform tuples.  Host only; also built with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scl_hip/detail/beaver.hpp"
using namespace sclhip;

#define CHECK_SEED 0x243F6A8885A308D3ull
#include "check.hpp"

static void check(bool ok, const char* what, long at, int add_ed) {
  ++g_checks;
  if (!ok) {
    if (g_bad < 20) std::printf("MISMATCH %s tuple %ld add_ed=%d\n", what, at, add_ed);
    ++g_bad;
  }
}

template <class F>
static typename F::E reference(const typename F::Ctx& c, const typename F::E& e, const typename F::E& d, const typename F::E& a,
                               const typename F::E& b, const typename F::E& cc, bool add_ed) {
  typename F::E z = F::add(c, F::add(c, F::mul(c, e, b), F::mul(c, d, a)), cc);
  if (add_ed) z = F::add(c, z, F::mul(c, e, d));
  return z;
}

template <class F>
static void one_tuple(const typename F::Ctx& c, const char* name, long at, const typename F::E& e, const typename F::E& d,
                      const typename F::E& a, const typename F::E& b, const typename F::E& cc) {
  for (int add_ed = 0; add_ed < 2; ++add_ed)
    check(F::eq(beaver_finish_one<F>(c, e, d, a, b, cc, add_ed != 0), reference<F>(c, e, d, a, b, cc, add_ed != 0)), name, at, add_ed);
  // the mask: (x - a) + a == x, with e and a standing in for x and a
  check(F::eq(F::add(c, beaver_mask_one<F>(c, e, a), a), e), name, at, -1);
}

template <class F>
static void run_field(const typename F::Ctx& c, const char* name, long uniform) {
  const auto pool = Gen<F>::pool(c);
  long at = 0;
  for (const auto& e : pool)
    for (const auto& d : pool)
      for (const auto& a : pool)
        for (const auto& b : pool)
          for (const auto& cc : pool) one_tuple<F>(c, name, at++, e, d, a, b, cc);
  for (long i = 0; i < uniform; ++i) {
    const auto e = Gen<F>::rnd(c), d = Gen<F>::rnd(c), a = Gen<F>::rnd(c), b = Gen<F>::rnd(c), cc = Gen<F>::rnd(c);
    one_tuple<F>(c, name, at++, e, d, a, b, cc);
  }
}

int main(int argc, char** argv) {
  const long uniform = 100000;
  run_field<M61>(M61::Ctx{}, "Mersenne61", uniform);
  run_field<M127>(M127::Ctx{}, "Mersenne127", uniform);
  run_field<Mont128>(Mont128::make_ctx(~(u128)0 - 158), "Mont128 at 2^128 - 159", uniform);
  // a second full-width prime (p >= 2^127): the third modulus of tests/golden/golden_mont128.json
  run_field<Mont128>(Mont128::make_ctx(((u128)0xc381e88f38c0c8fdull << 64) | 0x8712b8bc076f3787ull), "Mont128 at c381e88f..3787", uniform);
  run_field<Gf128>(Gf128::Ctx{}, "GF(2^128)", uniform);
  run_field<Secp256k1Scalar>(Secp256k1Scalar::Ctx{}, "secp256k1 order", uniform);
  run_field<Secp256k1Field>(Secp256k1Field::Ctx{}, "secp256k1 field", uniform);
  int rings = 0;
  for (int i = 1; i < argc; ++i) {
    const int K = std::atoi(argv[i]);
    if (K < 1 || K > 128) {
      std::printf("bad ring width %s\n", argv[i]);
      return 2;
    }
    char name[32];
    std::snprintf(name, sizeof name, "Z2k<%d>", K);
    if (K <= 64) run_field<Z2k64>(Z2k64::make_ctx(K), name, uniform);
    else run_field<Z2k128>(Z2k128::make_ctx(K), name, uniform);
    ++rings;
  }
  std::printf("%d rings, %ld checks, %ld mismatches\n", rings, g_checks, g_bad);
  return g_bad != 0;
}
