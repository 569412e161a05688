// tests/cxx/vf_host_check.cc -- vf_take, vf_take_partial, vf_combine_one and vf_sum_partials (detail/vf.hpp: random linear
// combinations along N on the fields' lazy accumulators, folded at each field's own term bound through ip_take_term) against the
// same values built from the field's own reduced mul and add, one operation at a time.  Every field struct of detail/field.hpp;
// Mont128 at its default prime 2^128 - 159 and at a second full-width prime.  Per field, at 1, 2, 3, 63, 64, 65, 127, 128, 129 and
// 300 terms: every operand at p - 1 (all ones over GF(2^128)) -- terms of (p-1)(p-1) in the plain form and of (p-1)(p-1)(p-1) in
// the product form, where x y is reduced first and is one term --, uniform operands, and p - 1 against uniform; the REPS
// accumulators of a column under one count, as the kernels keep them; the second stage over as many canonical partials.  The term
// count never exceeds the field's bound.  On the device a lane passes Mersenne61's 64 terms from 2^24 columns of one row on
// (docs/kernels/vf.md): tests/test_gpu_vf.py reaches that with worst-case operands through the streaming kernel and with the
// PRG's coins through the fused one, which cannot be fed the worst case -- for that path this program stands.
// Host only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scl_hip/detail/vf.hpp"
using namespace sclhip;

#define CHECK_SEED 0x243F6A8885A308D3ull
#include "check.hpp"

// out_j = sum_s rho_j[s] x[s] (y[s]) for two coefficient vectors (rho and rho reversed) under ONE count, and vf_combine_one
template <class F, bool PROD>
static void combine_case(const typename F::Ctx& c, const char* name, const std::vector<typename F::E>& rho, const std::vector<typename F::E>& x,
                         const std::vector<typename F::E>& y) {
  typedef typename F::E E;
  const long n = (long)x.size();
  const char* form = PROD ? "product" : "plain";
  E want[2] = {F::zero(), F::zero()};
  for (long s = 0; s < n; ++s) {
    const E m = PROD ? F::mul(c, x[s], y[s]) : x[s];  // one reduced operation at a time
    want[0] = F::add(c, want[0], F::mul(c, rho[s], m));
    want[1] = F::add(c, want[1], F::mul(c, rho[n - 1 - s], m));
  }
  check(F::eq(vf_combine_one<F>(c, rho.data(), x.data(), PROD ? y.data() : nullptr, x.size()), want[0]), name, form, n);

  IpAcc<F> acc[2];
  acc[0].zero(), acc[1].zero();
  int terms = 0, peak = 0;
  for (long s = 0; s < n; ++s) {
    const E cv[2] = {rho[s], rho[n - 1 - s]};
    vf_take<F, 2, PROD>(c, acc, terms, cv, x[s], y[s]);
    if (terms > peak) peak = terms;
  }
  check(peak <= (int)F::ACC_TERMS, name, "term count", n);
  check(F::eq(acc[0].fold(c), want[0]) && F::eq(acc[1].fold(c), want[1]), name, PROD ? "product, two repetitions" : "plain, two repetitions", n);
}

// the second stage: n canonical partials
template <class F>
static void partial_case(const typename F::Ctx& c, const char* name, const std::vector<typename F::E>& part) {
  typedef typename F::E E;
  E want = F::zero();
  for (const E& p : part) want = F::add(c, want, p);
  check(F::eq(vf_sum_partials<F>(c, part.data(), part.size()), want), name, "partials", (long)part.size());
  IpAcc<F> acc;
  acc.zero();
  int terms = 0, peak = 0;
  for (const E& p : part) {
    vf_take_partial<F>(c, acc, terms, p);
    if (terms > peak) peak = terms;
  }
  check(peak <= (int)F::ACC_TERMS && F::eq(acc.fold(c), want), name, "partials, count watched", (long)part.size());
}

template <class F>
static void run_field(const typename F::Ctx& c, const char* name) {
  typedef typename F::E E;
  const E top = Gen<F>::top(c);
  check(F::eq(vf_combine_one<F>(c, nullptr, nullptr, nullptr, 0), F::zero()) && F::eq(vf_sum_partials<F>(c, nullptr, 0), F::zero()), name,
        "the empty sum is zero", 0);
  for (std::size_t n : {1, 2, 3, 63, 64, 65, 127, 128, 129, 300}) {
    const std::vector<E> tops(n, top);
    combine_case<F, false>(c, name, tops, tops, tops);  // n terms of (p-1)(p-1)
    combine_case<F, true>(c, name, tops, tops, tops);   // n terms of (p-1)(p-1)(p-1)
    partial_case<F>(c, name, tops);
    for (int rep = 0; rep < 20; ++rep) {
      std::vector<E> rho, x, y;
      for (std::size_t i = 0; i < n; ++i) {
        rho.push_back(Gen<F>::rnd(c));
        x.push_back(Gen<F>::rnd(c));
        y.push_back(Gen<F>::rnd(c));
      }
      combine_case<F, false>(c, name, rho, x, y);
      combine_case<F, true>(c, name, rho, x, y);
      combine_case<F, true>(c, name, rho, x, x);  // x == y: sum rho x^2
      combine_case<F, false>(c, name, tops, x, y);
      combine_case<F, true>(c, name, rho, tops, y);
      partial_case<F>(c, name, x);
    }
  }
}

int main() {
  run_field<M61>(M61::Ctx{}, "Mersenne61");
  run_field<M127>(M127::Ctx{}, "Mersenne127");
  run_field<Mont128>(Mont128::make_ctx(~(u128)0 - 158), "Mont128 at 2^128 - 159");
  // a second full-width prime (p >= 2^127): the third modulus of tests/golden/golden_mont128.json
  run_field<Mont128>(Mont128::make_ctx(((u128)0xc381e88f38c0c8fdull << 64) | 0x8712b8bc076f3787ull), "Mont128 at c381e88f..3787");
  run_field<Gf128>(Gf128::Ctx{}, "GF(2^128)");
  run_field<Secp256k1Scalar>(Secp256k1Scalar::Ctx{}, "secp256k1 order");
  run_field<Secp256k1Field>(Secp256k1Field::Ctx{}, "secp256k1 field");
  return summary();
}
