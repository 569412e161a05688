// tests/cxx/ip_host_check.cc -- ip_mac_step, ip_finish and ip_dot_one (detail/ip.hpp: sums of products of two variable operands
// on the fields' lazy accumulators, folded at each field's own term bound, the addend counting as a term) against the same values
// built from the field's own reduced mul and add, one operation at a time.  Every field struct of detail/field.hpp; Mont128 at its
// default prime 2^128 - 159 and at a second full-width prime.  Per field, at the term counts of tests/test_gpu_ip.py -- 1, 2, 3,
// 4, 7, 63, 64, 65, 127, 128, 129 and 300 -- with and without the addend: uniform operands, every operand at p - 1 (all ones over
// GF(2^128)), and p - 1 against uniform.  Mersenne61's bound of 64 terms is met by 63 products and the addend, passed by 64
// products and the addend (the fold BEFORE the addend), and passed twice at 128 and 129; the term count never exceeds the bound.
// A tile's accumulators under one count (the matrix kernel's form: ip_take_term over four, ip_add_fold) give the same values.
// Host only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scl_hip/detail/ip.hpp"
using namespace sclhip;

#define CHECK_SEED 0x13198A2E03707344ull
#include "check.hpp"

// sum_k x[k] y[k] (+ r2): ip_dot_one, the step by hand with its count watched, and a 2 x 2 tile under one count
template <class F>
static void dot_case(const typename F::Ctx& c, const char* name, const std::vector<typename F::E>& x, const std::vector<typename F::E>& y,
                     const typename F::E* r2) {
  const long K = (long)x.size();
  typename F::E want = F::zero();
  for (long k = 0; k < K; ++k) want = F::add(c, want, F::mul(c, x[k], y[k]));
  if (r2) want = F::add(c, want, *r2);
  check(F::eq(ip_dot_one<F>(c, x.data(), 1, y.data(), 1, x.size(), r2), want), name, r2 ? "dot + r2" : "dot", K);

  IpAcc<F> acc;
  acc.zero();
  int terms = 0, peak = 0;
  for (long k = 0; k < K; ++k) {
    ip_mac_step<F>(c, acc, terms, x[k], y[k]);
    if (terms > peak) peak = terms;
  }
  check(peak <= (int)F::ACC_TERMS, name, "term count", K);
  const bool folds_for_addend = r2 && ip_full<IpAcc<F>>(terms);
  check(folds_for_addend == (r2 && terms == (int)F::ACC_TERMS), name, "addend counts as a term", K);
  check(F::eq(ip_finish<F>(c, acc, terms, r2 != nullptr, r2 ? *r2 : F::zero()), want), name, "step + finish", K);

  // the tile: acc[i][l] = sum_k xs[i][k] ys[l][k], xs[1] and ys[1] the operands reversed
  IpAcc<F> tile[2][2];
  for (auto& row : tile)
    for (auto& a : row) a.zero();
  int cnt = 0;
  for (long k = 0; k < K; ++k) {
    const typename F::E xs[2] = {x[k], x[K - 1 - k]}, ys[2] = {y[k], y[K - 1 - k]};
    ip_take_term<F, 4>(c, &tile[0][0], cnt);
    if (cnt > peak) peak = cnt;
    for (int i = 0; i < 2; ++i)
      for (int l = 0; l < 2; ++l) tile[i][l].mac(c, xs[i], ys[l]);
  }
  if (r2) ip_take_term<F, 4>(c, &tile[0][0], cnt);
  check(cnt <= (int)F::ACC_TERMS && peak <= (int)F::ACC_TERMS, name, "tile term count", K);
  for (int i = 0; i < 2; ++i)
    for (int l = 0; l < 2; ++l) {
      typename F::E w = F::zero();
      for (long k = 0; k < K; ++k) w = F::add(c, w, F::mul(c, i ? x[K - 1 - k] : x[k], l ? y[K - 1 - k] : y[k]));
      if (r2) w = F::add(c, w, *r2);
      check(F::eq(ip_add_fold<F>(c, tile[i][l], r2 != nullptr, r2 ? *r2 : F::zero()), w), name, "tile", K * 4 + i * 2 + l);
    }
}

template <class F>
static void run_field(const typename F::Ctx& c, const char* name) {
  const typename F::E top = Gen<F>::top(c);
  for (std::size_t terms : {1, 2, 3, 4, 7, 63, 64, 65, 127, 128, 129, 300}) {
    for (int rep = 0; rep < 20; ++rep) {
      std::vector<typename F::E> x, y;
      for (std::size_t i = 0; i < terms; ++i) {
        x.push_back(Gen<F>::rnd(c));
        y.push_back(Gen<F>::rnd(c));
      }
      const typename F::E r = Gen<F>::rnd(c);
      const std::vector<typename F::E> tops(terms, top);
      for (const typename F::E* r2 : {(const typename F::E*)nullptr, &r, &top}) {
        dot_case<F>(c, name, x, y, r2);
        dot_case<F>(c, name, tops, tops, r2);
        dot_case<F>(c, name, tops, y, r2);
        dot_case<F>(c, name, x, x, r2);  // x == y: sums of squares
      }
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
