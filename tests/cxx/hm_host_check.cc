// tests/cxx/hm_host_check.cc -- hm_mask_one, hm_finish_one and hm_mac_step (detail/hm.hpp: products on the fields' lazy
// accumulators, folded at each field's own term bound) against the same values built from the field's own reduced mul / add / sub,
// one operation at a time.  Every field struct of detail/field.hpp; Mont128 at its default prime 2^128 - 159 and at a second
// full-width prime.  Per field: the mask and the finish over operands crossed from {0, 1, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2}
// (all-ones, all-ones - 1 and the two halves for GF(2^128)) and 10^5 uniform tuples; the accumulation -- the inner step of
// apply and of the open -- over 1, 3, 10, 64, 65, 300 and 1100 terms, uniform and with every operand at p - 1 (all ones), which
// is where Mersenne61's bound of 64 products is met at 64 terms and passed at 65 and 300; the prepared-constant form apply uses
// (hm_kmac_step) passes Mersenne127's bound of 256 at 300 terms and Mersenne61's of 1024 at 1100.  Host only; also built with
// -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scl_hip/detail/hm.hpp"
using namespace sclhip;

#define CHECK_SEED 0x243F6A8885A308D3ull
#include "check.hpp"

// sum_i k[i] x[i] through hm_mac_step against reduced mul and add
template <class F>
static void dot_case(const typename F::Ctx& c, const char* name, const std::vector<typename F::E>& k, const std::vector<typename F::E>& x) {
  typename F::Acc acc = F::acc_zero();
  int terms = 0;
  typename F::E want = F::zero();
  for (std::size_t i = 0; i < k.size(); ++i) {
    hm_mac_step<F>(c, acc, terms, k[i], x[i]);
    want = F::add(c, want, F::mul(c, k[i], x[i]));
  }
  check(terms <= (int)F::ACC_TERMS, name, "term count", (long)k.size());
  check(F::eq(F::acc_fold(c, acc), want), name, "accumulate", (long)k.size());
  typename F::KAcc kacc = F::kacc_zero();  // the same sum against prepared constants, as apply takes it
  int kterms = 0;
  for (std::size_t i = 0; i < k.size(); ++i) hm_kmac_step<F>(c, kacc, kterms, F::kc_make(c, k[i]), x[i]);
  check(kterms <= (int)F::K_TERMS, name, "prepared term count", (long)k.size());
  check(F::eq(F::kacc_fold(c, kacc), want), name, "prepared accumulate", (long)k.size());
}

template <class F>
static void run_field(const typename F::Ctx& c, const char* name, long uniform) {
  const auto pool = Gen<F>::pool(c);
  long at = 0;
  auto one = [&](const typename F::E& x, const typename F::E& y, const typename F::E& r) {
    check(F::eq(hm_mask_one<F>(c, x, y, r), F::add(c, F::mul(c, x, y), r)), name, "mask", at);
    check(F::eq(hm_finish_one<F>(c, x, r), F::sub(c, x, r)), name, "finish", at);
    check(F::eq(F::add(c, hm_finish_one<F>(c, x, r), r), x), name, "finish + r", at);
    ++at;
  };
  for (const auto& x : pool)
    for (const auto& y : pool)
      for (const auto& r : pool) one(x, y, r);
  for (long i = 0; i < uniform; ++i) one(Gen<F>::rnd(c), Gen<F>::rnd(c), Gen<F>::rnd(c));
  const typename F::E top = pool[2];  // p - 1; all ones over GF(2^128)
  for (std::size_t terms : {1, 3, 10, 64, 65, 300, 1100}) {
    std::vector<typename F::E> k, x;
    for (std::size_t i = 0; i < terms; ++i) {
      k.push_back(Gen<F>::rnd(c));
      x.push_back(Gen<F>::rnd(c));
    }
    dot_case<F>(c, name, k, x);
    dot_case<F>(c, name, std::vector<typename F::E>(terms, top), std::vector<typename F::E>(terms, top));
    dot_case<F>(c, name, std::vector<typename F::E>(terms, top), x);
  }
}

int main() {
  const long uniform = 100000;
  run_field<M61>(M61::Ctx{}, "Mersenne61", uniform);
  run_field<M127>(M127::Ctx{}, "Mersenne127", uniform);
  run_field<Mont128>(Mont128::make_ctx(~(u128)0 - 158), "Mont128 at 2^128 - 159", uniform);
  // a second full-width prime (p >= 2^127): the third modulus of tests/golden/golden_mont128.json
  run_field<Mont128>(Mont128::make_ctx(((u128)0xc381e88f38c0c8fdull << 64) | 0x8712b8bc076f3787ull), "Mont128 at c381e88f..3787", uniform);
  run_field<Gf128>(Gf128::Ctx{}, "GF(2^128)", uniform);
  run_field<Secp256k1Scalar>(Secp256k1Scalar::Ctx{}, "secp256k1 order", uniform);
  run_field<Secp256k1Field>(Secp256k1Field::Ctx{}, "secp256k1 field", uniform);
  return summary();
}
