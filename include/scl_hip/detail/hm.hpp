// include/scl_hip/detail/hm.hpp -- the per-element arithmetic of honest-majority (Damgard-Nielsen) multiplication, once, for
// host and device.
//
//   mask     [d]_2t = [x]_t [y]_t + [R]_2t            one product, one reduction: mac, acc_add, acc_fold
//   open     d = sum_j lambda_j [d]_j                 the fields' lazy accumulator, folded at each field's own term bound
//   finish   [z]_t = d - [R]_t                        the field's sub
//   apply    out_k = sum_i M[k][i] in_i               one accumulator per output row, against PREPARED constants: an entry of M
//                                                     is the same for every lane, so it is split once (F::kc_make) and a term
//                                                     costs F::kmac -- for the Mersenne fields a handful of independent 32 x 32
//                                                     multiply-adds without carries; the other fields alias Acc / mac
// A lazy accumulator (field.hpp: Acc, mac, acc_add, acc_fold) holds F::ACC_TERMS products.  hm_mac_step counts them and, at the
// bound, folds the accumulator into itself (hm_refold): the canonical partial sum goes back in through acc_add and counts as one term
// (a canonical element is never larger than a product of two), so no second register set carries the running sum.  Every
// residue has one canonical representative, so each result is bit-identical to the same value built one reduced operation at a
// time (tests/cxx/hm_host_check.cc).
#pragma once

#include "field.hpp"

namespace sclhip {

// x y + r2, canonical
template <class F>
SCL_HD typename F::E hm_mask_one(const typename F::Ctx& ctx, const typename F::E& x, const typename F::E& y, const typename F::E& r2) {
  typename F::Acc acc = F::acc_zero();
  F::mac(ctx, acc, x, y);
  F::acc_add(ctx, acc, r2);
  return F::acc_fold(ctx, acc);
}

// the accumulator folded into itself: afterwards it holds ONE term, the canonical partial sum
template <class F>
SCL_HD void hm_refold(const typename F::Ctx& ctx, typename F::Acc& acc) {
  const typename F::E part = F::acc_fold(ctx, acc);
  acc = F::acc_zero();
  F::acc_add(ctx, acc, part);
}

// acc += k x, the inner step of apply and of the open; `terms` counts what acc holds
template <class F>
SCL_HD void hm_mac_step(const typename F::Ctx& ctx, typename F::Acc& acc, int& terms, const typename F::E& k, const typename F::E& x) {
  if (terms + 1 > (int)F::ACC_TERMS) {
    hm_refold<F>(ctx, acc);
    terms = 1;
  }
  F::mac(ctx, acc, k, x);
  ++terms;
}

// the same against a prepared constant, the inner step of apply: folds at F::K_TERMS.  The partial sum goes back in as one
// term, multiplied by the prepared constant one (KAcc has no plain addition).
template <class F>
SCL_HD void hm_krefold(const typename F::Ctx& ctx, typename F::KAcc& acc) {
  const typename F::E part = F::kacc_fold(ctx, acc);
  acc = F::kacc_zero();
  F::kmac(ctx, acc, F::kc_make(ctx, F::one(ctx)), part);
}
template <class F>
SCL_HD void hm_kmac_step(const typename F::Ctx& ctx, typename F::KAcc& acc, int& terms, const typename F::KC& k, const typename F::E& x) {
  if (terms + 1 > (int)F::K_TERMS) {
    hm_krefold<F>(ctx, acc);
    terms = 1;
  }
  F::kmac(ctx, acc, k, x);
  ++terms;
}

// opened - r, canonical
template <class F>
SCL_HD typename F::E hm_finish_one(const typename F::Ctx& ctx, const typename F::E& opened, const typename F::E& r) {
  return F::sub(ctx, opened, r);
}

}  // namespace sclhip
