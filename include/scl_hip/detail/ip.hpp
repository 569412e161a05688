// include/scl_hip/detail/ip.hpp -- the per-element arithmetic of inner and matrix products of Shamir sharings at one opening,
// once, for host and device.
//
//   accumulate   acc += x_k y_k                          two variable operands on a lazy accumulator; `terms` counts what it holds
//   finish       [d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t the addend goes in as ONE MORE TERM, then one fold
// The accumulator is any type with zero / mac / add / fold and a TERMS bound: IpAcc<F> below (the field's own Acc, host and
// device) or the matrix kernels' MatAcc<F> (csrc/kernels.hpp, device only: column sums for Mersenne127, for the reason given
// above it).  The step restates hm_mac_step / hm_refold (hm.hpp) on that interface: at the bound the accumulator is folded into
// itself and the canonical partial sum goes back in through add, counting as one term (a canonical element is never larger than
// a product of two).
//
// THE ADDEND COUNTS.  A field promises F::ACC_TERMS terms and nothing beyond: Mersenne61 holds 64 products in 128 bits and a
// 65th wraps (65 (p - 1)^2 > 2^128).  So a sum of exactly 64 products plus r2 folds BEFORE the addend goes in: the addend takes
// its term through ip_take_term as a product does, and the accumulator never holds more than the field promises.  Every
// residue has one canonical representative, so each result is bit-identical to the same value built one reduced operation at a
// time (tests/cxx/ip_host_check.cc).
#pragma once

#include "hm.hpp"

namespace sclhip {

// the field's own lazy accumulator behind the interface of the matrix kernels' MatAcc
template <class F>
struct IpAcc {
  typename F::Acc a;
  enum { TERMS = F::ACC_TERMS };
  SCL_HD void zero() { a = F::acc_zero(); }
  SCL_HD void mac(const typename F::Ctx& c, const typename F::E& x, const typename F::E& y) { F::mac(c, a, x, y); }
  SCL_HD void add(const typename F::Ctx& c, const typename F::E& x) { F::acc_add(c, a, x); }
  SCL_HD typename F::E fold(const typename F::Ctx& c) const { return F::acc_fold(c, a); }
};

// the accumulator folded into itself: afterwards it holds ONE term, the canonical partial sum (hm_refold on the interface)
template <class F, class A>
SCL_HD void ip_refold(const typename F::Ctx& ctx, A& acc) {
  const typename F::E part = acc.fold(ctx);
  acc.zero();
  acc.add(ctx, part);
}

// does one more term fit?
template <class A>
SCL_HD bool ip_full(int terms) {
  return terms + 1 > (int)A::TERMS;
}

// THE COUNT, in one place.  COUNT accumulators that take their terms together -- one, the W columns of a lane, the TI x TL tile of
// the matrix kernel -- share one count.  Before a term (a product or the addend) goes into them, this makes room for it in all of
// them and counts it; the caller then does the mac or the add.
template <class F, int COUNT, class A>
SCL_HD void ip_take_term(const typename F::Ctx& ctx, A* acc, int& terms) {
  if (ip_full<A>(terms)) {
#pragma unroll
    for (int c = 0; c < COUNT; ++c) ip_refold<F>(ctx, acc[c]);
    terms = 1;
  }
  ++terms;
}

// acc += x y
template <class F, class A>
SCL_HD void ip_mac_step(const typename F::Ctx& ctx, A& acc, int& terms, const typename F::E& x, const typename F::E& y) {
  ip_take_term<F, 1>(ctx, &acc, terms);
  acc.mac(ctx, x, y);
}

// the addend and the fold, for a caller that has taken the addend's term (ip_take_term)
template <class F, class A>
SCL_HD typename F::E ip_add_fold(const typename F::Ctx& ctx, A& acc, bool has_r2, const typename F::E& r2) {
  if (has_r2) acc.add(ctx, r2);
  return acc.fold(ctx);
}

// the addend as one more term, then the fold; without an addend the fold alone
template <class F, class A>
SCL_HD typename F::E ip_finish(const typename F::Ctx& ctx, A& acc, int terms, bool has_r2, const typename F::E& r2) {
  if (has_r2) ip_take_term<F, 1>(ctx, &acc, terms);
  return ip_add_fold<F>(ctx, acc, has_r2, r2);
}

// sum_{k<terms} x[k * xs] y[k * ys] (+ r2): the whole inner product of one column on the field's own accumulator -- what the
// host check and the C++ mirror's host mode run
template <class F>
SCL_HD typename F::E ip_dot_one(const typename F::Ctx& ctx, const typename F::E* x, size_t xs, const typename F::E* y, size_t ys,
                                size_t nterms, const typename F::E* r2) {
  IpAcc<F> acc;
  acc.zero();
  int terms = 0;
  for (size_t k = 0; k < nterms; ++k) ip_mac_step<F>(ctx, acc, terms, x[k * xs], y[k * ys]);
  return ip_finish<F>(ctx, acc, terms, r2 != nullptr, r2 ? *r2 : F::zero());
}

}  // namespace sclhip
