// include/scl_hip/detail/cmp.hpp -- the bitwise less-than of a public integer against shared bits, and the exact results that are
// linear on top of it, once, for host and device.
//
// c' is a public w-bit integer with the bits c_0 .. c_(w-1), r' = sum_{i<w} 2^i b_i is held as shared bits [b_i].  A node stands
// for a run of bit positions: lt = [c' < r' on the run], eq = [c' = r' on the run].
//
//   leaf i      lt_i = (1 - c_i) b_i,  eq_i = c_i ? b_i : 1 - b_i        linear in [b_i]: c_i is public (cmp_leaf, a select)
//   combine     lt = lt_hi + eq_hi lt_lo,  eq = eq_hi eq_lo              one product each (cmp_combine_lt / _eq)
//   identity    lt = 0, eq = 1                                           what a node without a partner combines with
//
// A product of two degree-t sharings is a degree-2t sharing; it is re-randomised on the spot, d = ... + [R]_2t, so a level is one
// Damgard-Nielsen multiplication (detail/hm.hpp): eq_hi lt_lo + lt_hi + R is one product and two addends, folded once through the
// field's lazy accumulator.  ceil(log2 w) levels, at least one, halve the node count; the last one needs lt only.
//
//   a = c' - r' + 2^w lt                                      x mod 2^w                          CMP_MOD
//   (x - a) 2^-w = (x - c' + r') 2^-w - lt                    floor(x / 2^w), exactly            CMP_TRUNC
//   -(x - a) 2^-w                                             [x < 0] at w = k - 1               CMP_LTZ
//
// Each finish costs one multiplication by a power of two: a rotation for the Mersenne fields, one constant product for the
// Montgomery fields (fx_scale of detail/fx.hpp, whose integer view of an element -- fx_limbs, fx_from_limbs -- is used for the
// bits of c as well).  Uses the fields' public add, sub, neg, one, zero and the lazy accumulator only.
#pragma once

#include "fx.hpp"

namespace sclhip {

constexpr int CMP_MOD = 0, CMP_TRUNC = 1, CMP_LTZ = 2;  // `what` of the finish
constexpr unsigned CMP_LT_ONLY = 1u;                    // the flag of a last level

// max(1, ceil(log2 w)), w >= 1
constexpr size_t cmp_levels(size_t w) {
  size_t n = 0;
  for (size_t cnt = w; cnt > 1; cnt = (cnt + 1) / 2) ++n;
  return n < 1 ? 1 : n;
}

// double-sharing planes over all levels: 2 ceil(cnt / 2) per level, 1 for the last
constexpr size_t cmp_planes(size_t w) {
  size_t planes = 0, cnt = w;
  for (size_t l = cmp_levels(w); l > 1; --l) {
    cnt = (cnt + 1) / 2;
    planes += 2 * cnt;
  }
  return planes + 1;
}

// cond ? a : b, limb by limb for the four-limb fields (a conditional expression over a struct selects between addresses)
template <class F>
SCL_HD typename F::E cmp_select(bool cond, const typename F::E& a, const typename F::E& b) {
  if constexpr (F::LIMBS == 4) {
    typename F::E r;
    for (int i = 0; i < 4; ++i) r.w[i] = cond ? a.w[i] : b.w[i];
    return r;
  } else {
    return cond ? a : b;
  }
}

// (a & mask) | (b & ~mask) in every limb: mask is all ones or zero, the public bit spread over a word
template <class F>
SCL_HD typename F::E cmp_blend(u64 mask, const typename F::E& a, const typename F::E& b) {
  if constexpr (F::LIMBS == 4) {
    typename F::E r;
    for (int i = 0; i < 4; ++i) r.w[i] = (a.w[i] & mask) | (b.w[i] & ~mask);
    return r;
  } else if constexpr (F::LIMBS == 2) {
    const u128 m = ((u128)mask << 64) | mask;
    return (a & m) | (b & ~m);
  } else {
    return (a & mask) | (b & ~mask);
  }
}

// all ones where integer bit i of the limb that holds it is set
SCL_HD u64 cmp_bit_mask(u64 limb, int i) { return (u64)0 - ((limb >> (i & 63)) & 1); }

// the leaf of bit i: `mask` the public bit c_i as a word of ones or zeros, b the share of b_i
template <class F>
SCL_HD void cmp_leaf(const typename F::Ctx& ctx, u64 mask, const typename F::E& b, typename F::E& lt, typename F::E& eq) {
  lt = cmp_blend<F>(mask, F::zero(), b);
  eq = cmp_blend<F>(mask, b, F::sub(ctx, F::one(ctx), b));
}

// lt_hi + eq_hi lt_lo + r2, canonical
template <class F>
SCL_HD typename F::E cmp_combine_lt(const typename F::Ctx& ctx, const typename F::E& lt_hi, const typename F::E& eq_hi, const typename F::E& lt_lo,
                                    const typename F::E& r2) {
  typename F::Acc acc = F::acc_zero();
  F::mac(ctx, acc, eq_hi, lt_lo);
  F::acc_add(ctx, acc, lt_hi);
  F::acc_add(ctx, acc, r2);
  return F::acc_fold(ctx, acc);
}

// eq_hi eq_lo + r2, canonical
template <class F>
SCL_HD typename F::E cmp_combine_eq(const typename F::Ctx& ctx, const typename F::E& eq_hi, const typename F::E& eq_lo, const typename F::E& r2) {
  typename F::Acc acc = F::acc_zero();
  F::mac(ctx, acc, eq_hi, eq_lo);
  F::acc_add(ctx, acc, r2);
  return F::acc_fold(ctx, acc);
}

// the column's part of the first level: the opened c -> its status, c mod 2^w as limbs (zero where the status is set) and as an
// element.  `prm`: fx_make_finish(w, B), whose masks are the ones of the probabilistic finish.
template <class F>
SCL_HD typename F::E cmp_open_col(const typename F::Ctx& ctx, const FxFinish<F>& prm, const typename F::E& opened, u64 (&w)[F::LIMBS], int& status) {
  fx_limbs<F>(ctx, opened, w);
  u64 over = 0;
  for (int i = 0; i < (int)F::LIMBS; ++i) over |= w[i] & prm.high[i];
  status = over ? FX_RANGE : FX_OK;
  for (int i = 0; i < (int)F::LIMBS; ++i) w[i] = over ? 0 : (w[i] & prm.low[i]);
  return fx_from_limbs<F>(ctx, w);
}

// the constants of a finish: the one power of two (CMP_MOD: 2^w, else 2^-w) in the form fx_scale takes
template <class F>
struct CmpFinish {
  FxFinish<F> scale;
  int what;
};

// 1 <= w <= |p| - 3
template <class F>
inline CmpFinish<F> cmp_make_finish(const typename F::Ctx& ctx, int w, int what) {
  CmpFinish<F> prm;
  prm.scale = fx_make_finish<F>(ctx, w, w + 1);  // rot = |p| - w, inv = 2^-w
  if (what == CMP_MOD) {
    prm.scale.rot = w;
    if constexpr (!fx_mersenne<F>()) prm.scale.inv = fx_pow2<F>(ctx, w);
  }
  prm.what = what;
  return prm;
}

// one element of the finish; zero where the column's status is set.  x is not looked at for CMP_MOD.
template <class F>
SCL_HD typename F::E cmp_finish_one(const typename F::Ctx& ctx, const CmpFinish<F>& prm, const typename F::E& cmod, int status, const typename F::E& lt,
                                    const typename F::E& rlow, const typename F::E& x) {
  typename F::E y;
  if (prm.what == CMP_MOD) {
    y = F::add(ctx, F::sub(ctx, cmod, rlow), fx_scale<F>(ctx, prm.scale, lt));
  } else {
    y = F::sub(ctx, fx_scale<F>(ctx, prm.scale, F::add(ctx, F::sub(ctx, x, cmod), rlow)), lt);
    if (prm.what == CMP_LTZ) y = F::neg(ctx, y);
  }
  return cmp_select<F>(status == FX_OK, y, F::zero());
}

}  // namespace sclhip
