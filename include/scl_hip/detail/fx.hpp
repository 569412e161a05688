// include/scl_hip/detail/fx.hpp -- probabilistic truncation of a Shamir sharing (Catrina, de Hoogh), once, for host and device.
//
// x stands for a signed integer in [-2^(k-1), 2^(k-1)); B = k + kappa shared random bits b_0 .. b_(B-1) mask it:
//
//   r = sum_{i<B} 2^i b_i,  r' = sum_{i<shift} 2^i b_i        fx_step, Horner from the top plane down: acc = 2 acc + b_i
//   c = x + 2^(k-1) + r                                        fx_mask_one; opened by the caller
//   c' = c mod 2^shift AS AN INTEGER                           fx_finish_col: the canonical value (after from_mont for the
//                                                              Montgomery fields), masked limb by limb; shift may lie in any limb
//   y = (x + r' - c') 2^-shift                                 fx_finish_one
//
// With 1 <= shift < k <= B <= |p| - 2 the opened c is below 2^(B+1) < p: nothing wraps, and
//   y = floor((x + 2^(k-1)) / 2^shift) + [ (x + 2^(k-1)) mod 2^shift + r' >= 2^shift ] - 2^(k-1-shift),
// floor(x / 2^shift) or that plus one.  A c at or above 2^(B+1) -- an input out of range, planes that were no bits, wrong shares
// -- sets the column's status and yields zero.  The check is best effort: a wrong c below 2^(B+1) passes it.
//
// The weights are powers of two, so there is no field product on the way to c: the Mersenne fields double by moving the bits
// that leave the top back to the bottom (2^61 = 1, 2^127 = 1) and stay lazy -- any word in, a congruent word out, never an
// overflow, one fx_canon at the end --, the Montgomery fields use their add (a residue x R doubles like x).  The Mersenne fields
// multiply by 2^-shift with a rotation; the Montgomery fields with one product by the constant.  The constants -- 2^(k-1),
// 2^-shift, the two masks -- are FxMask<F> / FxFinish<F>, made on the host per call from (k, shift, B) and handed to the kernels as
// arguments.  GF(2^128) and the rings have no such truncation (no integers below a prime to mask; a ring Z2k has no 2^-shift):
// fx_has_trunc says so by tag.  Uses the fields' public add, sub, mul, inv, one, zero, to_mont, from_mont only.
#pragma once

#include "field.hpp"

namespace sclhip {

constexpr int FX_OK = 0, FX_RANGE = 1;  // the status byte

constexpr bool fx_has_trunc(int tag) { return tag == 0 || tag == 1 || tag == 2 || tag == 4 || tag == 7; }

template <class F>
constexpr bool fx_mersenne() {
  return F::TAG == M61::TAG || F::TAG == M127::TAG;
}

// |p|, the bit length of the prime (Mont128: of the context's modulus)
template <class F>
inline int fx_prime_bits(const typename F::Ctx& c) {
  if constexpr (F::TAG == M61::TAG) {
    return 61;
  } else if constexpr (F::TAG == M127::TAG) {
    return 127;
  } else if constexpr (F::TAG == Mont128::TAG) {
    int n = 0;
    for (u128 v = c.p; v; v >>= 1) ++n;
    return n;
  } else {
    return 256;
  }
}

// 2 acc + b.  Mersenne: acc is any word congruent to the sum so far, b < 2^61 (2^127); the result is congruent and fits the word
// (below 2^62, or 2^128) whatever acc was -- p - 1 in every plane included.  Montgomery: canonical in and out.
template <class F>
SCL_HD typename F::E fx_step(const typename F::Ctx& c, const typename F::E& acc, const typename F::E& b) {
  if constexpr (F::TAG == M61::TAG) {
    return ((acc << 1) & M61::P) + (acc >> 60) + b;  // bits 60.. of acc weigh 2^61 = 1 after the doubling
  } else if constexpr (F::TAG == M127::TAG) {
    return ((acc << 1) & M127::P()) + (acc >> 126) + b;
  } else {
    return F::add(c, F::add(c, acc, acc), b);
  }
}

// a lazy sum -> canonical
template <class F>
SCL_HD typename F::E fx_canon(const typename F::E& acc) {
  if constexpr (F::TAG == M61::TAG) {
    const u64 f = (acc & M61::P) + (acc >> 61);  // <= p + 7
    return f >= M61::P ? f - M61::P : f;
  } else if constexpr (F::TAG == M127::TAG) {
    const u128 f = (acc & M127::P()) + (acc >> 127);  // <= p + 1
    return f >= M127::P() ? f - M127::P() : f;
  } else {
    return acc;
  }
}

// the constants of a mask: 2^(k-1) as an element
template <class F>
struct FxMask {
  typename F::E bias;
};

// the constants of a finish
template <class F>
struct FxFinish {
  typename F::E inv;  // 2^-shift as an element (the Montgomery fields; the Mersenne fields rotate by `rot`)
  u64 low[4];         // 2^shift - 1
  u64 high[4];        // the bits from B + 1 up: a canonical c that has one of them is out of range
  int rot;            // |p| - shift
};

// c = x + 2^(k-1) + r
template <class F>
SCL_HD typename F::E fx_mask_one(const typename F::Ctx& c, const FxMask<F>& prm, const typename F::E& x, const typename F::E& r) {
  return F::add(c, F::add(c, x, prm.bias), r);
}

// the canonical integer of an element, little-endian limbs
template <class F>
SCL_HD void fx_limbs(const typename F::Ctx& c, const typename F::E& a, u64 (&w)[F::LIMBS]) {
  if constexpr (F::TAG == M61::TAG) {
    w[0] = a;
  } else if constexpr (F::TAG == M127::TAG) {
    w[0] = (u64)a;
    w[1] = (u64)(a >> 64);
  } else if constexpr (F::TAG == Mont128::TAG) {
    const u128 v = F::from_mont(c, a);
    w[0] = (u64)v;
    w[1] = (u64)(v >> 64);
  } else {
    const typename F::E v = F::from_mont(c, a);
    for (int i = 0; i < 4; ++i) w[i] = v.w[i];
  }
}

// an integer below p, little-endian limbs -> the element
template <class F>
SCL_HD typename F::E fx_from_limbs(const typename F::Ctx& c, const u64 (&w)[F::LIMBS]) {
  if constexpr (F::TAG == M61::TAG) {
    return w[0];
  } else if constexpr (F::TAG == M127::TAG) {
    return ((u128)w[1] << 64) | w[0];
  } else if constexpr (F::TAG == Mont128::TAG) {
    return F::to_mont(c, ((u128)w[1] << 64) | w[0]);
  } else {
    return F::to_mont(c, F::make(w[0], w[1], w[2], w[3]));
  }
}

// the column's part of the finish: c' = c mod 2^shift as an element, and the status of c
template <class F>
SCL_HD typename F::E fx_finish_col(const typename F::Ctx& c, const FxFinish<F>& prm, const typename F::E& opened, int& status) {
  u64 w[F::LIMBS];
  fx_limbs<F>(c, opened, w);
  u64 over = 0;
  for (int i = 0; i < (int)F::LIMBS; ++i) {
    over |= w[i] & prm.high[i];
    w[i] &= prm.low[i];
  }
  status = over ? FX_RANGE : FX_OK;
  return fx_from_limbs<F>(c, w);
}

// a * 2^-shift
template <class F>
SCL_HD typename F::E fx_scale(const typename F::Ctx& c, const FxFinish<F>& prm, const typename F::E& a) {
  if constexpr (F::TAG == M61::TAG) {
    return ((a << prm.rot) & M61::P) | (a >> (61 - prm.rot));  // 2^-shift = 2^(61 - shift): a rotation of the 61 bits, 1 <= rot <= 60
  } else if constexpr (F::TAG == M127::TAG) {
    return ((a << prm.rot) & M127::P()) | (a >> (127 - prm.rot));
  } else {
    return F::mul(c, a, prm.inv);
  }
}

// y = (x + r' - c') 2^-shift; zero where the column's status is set
template <class F>
SCL_HD typename F::E fx_finish_one(const typename F::Ctx& c, const FxFinish<F>& prm, const typename F::E& cp, int status, const typename F::E& x,
                                   const typename F::E& rlow) {
  const typename F::E y = fx_scale<F>(c, prm, F::sub(c, F::add(c, x, rlow), cp));
  if constexpr (F::LIMBS == 4) {  // limb by limb: a conditional expression over a four-limb struct selects between addresses
    typename F::E r;
    for (int i = 0; i < 4; ++i) r.w[i] = status == FX_OK ? y.w[i] : 0;
    return r;
  } else {
    return status == FX_OK ? y : F::zero();
  }
}

// ---- the constants, on the host --------------------------------------------------------------------------------------------
// 2^e as an element, e < |p| - 1: doublings of one (a Montgomery residue doubles like the value it stands for)
template <class F>
inline typename F::E fx_pow2(const typename F::Ctx& c, int e) {
  typename F::E r = F::one(c);
  for (int i = 0; i < e; ++i) r = F::add(c, r, r);
  return r;
}

// 1 <= k <= |p| - 2
template <class F>
inline FxMask<F> fx_make_mask(const typename F::Ctx& c, int k) {
  FxMask<F> prm;
  prm.bias = fx_pow2<F>(c, k - 1);
  return prm;
}

// 1 <= shift < B <= |p| - 2
template <class F>
inline FxFinish<F> fx_make_finish(const typename F::Ctx& c, int shift, int B) {
  FxFinish<F> prm;
  for (int i = 0; i < 4; ++i) {
    const int lo = shift - 64 * i, hi = B + 1 - 64 * i;  // bits of limb i below 2^shift; below 2^(B+1)
    prm.low[i] = lo >= 64 ? ~(u64)0 : lo <= 0 ? 0 : (((u64)1 << lo) - 1);
    prm.high[i] = hi >= 64 ? 0 : hi <= 0 ? ~(u64)0 : ~(((u64)1 << hi) - 1);
  }
  prm.rot = fx_prime_bits<F>(c) - shift;
  if constexpr (fx_mersenne<F>()) prm.inv = F::one(c);
  else prm.inv = F::inv(c, fx_pow2<F>(c, shift));
  return prm;
}

// ---- the per-secret host forms (include/scl_hip/ss/trunc.h) -------------------------------------------------------------------
// sum_{i<count} 2^i bits[i * stride], canonical
template <class F>
inline typename F::E fx_compose_host(const typename F::Ctx& c, const typename F::E* bits, size_t stride, int count) {
  typename F::E acc = F::zero();
  for (int i = count - 1; i >= 0; --i) acc = fx_step<F>(c, acc, bits[(size_t)i * stride]);
  return fx_canon<F>(acc);
}

}  // namespace sclhip
