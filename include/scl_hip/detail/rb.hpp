// include/scl_hip/detail/rb.hpp -- modular square roots and the finish of a random shared bit, once, for host and device.
//
// One algorithm for every prime field, p - 1 = 2^s q with q odd (constant-time Tonelli-Shanks; only the constants differ):
//
//   w = a^((q-1)/2),  x = a w,  b = x w = a^q                      one chain of about the field's bit length
//   with g = z^q for a fixed non-residue z, for i = s-1 .. 1:
//       t = b^(2^(i-1));  where t != 1:  x *= g,  b *= g^2;  then g = g^2          (a select, no branch on data)
//   accept when x^2 == a, else a is a non-residue.
//
// The invariant is x^2 = a b; a residue's b has order dividing 2^(s-1), and each round halves it.  s = 1 has no rounds.
// The inverse root costs no second chain: 1/a = w^2 b0^(2^s - 1) (b0 the first b), so 1/x = x / a; for s = 1 it is w itself
// (a w^2 = 1).  THE CANONICAL ROOT is the one whose integer value -- what FF::write serialises, after from_mont for the
// Montgomery fields -- is even; the other one on request.  Zero has the root zero (and the "inverse" zero) and its own status.
//
//   field             s    (q-1)/2
//   Mersenne61        1    2^59 - 1      the addition chain of M61::inv passes through it (x59)
//   Mersenne127       1    2^125 - 1     the addition chain of M127::inv (x125)
//   secp256k1 prime   1    (p-3)/4       an addition chain over its runs of ones (223, 22): 253 squarings, 15 products
//   secp256k1 order   6    (q-1)/2       fixed 2-bit windows; the exponent is the same in every lane
//   Mont128           from the modulus (5 for 2^128 - 159, 1 for 2^127 - 1): fixed 2-bit windows over the run-time exponent
//
// The constants -- s, the exponent, g, 2^-1 -- are RbParams<F>, derived on the host from the prime alone (rb_make_params: the
// non-residue is the smallest integer that fails Euler's criterion) and handed to the kernels as arguments.  GF(2^128) and the
// rings have no such roots (squaring is a bijection of GF(2^128); a ring is no field): rb_has_roots says so by tag.
// Uses the fields' public mul, sqr, sqn_mul, add, neg, inv, from_mont, is_zero, eq, one only.
#pragma once

#include "field.hpp"

namespace sclhip {

constexpr int RB_OK = 0, RB_ZERO = 1, RB_NONRESIDUE = 2;  // the status byte
constexpr unsigned RB_ODD_ROOT = 1u, RB_INVERSE = 2u;     // the flags of scl_rb_sqrt

constexpr bool rb_has_roots(int tag) { return tag == 0 || tag == 1 || tag == 2 || tag == 4 || tag == 7; }

template <class F>
struct RbParams {
  typename F::E half, g;  // 2^-1 and z^q, as elements (Montgomery form where the field keeps it)
  u64 e[4];               // (q-1)/2
  int s, top;             // p - 1 = 2^s q; the highest non-zero 2-bit window of e
};

template <class F>
constexpr bool rb_mersenne() {
  return F::TAG == M61::TAG || F::TAG == M127::TAG;
}

// s where the field fixes it, so that the rounds unroll away; Mont128 reads it
template <class F>
SCL_HD int rb_s(const RbParams<F>& prm) {
  if constexpr (F::TAG == Mont128::TAG) return prm.s;
  else if constexpr (F::TAG == Secp256k1Scalar::TAG) return 6;
  else return 1;
}

// cond ? a : b, limb by limb: a conditional expression over a four-limb struct selects between ADDRESSES, which keeps both
// operands in memory (scratch, or LDS where the compiler moves them)
template <class F>
SCL_HD typename F::E rb_sel(bool cond, const typename F::E& a, const typename F::E& b) {
  if constexpr (F::LIMBS == 4) {
    typename F::E r;
    for (int i = 0; i < 4; ++i) r.w[i] = cond ? a.w[i] : b.w[i];
    return r;
  } else {
    return cond ? a : b;
  }
}

// x^(2^k) * y (the Montgomery fields have no sqn_mul of their own)
template <class F>
SCL_HD typename F::E rb_sqn_mul(const typename F::Ctx& c, typename F::E x, int k, const typename F::E& y) {
  for (int i = 0; i < k; ++i) x = F::sqr(c, x);
  return F::mul(c, x, y);
}

// a^((q-1)/2)
template <class F>
SCL_HD typename F::E rb_pow_w(const typename F::Ctx& c, const RbParams<F>& prm, const typename F::E& a) {
  typedef typename F::E E;
  if constexpr (F::TAG == M61::TAG) {
    const E x2 = F::sqn_mul(c, a, 1, a);
    const E x4 = F::sqn_mul(c, x2, 2, x2);
    const E x8 = F::sqn_mul(c, x4, 4, x4);
    const E x16 = F::sqn_mul(c, x8, 8, x8);
    const E x32 = F::sqn_mul(c, x16, 16, x16);
    const E x48 = F::sqn_mul(c, x32, 16, x16);
    const E x56 = F::sqn_mul(c, x48, 8, x8);
    const E x58 = F::sqn_mul(c, x56, 2, x2);
    return F::sqn_mul(c, x58, 1, a);  // 2^59 - 1
  } else if constexpr (F::TAG == M127::TAG) {
    const E x2 = F::sqn_mul(c, a, 1, a);
    const E x4 = F::sqn_mul(c, x2, 2, x2);
    const E x8 = F::sqn_mul(c, x4, 4, x4);
    const E x16 = F::sqn_mul(c, x8, 8, x8);
    const E x32 = F::sqn_mul(c, x16, 16, x16);
    const E x64 = F::sqn_mul(c, x32, 32, x32);
    const E x96 = F::sqn_mul(c, x64, 32, x32);
    const E x112 = F::sqn_mul(c, x96, 16, x16);
    const E x120 = F::sqn_mul(c, x112, 8, x8);
    const E x124 = F::sqn_mul(c, x120, 4, x4);
    return F::sqn_mul(c, x124, 1, a);  // 2^125 - 1
  } else if constexpr (F::TAG == Secp256k1Field::TAG) {
    // (p-3)/4 = 2^254 - 2^30 - 245: 223 ones, a zero, 22 ones, then 0000 1011 -- the runs of ones as for a Mersenne prime
    const E x2 = rb_sqn_mul<F>(c, a, 1, a);
    const E x3 = rb_sqn_mul<F>(c, x2, 1, a);
    const E x6 = rb_sqn_mul<F>(c, x3, 3, x3);
    const E x9 = rb_sqn_mul<F>(c, x6, 3, x3);
    const E x11 = rb_sqn_mul<F>(c, x9, 2, x2);
    const E x22 = rb_sqn_mul<F>(c, x11, 11, x11);
    const E x44 = rb_sqn_mul<F>(c, x22, 22, x22);
    const E x88 = rb_sqn_mul<F>(c, x44, 44, x44);
    const E x176 = rb_sqn_mul<F>(c, x88, 88, x88);
    const E x220 = rb_sqn_mul<F>(c, x176, 44, x44);
    const E x223 = rb_sqn_mul<F>(c, x220, 3, x3);
    E r = rb_sqn_mul<F>(c, x223, 23, x22);
    r = rb_sqn_mul<F>(c, r, 5, a);  // 0000 1
    r = rb_sqn_mul<F>(c, r, 2, a);  // 01
    return rb_sqn_mul<F>(c, r, 1, a);
  } else {
    // fixed 2-bit windows over the run-time exponent: a, a^2, a^3 once, then two squarings and at most one product per window.
    // The exponent is the same in every lane, so the choice among the three is a scalar select: the table stays in registers
    // (a 4-bit table indexed by a run-time window does not: the compiler moves it to scratch memory or LDS).
    const E t1 = a, t2 = F::sqr(c, a), t3 = F::mul(c, t2, a);
    const unsigned first = (unsigned)(prm.e[prm.top >> 5] >> (2 * (prm.top & 31))) & 3u;
    // (first is 0 only where the exponent is: p = 2^s + 1, q = 1, w = a^0)
    E r = rb_sel<F>(first == 0, F::one(c), rb_sel<F>(first == 1, t1, rb_sel<F>(first == 2, t2, t3)));
    for (int i = prm.top - 1; i >= 0; --i) {
      r = F::sqr(c, F::sqr(c, r));
      const unsigned win = (unsigned)(prm.e[i >> 5] >> (2 * (i & 31))) & 3u;
      if (win) r = F::mul(c, r, rb_sel<F>(win == 1, t1, rb_sel<F>(win == 2, t2, t3)));
    }
    return r;
  }
}

// is the integer value of x odd
template <class F>
SCL_HD bool rb_is_odd(const typename F::Ctx& c, const typename F::E& x) {
  if constexpr (rb_mersenne<F>()) return (unsigned)x & 1u;
  else if constexpr (F::TAG == Mont128::TAG) return (unsigned)F::from_mont(c, x) & 1u;
  else return (unsigned)F::from_mont(c, x).w[0] & 1u;
}

template <class F>
struct RbRoot {
  typename F::E root, inv;  // both zero unless status is RB_OK
  int status;
};

// the root of a with the even integer value (odd: the other one), its inverse, and the status
template <class F>
SCL_HD RbRoot<F> rb_sqrt_one(const typename F::Ctx& c, const RbParams<F>& prm, const typename F::E& a, bool odd) {
  typedef typename F::E E;
  const int s = rb_s<F>(prm);
  const E one = F::one(c);
  const E w = rb_pow_w<F>(c, prm, a);
  E x = F::mul(c, a, w);
  E b = F::mul(c, x, w);
  const E b0 = b;
  E g = prm.g;
  for (int i = s - 1; i >= 1; --i) {
    E t = b;
    for (int k = 1; k < i; ++k) t = F::sqr(c, t);
    const bool ne = !F::eq(t, one);
    const E xg = F::mul(c, x, g);
    g = F::sqr(c, g);
    const E bg = F::mul(c, b, g);
    x = rb_sel<F>(ne, xg, x);
    b = rb_sel<F>(ne, bg, b);
  }
  E inv = w;
  if (s > 1) {
    E r = b0;  // b0^(2^s - 1)
    for (int i = 1; i < s; ++i) r = F::mul(c, F::sqr(c, r), b0);
    inv = F::mul(c, x, F::mul(c, F::sqr(c, w), r));
  }
  const bool ok = F::eq(F::sqr(c, x), a);
  const bool flip = rb_is_odd<F>(c, x) != odd;
  x = rb_sel<F>(flip, F::neg(c, x), x);
  inv = rb_sel<F>(flip, F::neg(c, inv), inv);
  RbRoot<F> out;
  out.status = F::is_zero(a) ? RB_ZERO : ok ? RB_OK : RB_NONRESIDUE;
  out.root = rb_sel<F>(out.status == RB_OK, x, F::zero());
  out.inv = rb_sel<F>(out.status == RB_OK, inv, F::zero());
  return out;
}

// h = 2^-1 / root(u), the column's factor of the bit finish (zero unless the status is RB_OK)
template <class F>
SCL_HD typename F::E rb_bit_factor(const typename F::Ctx& c, const RbParams<F>& prm, const typename F::E& u, int& status) {
  const RbRoot<F> r = rb_sqrt_one<F>(c, prm, u, false);
  status = r.status;
  return F::mul(c, prm.half, r.inv);
}

// b = h r + 2^-1 = (r / root(r^2) + 1) / 2: 0 or 1 when opened; zero where the column's status is set
template <class F>
SCL_HD typename F::E rb_bit_one(const typename F::Ctx& c, const RbParams<F>& prm, const typename F::E& h, int status, const typename F::E& r) {
  const typename F::E v = F::add(c, F::mul(c, h, r), prm.half);
  return rb_sel<F>(status == RB_OK, v, F::zero());
}

// ---- the constants, on the host --------------------------------------------------------------------------------------------
template <class F>
inline void rb_prime(const typename F::Ctx& c, u64 (&p)[4]) {
  p[0] = p[1] = p[2] = p[3] = 0;
  if constexpr (F::TAG == M61::TAG) {
    p[0] = M61::P;
  } else if constexpr (F::TAG == M127::TAG) {
    p[0] = (u64)M127::P();
    p[1] = (u64)(M127::P() >> 64);
  } else if constexpr (F::TAG == Mont128::TAG) {
    p[0] = (u64)c.p;
    p[1] = (u64)(c.p >> 64);
  } else {
    for (int i = 0; i < 4; ++i) p[i] = F::P(i);
  }
}

inline void rb_shr1(u64 (&v)[4]) {
  for (int i = 0; i < 4; ++i) v[i] = (v[i] >> 1) | (i < 3 ? v[i + 1] << 63 : 0);
}

// base^e, bit by bit from the top (host: the constants are made once)
template <class F>
inline typename F::E rb_pow_host(const typename F::Ctx& c, const typename F::E& base, const u64 (&e)[4]) {
  typename F::E r = F::one(c);
  for (int i = 255; i >= 0; --i) {
    r = F::sqr(c, r);
    if ((e[i >> 6] >> (i & 63)) & 1) r = F::mul(c, r, base);
  }
  return r;
}

template <class F>
inline RbParams<F> rb_make_params(const typename F::Ctx& c) {
  typedef typename F::E E;
  RbParams<F> prm;
  u64 q[4], euler[4];
  rb_prime<F>(c, q);
  q[0] &= ~(u64)1;  // p - 1
  for (int i = 0; i < 4; ++i) euler[i] = q[i];
  rb_shr1(euler);   // (p - 1) / 2
  prm.s = 0;
  while (!(q[0] & 1)) {
    rb_shr1(q);
    ++prm.s;
  }
  for (int i = 0; i < 4; ++i) prm.e[i] = q[i];
  rb_shr1(prm.e);   // (q - 1) / 2
  prm.top = 0;
  for (int i = 0; i < 128; ++i)
    if ((prm.e[i >> 5] >> (2 * (i & 31))) & 3) prm.top = i;
  const E one = F::one(c), two = F::add(c, one, one);
  prm.half = F::inv(c, two);
  E z = two;  // the smallest integer that fails Euler's criterion
  while (F::eq(rb_pow_host<F>(c, z, euler), one)) z = F::add(c, z, one);
  prm.g = rb_pow_host<F>(c, z, q);
  return prm;
}

}  // namespace sclhip
