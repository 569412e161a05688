// include/scl_hip/ss/compare.h -- the per-secret host forms of the comparison extension: ss::cmpOpen, ss::bitLtLeaves, ss::combine
// and the three finishes ss::mod2m, ss::truncExact and ss::ltz, the local steps of an exact comparison for ONE party and ONE
// value, all over include/scl_hip/detail/cmp.hpp -- the arithmetic the kernels of libscl_hip_cmp.so run, so hip::cmpFirstMask,
// hip::cmpLevelMask and hip::cmpFinish (hip/cmp.h) compute the same words.  The protocol, the ranges and the status are stated in
// include/scl_hip_cmp.h.
#ifndef SCL_HIP_SS_COMPARE_H
#define SCL_HIP_SS_COMPARE_H

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../detail/cmp.hpp"
#include "../math/ff.h"

namespace scl {
namespace ss {

/// A node of the comparison tree, one party's shares: lt = [c' < r' on the node's bits], eq = [c' = r' on them].
template <typename T>
struct CmpNode {
  T lt, eq;
};

/// What every party learns from the opened c: c mod 2^w as an element and as an integer, and the status (1: c >= 2^(B+1); the
/// value is 0 then).
template <typename T>
struct CmpOpened {
  T cmod;
  std::uint64_t limbs[4] = {0, 0, 0, 0};
  int status = 0;
  bool bit(std::size_t i) const { return (limbs[i >> 6] >> (i & 63)) & 1; }
};

namespace cmp_detail {
template <typename FIELD>
void checkRange(const typename FIELD::Impl::Ctx& ctx, std::size_t w, std::size_t B, const char* who) {
  static_assert(sclhip::fx_has_trunc(FIELD::Impl::TAG), "a comparison needs a prime field: not GF(2^128)");
  if (w == 0 || w >= B || B > (std::size_t)sclhip::fx_prime_bits<typename FIELD::Impl>(ctx) - 2) throw std::invalid_argument(who);
}
}  // namespace cmp_detail

/// The column's part of the first level: 1 <= w < B <= |p| - 2.
template <typename FIELD>
CmpOpened<math::FF<FIELD>> cmpOpen(const math::FF<FIELD>& opened, std::size_t w, std::size_t B) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  cmp_detail::checkRange<FIELD>(ctx, w, B, "cmpOpen: 1 <= w < B <= |p| - 2 does not hold");
  CmpOpened<math::FF<FIELD>> out;
  sclhip::u64 limbs[F::LIMBS];
  out.cmod.value() = sclhip::cmp_open_col<F>(ctx, sclhip::fx_make_finish<F>(ctx, (int)w, (int)B), opened.value(), limbs, out.status);
  for (std::size_t i = 0; i < (std::size_t)F::LIMBS; ++i) out.limbs[i] = limbs[i];
  return out;
}

/// One party's leaves from its shares of the bits b_0 .. b_(w-1): lt_i = (1 - c_i) b_i, eq_i = c_i ? b_i : 1 - b_i.
template <typename FIELD>
std::vector<CmpNode<math::FF<FIELD>>> bitLtLeaves(const CmpOpened<math::FF<FIELD>>& c, const std::vector<math::FF<FIELD>>& bits) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  if (bits.empty() || bits.size() > 256) throw std::invalid_argument("bitLtLeaves: w must be in 1 .. 256");
  std::vector<CmpNode<math::FF<FIELD>>> out(bits.size());
  for (std::size_t i = 0; i < bits.size(); ++i)
    sclhip::cmp_leaf<F>(ctx, sclhip::cmp_bit_mask(c.limbs[i >> 6], (int)i), bits[i].value(), out[i].lt.value(), out[i].eq.value());
  return out;
}

/// The node a node without a partner combines with: lt = 0, eq = 1.
template <typename T>
CmpNode<T> cmpIdentity() {
  return CmpNode<T>{T{}, T(1)};
}

/// One party's masked combination [d]_2t of two adjacent nodes: lt = lt_hi + eq_hi lt_lo + r2.lt, eq = eq_hi eq_lo + r2.eq, r2
/// its shares of two degree-2t sharings.  Opened and reduced by the matching degree-t shares it is the node of both runs of bits.
template <typename FIELD>
CmpNode<math::FF<FIELD>> combine(const CmpNode<math::FF<FIELD>>& hi, const CmpNode<math::FF<FIELD>>& lo, const CmpNode<math::FF<FIELD>>& r2) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  CmpNode<math::FF<FIELD>> out;
  out.lt.value() = sclhip::cmp_combine_lt<F>(ctx, hi.lt.value(), hi.eq.value(), lo.lt.value(), r2.lt.value());
  out.eq.value() = sclhip::cmp_combine_eq<F>(ctx, hi.eq.value(), lo.eq.value(), r2.eq.value());
  return out;
}

namespace cmp_detail {
template <typename FIELD>
math::FF<FIELD> finish(const CmpOpened<math::FF<FIELD>>& c, const math::FF<FIELD>& lt, const math::FF<FIELD>& rlow, const math::FF<FIELD>& x, std::size_t w,
                       int what, const char* who) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  if (w == 0 || w + 2 >= (std::size_t)sclhip::fx_prime_bits<F>(ctx)) throw std::invalid_argument(who);
  math::FF<FIELD> out;
  out.value() = sclhip::cmp_finish_one<F>(ctx, sclhip::cmp_make_finish<F>(ctx, (int)w, what), c.cmod.value(), c.status, lt.value(), rlow.value(), x.value());
  return out;
}
}  // namespace cmp_detail

/// One party's share of x mod 2^w: c' - r' + 2^w lt; zero where the status of c is set.
template <typename FIELD>
math::FF<FIELD> mod2m(const CmpOpened<math::FF<FIELD>>& c, const math::FF<FIELD>& lt, const math::FF<FIELD>& rlow, std::size_t w) {
  return cmp_detail::finish<FIELD>(c, lt, rlow, math::FF<FIELD>{}, w, sclhip::CMP_MOD, "mod2m: 1 <= w <= |p| - 3 does not hold");
}

/// One party's share of floor(x / 2^w), exactly: (x - (c' - r' + 2^w lt)) 2^-w.
template <typename FIELD>
math::FF<FIELD> truncExact(const CmpOpened<math::FF<FIELD>>& c, const math::FF<FIELD>& lt, const math::FF<FIELD>& rlow, const math::FF<FIELD>& x, std::size_t w) {
  return cmp_detail::finish<FIELD>(c, lt, rlow, x, w, sclhip::CMP_TRUNC, "truncExact: 1 <= w <= |p| - 3 does not hold");
}

/// One party's share of [x < 0] for a signed k-bit x masked with w = k - 1: the exact truncation, negated.
template <typename FIELD>
math::FF<FIELD> ltz(const CmpOpened<math::FF<FIELD>>& c, const math::FF<FIELD>& lt, const math::FF<FIELD>& rlow, const math::FF<FIELD>& x, std::size_t w) {
  return cmp_detail::finish<FIELD>(c, lt, rlow, x, w, sclhip::CMP_LTZ, "ltz: 1 <= w <= |p| - 3 does not hold");
}

}  // namespace ss
}  // namespace scl

#endif
