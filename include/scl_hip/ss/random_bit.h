// include/scl_hip/ss/random_bit.h -- the per-element host forms of the random-bit extension: math::sqrt over a prime field and
// the last step of a random shared bit, ss::randomBitFinish, both over include/scl_hip/detail/rb.hpp -- the arithmetic the
// kernels of libscl_hip_rb.so run, so hip::sqrt and hip::bitsFinish (hip/rb.h) compute the same words.  The protocol and the
// canonical-root rule are stated in include/scl_hip_rb.h.
#ifndef SCL_HIP_SS_RANDOM_BIT_H
#define SCL_HIP_SS_RANDOM_BIT_H

#include <stdexcept>

#include "../detail/rb.hpp"
#include "../math/ff.h"

namespace scl {
namespace math {

namespace rb_detail {
/// the field's constants: made once per thread, and again when the thread's Mont128 modulus has changed
template <typename FIELD>
const sclhip::RbParams<typename FIELD::Impl>& params(const typename FIELD::Impl::Ctx& ctx) {
  using F = typename FIELD::Impl;
  static_assert(sclhip::rb_has_roots(F::TAG), "square roots need a prime field: not GF(2^128)");
  static thread_local bool made = false;
  static thread_local sclhip::RbParams<F> cached;
  if constexpr (FIELD::TAG == SCL_MONT128) {
    static thread_local __uint128_t prime = 0;
    if (prime != ctx.p) made = false;
    prime = ctx.p;
  }
  if (!made) {
    cached = sclhip::rb_make_params<F>(ctx);
    made = true;
  }
  return cached;
}
}  // namespace rb_detail

/// The square root of a whose integer value -- the one FF::write serialises -- is even (odd: the other root).  sqrt(0) = 0.
/// Throws std::logic_error where a is not a square.
template <typename FIELD>
FF<FIELD> sqrt(const FF<FIELD>& a, bool odd = false) {
  using F = typename FIELD::Impl;
  const auto ctx = ff::detail::context<FIELD>();
  const auto r = sclhip::rb_sqrt_one<F>(ctx, rb_detail::params<FIELD>(ctx), a.value(), odd);
  if (r.status == sclhip::RB_NONRESIDUE) throw std::logic_error("not a square modulo prime");
  FF<FIELD> out;
  out.value() = r.root;
  return out;
}

}  // namespace math

namespace ss {

/// One party's share of the bit (r / sqrt(u) + 1) / 2 from the opened u = r^2 and its share of r: 2^-1 / root(u) * share + 2^-1
/// with the even root.  status (optional): 0 ok, 1 u was zero, 2 u is not a square -- the share is zero then, as on the device.
template <typename FIELD>
math::FF<FIELD> randomBitFinish(const math::FF<FIELD>& u, const math::FF<FIELD>& share, int* status = nullptr) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  const auto& prm = math::rb_detail::params<FIELD>(ctx);
  int st = 0;
  const auto h = sclhip::rb_bit_factor<F>(ctx, prm, u.value(), st);
  if (status) *status = st;
  math::FF<FIELD> out;
  out.value() = sclhip::rb_bit_one<F>(ctx, prm, h, st, share.value());
  return out;
}

}  // namespace ss
}  // namespace scl

#endif
