// include/scl_hip/ss/trunc.h -- the per-secret host forms of the fixed-point extension: ss::composeBits, ss::truncMask and
// ss::truncFinish, the two local steps of a probabilistic truncation (Catrina, de Hoogh) for ONE party and ONE value, all over
// include/scl_hip/detail/fx.hpp -- the arithmetic the kernels of libscl_hip_fx.so run, so hip::composeBits, hip::truncMask and
// hip::truncFinish (hip/fx.h) compute the same words.  The protocol, the ranges and the status are stated in include/scl_hip_fx.h.
#ifndef SCL_HIP_SS_TRUNC_H
#define SCL_HIP_SS_TRUNC_H

#include <cstddef>
#include <stdexcept>
#include <vector>

#include "../detail/fx.hpp"
#include "../math/ff.h"

namespace scl {
namespace ss {

namespace fx_detail {
template <typename FIELD>
std::size_t maxBits(const typename FIELD::Impl::Ctx& ctx) {
  static_assert(sclhip::fx_has_trunc(FIELD::Impl::TAG), "truncation needs a prime field: not GF(2^128)");
  return (std::size_t)sclhip::fx_prime_bits<typename FIELD::Impl>(ctx) - 2;
}
}  // namespace fx_detail

/// One party's share of sum_i 2^i b_i from its shares of the bits b_0 .. b_(B-1); 1 <= B <= |p| - 2.
template <typename FIELD>
math::FF<FIELD> composeBits(const std::vector<math::FF<FIELD>>& bits) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  if (bits.empty() || bits.size() > fx_detail::maxBits<FIELD>(ctx)) throw std::invalid_argument("composeBits: B must be in 1 .. |p| - 2");
  typename F::E acc = F::zero();
  for (std::size_t i = bits.size(); i-- > 0;) acc = sclhip::fx_step<F>(ctx, acc, bits[i].value());
  math::FF<FIELD> out;
  out.value() = sclhip::fx_canon<F>(acc);
  return out;
}

template <typename T>
struct TruncMasked {
  T c;     ///< the share of x + 2^(k-1) + r, to be opened
  T rlow;  ///< the share of r', the lowest `shift` bits of r
};

/// One party's mask of its share x of a signed k-bit value under its shares of B >= k random bits: 1 <= shift < k <= B <= |p| - 2.
template <typename FIELD>
TruncMasked<math::FF<FIELD>> truncMask(const math::FF<FIELD>& x, const std::vector<math::FF<FIELD>>& bits, std::size_t k, std::size_t shift) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  if (shift == 0 || shift >= k || k > bits.size() || bits.size() > fx_detail::maxBits<FIELD>(ctx))
    throw std::invalid_argument("truncMask: 1 <= shift < k <= B <= |p| - 2 does not hold");
  typename F::E acc = F::zero(), low = F::zero();
  for (std::size_t i = bits.size(); i-- > 0;) {
    acc = sclhip::fx_step<F>(ctx, acc, bits[i].value());
    if (i < shift) low = sclhip::fx_step<F>(ctx, low, bits[i].value());
  }
  TruncMasked<math::FF<FIELD>> out;
  out.c.value() = sclhip::fx_mask_one<F>(ctx, sclhip::fx_make_mask<F>(ctx, (int)k), x.value(), sclhip::fx_canon<F>(acc));
  out.rlow.value() = sclhip::fx_canon<F>(low);
  return out;
}

/// One party's share of the truncated value from the opened c, its share x and its share rlow of r':
/// (x + rlow - (c mod 2^shift)) * 2^-shift.  status (optional): 0 ok, 1 c >= 2^(B+1) -- the share is zero then, as on the device.
template <typename FIELD>
math::FF<FIELD> truncFinish(const math::FF<FIELD>& opened, const math::FF<FIELD>& x, const math::FF<FIELD>& rlow, std::size_t shift, std::size_t B,
                            int* status = nullptr) {
  using F = typename FIELD::Impl;
  const auto ctx = math::ff::detail::context<FIELD>();
  if (shift == 0 || shift >= B || B > fx_detail::maxBits<FIELD>(ctx)) throw std::invalid_argument("truncFinish: 1 <= shift < B <= |p| - 2 does not hold");
  const auto prm = sclhip::fx_make_finish<F>(ctx, (int)shift, (int)B);
  int st = 0;
  const auto cp = sclhip::fx_finish_col<F>(ctx, prm, opened.value(), st);
  if (status) *status = st;
  math::FF<FIELD> out;
  out.value() = sclhip::fx_finish_one<F>(ctx, prm, cp, st, x.value(), rlow.value());
  return out;
}

}  // namespace ss
}  // namespace scl

#endif
