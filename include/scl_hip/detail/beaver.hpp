// include/scl_hip/detail/beaver.hpp -- the per-element arithmetic of Beaver multiplication, once, for host and device.
//
// The reference's only in-tree protocol (test/scl/protocol/beaver.h:31-70) multiplies two shared values with a triple
// ([a], [b], [c] = [a b]):
//   mask     [e] = [x] - [a],  [d] = [y] - [b]                               beaver.h:40-41
//   finish   [z] = e [b] + d [a] + [c]  (+ e d, by the parties that add constants)   beaver.h:57-61
// with e and d opened in between.  The mask is the field's sub.  The finish is two products and ONE reduction on the field's
// lazy accumulator (field.hpp: Acc, mac, acc_add, acc_fold): because e b + d a + e d = e (b + d) + d a, the constant costs
// one reduced addition, not a third product.  b + d is the field's reduced add, so it is canonical before it enters mac; c
// goes in through acc_add.  Every field and ring of field.hpp has acc_add, so none adds c after the fold.  Every residue has
// one canonical representative, so the result is bit-identical to the same value built one reduced operation at a time
// (tests/cxx/beaver_host_check.cc).  Rings wrap at their word and are returned masked, as everywhere else.
#pragma once

#include "field.hpp"

namespace sclhip {

template <class F>
SCL_HD typename F::E beaver_mask_one(const typename F::Ctx& ctx, const typename F::E& x, const typename F::E& a) {
  return F::sub(ctx, x, a);
}

#if defined(__HIP_DEVICE_COMPILE__)
// GF(2^128) on the device: e y + d a, both products in ONE pass over the nibbles.  Gf128::mul (field.hpp) walks the 32
// nibbles of its second operand from the top, multiplying the running value by x^4 and adding the multiples x^j a its bits
// select; two products share that walk -- one multiplication by x^4 per nibble position instead of two, which is the lazy
// accumulation of this field: the sum is reduced as it goes, once.  A bit selects with a sign-extended one-bit extract and
// r ^= m & t in one three-input operation per word (truth table 0x78 over (r, t, m)): ~1.7 k vector instructions for the
// two products (counted in docs/kernels/beaver.md), where two calls of Gf128::mul spend ~3.8 k (kernels.hpp, above
// k_ew_gf128_mul).  No table is indexed, so nothing leaves the registers.
__device__ __forceinline__ u128 gf128_two_products(u128 e, u128 y, u128 d, u128 a) {
  u32 te[4][4], td[4][4];  // word w of x^j e and of x^j d
  u128 me = e, md = d;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      te[j][w] = (u32)(me >> (32 * w));
      td[j][w] = (u32)(md >> (32 * w));
    }
    me = Gf128::mulx(me);
    md = Gf128::mulx(md);
  }
  const u32 yw[4] = {(u32)y, (u32)(y >> 32), (u32)(y >> 64), (u32)(y >> 96)};
  const u32 aw[4] = {(u32)a, (u32)(a >> 32), (u32)(a >> 64), (u32)(a >> 96)};
  u32 r0 = 0, r1 = 0, r2 = 0, r3 = 0;
#pragma unroll
  for (int w = 3; w >= 0; --w) {
#pragma unroll
    for (int k = 7; k >= 0; --k) {
      const u32 t = r3 >> 28;  // the four bits leaving the top come back as t (x^7 + x^2 + x + 1)
      r3 = __builtin_amdgcn_alignbit(r3, r2, 28);
      r2 = __builtin_amdgcn_alignbit(r2, r1, 28);
      r1 = __builtin_amdgcn_alignbit(r1, r0, 28);
      r0 = (r0 << 4) ^ t ^ (t << 1) ^ (t << 2) ^ (t << 7);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sh = 31 - (4 * k + j);
        const u32 my = (u32)((int)(yw[w] << sh) >> 31), ma = (u32)((int)(aw[w] << sh) >> 31);
        r0 = __builtin_amdgcn_bitop3_b32(r0, te[j][0], my, 0x78);
        r1 = __builtin_amdgcn_bitop3_b32(r1, te[j][1], my, 0x78);
        r2 = __builtin_amdgcn_bitop3_b32(r2, te[j][2], my, 0x78);
        r3 = __builtin_amdgcn_bitop3_b32(r3, te[j][3], my, 0x78);
        r0 = __builtin_amdgcn_bitop3_b32(r0, td[j][0], ma, 0x78);
        r1 = __builtin_amdgcn_bitop3_b32(r1, td[j][1], ma, 0x78);
        r2 = __builtin_amdgcn_bitop3_b32(r2, td[j][2], ma, 0x78);
        r3 = __builtin_amdgcn_bitop3_b32(r3, td[j][3], ma, 0x78);
      }
    }
  }
  return (u128)r0 | ((u128)r1 << 32) | ((u128)r2 << 64) | ((u128)r3 << 96);
}
#endif

// e b + d a + c (+ e d), canonical
template <class F>
SCL_HD typename F::E beaver_finish_one(const typename F::Ctx& ctx, const typename F::E& e, const typename F::E& d,
                                       const typename F::E& a, const typename F::E& b, const typename F::E& c, bool add_ed) {
  const typename F::E y = add_ed ? F::add(ctx, b, d) : b;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (F::TAG == Gf128::TAG) return gf128_two_products(e, y, d, a) ^ c;
#endif
  typename F::Acc acc = F::acc_zero();
  F::mac(ctx, acc, e, y);
  F::mac(ctx, acc, d, a);
  F::acc_add(ctx, acc, c);
  return F::acc_fold(ctx, acc);
}

}  // namespace sclhip
