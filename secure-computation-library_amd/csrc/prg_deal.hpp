// csrc/prg_deal.hpp -- a dealer's draws in the reference's PRG order, for the kernels that deal from one util::PRG stream
// (triples_unit.hip: randomTriple2; hm_unit.hip: the double sharings): a lane addresses the AES blocks of its own secret by
// counter and draws, one after another, single elements (FF::random) and the coefficients of Shamir polynomials
// (Vector::random(d + 1), element 0 discarded).  On the four-table AES of kernels.hpp.  The host side -- the limits on n and the
// degree, the counter range -- is the AES part of unit_host.hpp.
//
// (vf_unit.hip's CoeffPrg draws whole vectors in scl_hip_vector_random's order, pack q at block q: another order, kept there.)
#pragma once

#include "kernels.hpp"

namespace sclhip {

template <class F>
constexpr int bpe() {  // FF::random burns ceil(byteSize/16) blocks (ff.h:72-76)
  return F::LIMBS >= 2 ? F::LIMBS / 2 : 1;
}

// one FF::random at block c0: a one-limb element is the first 8 bytes of its block
template <class F>
__device__ __forceinline__ typename F::E draw_elem(const typename F::Ctx& ctx, const Aes4& aes, const AesKey& key, u64 c0) {
  constexpr int BPE = bpe<F>();
  u64 lo[BPE], hi[BPE];
#pragma unroll
  for (int b = 0; b < BPE; ++b) aes.block(key, c0 + b, lo[b], hi[b]);
  if constexpr (F::LIMBS == 1) return F::from_le_word(ctx, lo[0]);
  else return elem_from_blocks<F>(ctx, lo, hi);
}

// Blocks of one Vector::random(d+1) draw
template <class F>
__host__ __device__ constexpr u64 poly_blocks(u64 d) {
  return ((d + 1) * (u64)(8 * F::LIMBS) + 15) / 16;
}

// coefficients 1..D of the polynomial whose Vector::random(D+1) draw starts at block p0 (element 0 is discarded, shamir.h:57):
// one-limb fields hold elements 2j and 2j+1 in block j, wider ones element k in blocks k*BPE ..
template <class F, int D>
__device__ __forceinline__ void draw_poly(const typename F::Ctx& ctx, const Aes4& aes, const AesKey& key, u64 p0,  // (by value)
                                          typename F::E (&c)[D + 1]) {
  if constexpr (F::LIMBS == 1) {
#pragma unroll
    for (int j = 0; 2 * j <= D; ++j) {
      u64 lo, hi;
      aes.block(key, p0 + j, lo, hi);
      if (j > 0) c[2 * j] = F::from_le_word(ctx, lo);
      if (2 * j + 1 <= D) c[2 * j + 1] = F::from_le_word(ctx, hi);
    }
  } else {
    constexpr int BPE = bpe<F>();
#pragma unroll
    for (int k = 1; k <= D; ++k) {
      u64 lo[BPE], hi[BPE];
#pragma unroll
      for (int b = 0; b < BPE; ++b) aes.block(key, p0 + (u64)k * BPE + b, lo[b], hi[b]);
      c[k] = elem_from_blocks<F>(ctx, lo, hi);
      // one coefficient's blocks at a time: left alone the compiler runs all D draws abreast (some ten
      // registers each) and runs out of the 128 registers a 1024-lane workgroup has.  The empty statement makes the next
      // counter wait for this result.
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+v"(p0) : "v"((u32)lo[0]));
#endif
    }
  }
}

// the polynomial c at the nodes 1..n into rows of `out`: F::muladd_small_lazy steps, one F::canon at the end
template <class F, int D>
__device__ __forceinline__ void eval_rows(const typename F::Ctx& ctx, const typename F::E (&c)[D + 1], u64* out, size_t stride, int n) {
#pragma unroll 1
  for (int i = 0; i < n; ++i) {
    const u32 x = (u32)(i + 1);
    typename F::E y = c[D];
#pragma unroll
    for (int k = D; k >= 1; --k) y = F::muladd_small_lazy(ctx, y, x, c[k - 1]);  // congruent, not yet canonical
    Pack<F, 1> r;
    r.v[0] = F::canon(y);
    store_pack<F, 1, true>(out + (size_t)i * stride * F::LIMBS, r);
  }
}

// (The first pass of a two-pass deal -- k_triple_coeff_rows, k_double_coeff_rows: the same draws at a run-time degree, stored row
// by row -- stays spelled out in its kernels: as a function of this file the loop nest compiled to other code, a register and
// a few instructions more or fewer per field, and the kernels are to stay as they were.)

}  // namespace sclhip
