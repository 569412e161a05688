// csrc/unit_device.hpp -- what the streaming kernels of the extension units (beaver_, hm_, ip_, rb_, fx_unit.hip) share, on top
// of the pack type of kernels.hpp: 256-lane blocks, one pack per lane behind a capped grid, 16-byte non-temporal accesses -- two
// one-limb elements, one 16-byte element or half a 32-byte element each.  The pack width of the one-limb fields is chosen on the
// host per call (unit_host.hpp: two_per_lane, PACK_LAUNCH -- 16-byte aligned bases and even strides: two elements per lane,
// else one); with two per lane an odd N leaves one element, which the lane after the last pair takes on its own, so a call stays
// one launch.
//
//   for_each_pack   the grid-stride loop over the packs of a row and its odd tail
//   OpenTable       the recombination vector of an opening inside a finish kernel, a kernel argument, and
//   open_at         the opening itself: sum_j lambda_j sh[j] on the field's lazy accumulator
// Device code.  A unit includes it after kernels.hpp; unit_host.hpp holds the host side of the same conventions.
#pragma once

#include <type_traits>

#include "kernels.hpp"

namespace sclhip {

// lanes a row of N elements takes at VEC elements per lane: the packs, and with pairs the odd element after the last one
template <int VEC>
__device__ __forceinline__ size_t pack_items(size_t N) {
  return N / VEC + (VEC == 2 ? (N & 1) : 0);
}

// at(integral_constant<int, W>, i) for every pack of a row of N elements: W = VEC at i = q * VEC, and W = 1 at i = N - 1 for the
// odd element after the last pair.  Grid-stride along blockIdx.x; the row (blockIdx.y) is the kernel's own business.
template <int VEC, class At>
__device__ __forceinline__ void for_each_pack(size_t N, At&& at) {
  const size_t npacks = N / VEC, items = pack_items<VEC>(N);
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < items; q += (size_t)gridDim.x * BLOCK) {
    if (VEC == 1 || q < npacks) at(std::integral_constant<int, VEC>{}, q * VEC);
    else at(std::integral_constant<int, 1>{}, N - 1);
  }
}

// ---- the open inside a finish kernel ---------------------------------------------------------------------------------------
constexpr int OPEN_M_MAX = 64;  // shares an opening takes: lambda travels with the launch
static_assert(OPEN_M_MAX <= (int)M61::ACC_TERMS, "the open of a finish kernel never folds");

template <class F>
struct OpenTable {  // kernel-argument table (2 KiB for the 32-byte fields); make_open_table of unit_host.hpp fills it
  typename F::E v[OPEN_M_MAX];
};

// opened[v] = sum_j lam[j] sh[j][i + v], j < m.  `lam` is whatever yields lambda_j at a wave-uniform j: the table where it
// lies among the kernel arguments (OpenTable::v), or a copy of it in LDS.
template <class F, int W, class Lam>
__device__ __forceinline__ void open_at(const typename F::Ctx& ctx, const u64* sh, size_t stride, const Lam& lam, int m, size_t i,
                                        typename F::E (&opened)[W]) {
  typename F::Acc acc[W];
#pragma unroll
  for (int v = 0; v < W; ++v) acc[v] = F::acc_zero();
#pragma unroll 1
  for (int j = 0; j < m; ++j) {  // m <= 64 <= every field's F::ACC_TERMS: no fold on the way
    const Pack<F, W> sv = load_pack<F, W, true>(sh + ((size_t)j * stride + i) * F::LIMBS);
    const typename F::E l = lam[j];
#pragma unroll
    for (int v = 0; v < W; ++v) F::mac(ctx, acc[v], l, sv.v[v]);
  }
#pragma unroll
  for (int v = 0; v < W; ++v) opened[v] = F::acc_fold(ctx, acc[v]);
}

}  // namespace sclhip
