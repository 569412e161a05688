// csrc/beaver_unit.hip -- Beaver multiplication of shared vectors: the fused mask and finish kernels and the C ABI of
// libscl_hip_mpc.so (include/scl_hip_mpc.h), an extension library beside the engine.  One translation unit, all fields.
//
// Replaces the arithmetic around the open step of the reference's BeaverMul (test/scl/protocol/beaver.h:40-41 and 57-61) over
// batches of secrets and parties.  The per-element functions are include/scl_hip/detail/beaver.hpp; the conventions are those
// of the streaming kernels of every extension unit, csrc/unit_device.hpp: 256-lane blocks, one pack (kernels.hpp) per lane, a
// grid-stride loop behind a capped grid, non-temporal 16-byte accesses, the pack width of the one-limb fields -- the rings
// Z2k<K <= 64> among them -- chosen on the host per call, the odd last element taken by the lane after the last pair.  No LDS,
// no scratch; the engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_mpc.h"
#include "../../include/scl_hip/detail/beaver.hpp"
#include "kernels.hpp"
#include "unit_device.hpp"

namespace sclhip {
namespace {

// dst[i .. i + W) = x - a
template <class F, int W>
__device__ __forceinline__ void mask_at(const typename F::Ctx& ctx, u64* dst, const u64* x, const u64* a, size_t i) {
  const Pack<F, W> xv = load_pack<F, W, true>(x + i * F::LIMBS), av = load_pack<F, W, true>(a + i * F::LIMBS);
  Pack<F, W> r;
#pragma unroll
  for (int v = 0; v < W; ++v) r.v[v] = beaver_mask_one<F>(ctx, xv.v[v], av.v[v]);
  store_pack<F, W, true>(dst + i * F::LIMBS, r);
}

// Both subtractions of the mask in one launch: row blockIdx.y of e = x - a and of d = y - b (d lies `d_off` words past e).
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_beaver_mask(typename F::Ctx ctx, u64* de, size_t de_stride, size_t d_off, const u64* x,
                                                       const u64* y, const u64* a, const u64* b, size_t op_stride, size_t n) {
  const size_t in_row = (size_t)blockIdx.y * op_stride * F::LIMBS;
  u64* e_out = de + (size_t)blockIdx.y * de_stride * F::LIMBS;
  u64* d_out = e_out + d_off;
  x += in_row;
  y += in_row;
  a += in_row;
  b += in_row;
  for_each_pack<VEC>(n, [&](auto w, size_t i) {
    mask_at<F, w>(ctx, e_out, x, a, i);
    mask_at<F, w>(ctx, d_out, y, b, i);
  });
}

// z[r][i .. i + W) for every row r: e and d are loaded once, each row's a, b, c are read and its z written where they lie.
// A lane reads its elements of a row before it writes them, so z may be a, b or c.
template <class F, int W>
__device__ __forceinline__ void finish_at(const typename F::Ctx& ctx, u64* z, size_t z_stride, const u64* e, const u64* d, const u64* a,
                                          const u64* b, const u64* c, size_t op_stride, size_t rows, size_t ed_rows, size_t i) {
  const Pack<F, W> ev = load_pack<F, W, true>(e + i * F::LIMBS), dv = load_pack<F, W, true>(d + i * F::LIMBS);
#pragma unroll 1
  for (size_t r = 0; r < rows; ++r) {
    const size_t off = (r * op_stride + i) * F::LIMBS;
    const Pack<F, W> av = load_pack<F, W, true>(a + off), bv = load_pack<F, W, true>(b + off), cv = load_pack<F, W, true>(c + off);
    const bool add_ed = r < ed_rows;  // the same in every lane
    Pack<F, W> zv;
#pragma unroll
    for (int v = 0; v < W; ++v) zv.v[v] = beaver_finish_one<F>(ctx, ev.v[v], dv.v[v], av.v[v], bv.v[v], cv.v[v], add_ed);
    store_pack<F, W, true>(z + (r * z_stride + i) * F::LIMBS, zv);
  }
}

// One secret (VEC = 2: two) per lane across all rows: (4 rows + 2) N elements of traffic.
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_beaver_finish(typename F::Ctx ctx, u64* z, size_t z_stride, const u64* e, const u64* d,
                                                         const u64* a, const u64* b, const u64* c, size_t op_stride, size_t rows,
                                                         size_t ed_rows, size_t n) {
  for_each_pack<VEC>(n, [&](auto w, size_t i) { finish_at<F, w>(ctx, z, z_stride, e, d, a, b, c, op_stride, rows, ed_rows, i); });
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#include "unit_host.hpp"

namespace {
bool known_tag(int field) { return is_field(field) || is_ring(field); }
}  // namespace

extern "C" {

int scl_mpc_abi_version(void) { return SCL_MPC_ABI_VERSION; }
const char* scl_mpc_last_error(void) { return g_err.c_str(); }

int scl_mpc_beaver_mask(int field, uint64_t* de, size_t de_stride, const uint64_t* x, const uint64_t* y, const uint64_t* a,
                        const uint64_t* b, size_t op_stride, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  if (!known_tag(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  if (!de || !x || !y || !a || !b) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;  // (this library asks after its tag and NULL checks)
  return with_ring_or_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = check_align(nullptr, F::LIMBS, {de, x, y, a, b})) return rc;
    if (de_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "de_stride < N");
    if (op_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "op_stride < N");
    // the output has 2 rows rows of de_stride elements, an operand rows rows of op_stride: neither extent may wrap
    if (rows > ((size_t)1 << 61) / (de_stride > op_stride ? de_stride : op_stride) / F::LIMBS)
      return fail(SCL_ERR_BAD_ARG, "beaver_mask: rows * stride overflows");
    const Span out = span_of(de, 2 * rows, de_stride, N, F::LIMBS);
    for (const uint64_t* p : {x, y, a, b})
      if (overlap(out, span_of(p, rows, op_stride, N, F::LIMBS))) return fail(SCL_ERR_BAD_ARG, "beaver_mask: de overlaps an operand");
    if (const int rc = need_device()) return rc;
    const size_t d_off = rows * de_stride * F::LIMBS;
    // (an odd rows * de_stride puts d an odd number of words past e: its rows are then 8 bytes off the 16-byte grid)
    const bool two = two_per_lane(F::LIMBS, {de, x, y, a, b}, {rows > 1 ? de_stride : 0, rows > 1 ? op_stride : 0, rows * de_stride});
    for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
      const size_t r = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
      u64* out0 = de + r0 * de_stride * F::LIMBS;
      const size_t in0 = r0 * op_stride * F::LIMBS;
      PACK_LAUNCH((k_beaver_mask, F), two, dim3(grid_for_packs(two, N), (unsigned)r), S(stream), ctx, out0, de_stride, d_off, x + in0, y + in0,
                  a + in0, b + in0, op_stride, N);
    }
    return SCL_OK;
  });
}

int scl_mpc_beaver_finish(int field, uint64_t* z, size_t z_stride, const uint64_t* e, const uint64_t* d, const uint64_t* a,
                          const uint64_t* b, const uint64_t* c, size_t op_stride, size_t rows, size_t ed_rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  if (!known_tag(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  if (!z || !e || !d || !a || !b || !c) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;  // (this library asks after its tag and NULL checks)
  return with_ring_or_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = check_align(nullptr, F::LIMBS, {z, e, d, a, b, c})) return rc;
    if (z_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "z_stride < N");
    if (op_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "op_stride < N");
    if (ed_rows > rows) return fail(SCL_ERR_BAD_ARG, "beaver_finish: ed_rows > rows");
    if (rows > ((size_t)1 << 62) / (z_stride > op_stride ? z_stride : op_stride) / F::LIMBS)
      return fail(SCL_ERR_BAD_ARG, "beaver_finish: rows * stride overflows");
    const Span out = span_of(z, rows, z_stride, N, F::LIMBS);
    for (const uint64_t* p : {a, b, c}) {
      if (p == z && z_stride == op_stride) continue;  // in place: each lane reads its elements of a row before it writes them
      if (overlap(out, span_of(p, rows, op_stride, N, F::LIMBS)))
        return fail(SCL_ERR_BAD_ARG, "beaver_finish: z overlaps an operand (only z == a, b or c with z_stride == op_stride is allowed)");
    }
    if (overlap(out, span_of(e, 1, N, N, F::LIMBS)) || overlap(out, span_of(d, 1, N, N, F::LIMBS)))
      return fail(SCL_ERR_BAD_ARG, "beaver_finish: z overlaps e or d");
    if (const int rc = need_device()) return rc;
    const bool two = two_per_lane(F::LIMBS, {z, e, d, a, b, c}, {rows > 1 ? z_stride : 0, rows > 1 ? op_stride : 0});
    PACK_LAUNCH((k_beaver_finish, F), two, dim3(grid_for_packs(two, N)), S(stream), ctx, z, z_stride, e, d, a, b, c, op_stride, rows, ed_rows, N);
    return SCL_OK;
  });
}

}  // extern "C"
