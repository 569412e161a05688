// csrc/beaver_unit.hip -- Beaver multiplication of shared vectors: the fused mask and finish kernels and the C ABI of
// libscl_hip_mpc.so (include/scl_hip_mpc.h), an extension library beside the engine.  One translation unit, all fields.
//
// Replaces the arithmetic around the open step of the reference's BeaverMul (test/scl/protocol/beaver.h:40-41 and 57-61) over
// batches of secrets and parties.  The per-element functions are include/scl_hip/detail/beaver.hpp; the conventions are those of
// the element-wise kernels of kernels.hpp: 256-lane blocks, one pack per lane, a grid-stride loop behind a capped grid,
// streaming (non-temporal) 16-byte accesses -- two one-limb elements, one 16-byte element or half a 32-byte element each.  The
// pack width of the one-limb fields is chosen on the host per call (16-byte aligned bases and even strides: two elements per
// lane, else one); with two per lane an odd N leaves one element, which the lane after the last pack takes on its own, so a
// call stays one launch.  No LDS, no scratch; the engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_mpc.h"
#include "../../include/scl_hip/detail/beaver.hpp"

namespace sclhip {
namespace {

constexpr int BLOCK = 256;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// W consecutive elements at p (W = 2: one-limb fields only, p 16-byte aligned)
template <class F, int W>
struct Elems {
  typename F::E v[W];
};

template <class F, int W>
__device__ __forceinline__ Elems<F, W> load_elems(const u64* p) {
  Elems<F, W> r;
  if constexpr (F::LIMBS == 1 && W == 2) {
    const u64x2 w = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p));
    r.v[0] = w.x;
    r.v[1] = w.y;
  } else if constexpr (F::LIMBS == 1) {
    r.v[0] = __builtin_nontemporal_load(p);
  } else if constexpr (F::LIMBS == 2) {
    static_assert(W == 1, "16-byte elements: one per lane");
    const u64x2 w = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p));
    r.v[0] = ((u128)w.y << 64) | w.x;
  } else {
    static_assert(W == 1 && F::LIMBS == 4, "32-byte elements: one per lane");
    const u64x2 w0 = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p));
    const u64x2 w1 = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(p) + 1);
    r.v[0].w[0] = w0.x;
    r.v[0].w[1] = w0.y;
    r.v[0].w[2] = w1.x;
    r.v[0].w[3] = w1.y;
  }
  return r;
}

template <class F, int W>
__device__ __forceinline__ void store_elems(u64* p, const Elems<F, W>& r) {
  if constexpr (F::LIMBS == 1 && W == 2) {
    u64x2 w;
    w.x = r.v[0];
    w.y = r.v[1];
    __builtin_nontemporal_store(w, reinterpret_cast<u64x2*>(p));
  } else if constexpr (F::LIMBS == 1) {
    __builtin_nontemporal_store(r.v[0], p);
  } else if constexpr (F::LIMBS == 2) {
    u64x2 w;
    w.x = (u64)r.v[0];
    w.y = (u64)(r.v[0] >> 64);
    __builtin_nontemporal_store(w, reinterpret_cast<u64x2*>(p));
  } else {
    u64x2 w0, w1;
    w0.x = r.v[0].w[0];
    w0.y = r.v[0].w[1];
    w1.x = r.v[0].w[2];
    w1.y = r.v[0].w[3];
    __builtin_nontemporal_store(w0, reinterpret_cast<u64x2*>(p));
    __builtin_nontemporal_store(w1, reinterpret_cast<u64x2*>(p) + 1);
  }
}

// dst[i .. i + W) = x - a
template <class F, int W>
__device__ __forceinline__ void mask_at(const typename F::Ctx& ctx, u64* dst, const u64* x, const u64* a, size_t i) {
  const Elems<F, W> xv = load_elems<F, W>(x + i * F::LIMBS), av = load_elems<F, W>(a + i * F::LIMBS);
  Elems<F, W> r;
#pragma unroll
  for (int v = 0; v < W; ++v) r.v[v] = beaver_mask_one<F>(ctx, xv.v[v], av.v[v]);
  store_elems<F, W>(dst + i * F::LIMBS, r);
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
  const size_t npacks = n / VEC, items = npacks + (VEC == 2 ? (n & 1) : 0);
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < items; q += (size_t)gridDim.x * BLOCK) {
    if (VEC == 1 || q < npacks) {
      mask_at<F, VEC>(ctx, e_out, x, a, q * VEC);
      mask_at<F, VEC>(ctx, d_out, y, b, q * VEC);
    } else {  // the odd element after the last pair
      mask_at<F, 1>(ctx, e_out, x, a, n - 1);
      mask_at<F, 1>(ctx, d_out, y, b, n - 1);
    }
  }
}

// z[r][i .. i + W) for every row r: e and d are loaded once, each row's a, b, c are read and its z written where they lie.
// A lane reads its elements of a row before it writes them, so z may be a, b or c.
template <class F, int W>
__device__ __forceinline__ void finish_at(const typename F::Ctx& ctx, u64* z, size_t z_stride, const u64* e, const u64* d, const u64* a,
                                          const u64* b, const u64* c, size_t op_stride, size_t rows, size_t ed_rows, size_t i) {
  const Elems<F, W> ev = load_elems<F, W>(e + i * F::LIMBS), dv = load_elems<F, W>(d + i * F::LIMBS);
#pragma unroll 1
  for (size_t r = 0; r < rows; ++r) {
    const size_t off = (r * op_stride + i) * F::LIMBS;
    const Elems<F, W> av = load_elems<F, W>(a + off), bv = load_elems<F, W>(b + off), cv = load_elems<F, W>(c + off);
    const bool add_ed = r < ed_rows;  // the same in every lane
    Elems<F, W> zv;
#pragma unroll
    for (int v = 0; v < W; ++v) zv.v[v] = beaver_finish_one<F>(ctx, ev.v[v], dv.v[v], av.v[v], bv.v[v], cv.v[v], add_ed);
    store_elems<F, W>(z + (r * z_stride + i) * F::LIMBS, zv);
  }
}

// One secret (VEC = 2: two) per lane across all rows: (4 rows + 2) N elements of traffic.
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_beaver_finish(typename F::Ctx ctx, u64* z, size_t z_stride, const u64* e, const u64* d,
                                                         const u64* a, const u64* b, const u64* c, size_t op_stride, size_t rows,
                                                         size_t ed_rows, size_t n) {
  const size_t npacks = n / VEC, items = npacks + (VEC == 2 ? (n & 1) : 0);
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < items; q += (size_t)gridDim.x * BLOCK) {
    if (VEC == 1 || q < npacks) finish_at<F, VEC>(ctx, z, z_stride, e, d, a, b, c, op_stride, rows, ed_rows, q * VEC);
    else finish_at<F, 1>(ctx, z, z_stride, e, d, a, b, c, op_stride, rows, ed_rows, n - 1);
  }
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
      if (two)
        hipLaunchKernelGGL((k_beaver_mask<F, F::LIMBS == 1 ? 2 : 1>), dim3(grid_for(N / 2 + (N & 1)), (unsigned)r), dim3(BLOCK), 0,
                           S(stream), ctx, out0, de_stride, d_off, x + in0, y + in0, a + in0, b + in0, op_stride, N);
      else
        hipLaunchKernelGGL((k_beaver_mask<F, 1>), dim3(grid_for(N), (unsigned)r), dim3(BLOCK), 0, S(stream), ctx, out0, de_stride,
                           d_off, x + in0, y + in0, a + in0, b + in0, op_stride, N);
      HIP_TRY(hipGetLastError());
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
    if (two_per_lane(F::LIMBS, {z, e, d, a, b, c}, {rows > 1 ? z_stride : 0, rows > 1 ? op_stride : 0}))
      hipLaunchKernelGGL((k_beaver_finish<F, F::LIMBS == 1 ? 2 : 1>), dim3(grid_for(N / 2 + (N & 1))), dim3(BLOCK), 0, S(stream), ctx, z,
                         z_stride, e, d, a, b, c, op_stride, rows, ed_rows, N);
    else
      hipLaunchKernelGGL((k_beaver_finish<F, 1>), dim3(grid_for(N)), dim3(BLOCK), 0, S(stream), ctx, z, z_stride, e, d, a, b, c,
                         op_stride, rows, ed_rows, N);
    HIP_TRY(hipGetLastError());
    return SCL_OK;
  });
}

}  // extern "C"
