// csrc/ip_unit.hip -- inner and matrix products of Shamir sharings at one opening each: the local step
// [d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t over many independent instances; the kernels and the C ABI of libscl_hip_ip.so
// (include/scl_hip_ip.h), an extension library beside the engine.  One translation unit, all six fields.  The per-element
// arithmetic is include/scl_hip/detail/ip.hpp, on the matrix kernels' accumulator (kernels.hpp: MatAcc -- the field's Acc, column
// sums for Mersenne127).
//
//   k_ip_dot      one lane = one column of row blockIdx.y (Mersenne61: two), grid-stride over N: 2 terms coalesced loads into one
//                 accumulator, the loads of dot_unroll<F>() terms issued before their products are consumed, r2 as one more term, one store
//   k_ip_matmul   one lane = one column of batch blockIdx.y and the TI x TL output tile blockIdx.z: TI TL accumulators, TI + TL
//                 operand loads per k, rows and columns past the matrix edge clamped and discarded as k_matmul clamps; one term
//                 count for all accumulators, which fold together
// A 1 x 1 product is the dot kernel (rows = batches).  The streaming kernel keeps the conventions of csrc/unit_device.hpp: 256-lane
// blocks, 16-byte non-temporal accesses, the pack width of Mersenne61 chosen on the host per call, the odd last element taken by
// the lane after the last pair.  The matrix kernel reads its operands cached: every element is read once per tile row or column.
// The engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_ip.h"
#include "../../include/scl_hip/detail/ip.hpp"
#include "kernels.hpp"
#include "unit_device.hpp"

namespace sclhip {
namespace {

// terms whose 2 W loads a lane issues before it consumes the first product: 16 bytes each for one- and two-limb fields (8 loads
// in flight), 32 bytes for the wide ones (4 loads of two requests each) -- docs/kernels/ip.md
template <class F>
constexpr int dot_unroll() {
  return F::LIMBS == 4 ? 2 : 4;
}

// d[i .. i + W) = sum_k x[k] y[k] (+ r2); a lane reads r2 before it writes d, so d may be r2
template <class F, int W>
__device__ __forceinline__ void dot_at(const typename F::Ctx& ctx, u64* d, const u64* x, size_t xts, const u64* y, size_t yts, const u64* r2,
                                       size_t nterms, size_t i) {
  constexpr int U = dot_unroll<F>();
  Pack<F, W> rv;
  if (r2) rv = load_pack<F, W, true>(r2 + i * F::LIMBS);
  MatAcc<F> acc[W];
#pragma unroll
  for (int v = 0; v < W; ++v) acc[v].zero();
  int terms = 0;
  x += i * F::LIMBS;  // the lane's own pointers, advanced term by term
  y += i * F::LIMBS;
  const size_t xstep = xts * F::LIMBS, ystep = yts * F::LIMBS;
  size_t k = 0;
  for (; k + U <= nterms; k += U) {
    Pack<F, W> xv[U], yv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xv[u] = load_pack<F, W, true>(x + u * xstep);
      yv[u] = load_pack<F, W, true>(y + u * ystep);
    }
    x += U * xstep;
    y += U * ystep;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      ip_take_term<F, W>(ctx, acc, terms);  // one count for the lane's W accumulators
#pragma unroll
      for (int v = 0; v < W; ++v) acc[v].mac(ctx, xv[u].v[v], yv[u].v[v]);
    }
  }
  for (; k < nterms; ++k) {
    const Pack<F, W> xv = load_pack<F, W, true>(x), yv = load_pack<F, W, true>(y);
    x += xstep;
    y += ystep;
    ip_take_term<F, W>(ctx, acc, terms);
#pragma unroll
    for (int v = 0; v < W; ++v) acc[v].mac(ctx, xv.v[v], yv.v[v]);
  }
  if (r2) ip_take_term<F, W>(ctx, acc, terms);  // the addend is a term
  Pack<F, W> o;
#pragma unroll
  for (int v = 0; v < W; ++v) o.v[v] = ip_add_fold<F>(ctx, acc[v], r2 != nullptr, r2 ? rv.v[v] : F::zero());
  store_pack<F, W, true>(d + i * F::LIMBS, o);
}

// row blockIdx.y; every operand has a row stride of its own (the 1 x 1 matrix product passes its batch strides)
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_ip_dot(typename F::Ctx ctx, u64* d, size_t d_rs, const u64* x, size_t x_ts, size_t x_rs, const u64* y,
                                                  size_t y_ts, size_t y_rs, const u64* r2, size_t r2_rs, size_t nterms, size_t N) {
  d += (size_t)blockIdx.y * d_rs * F::LIMBS;
  x += (size_t)blockIdx.y * x_rs * F::LIMBS;
  y += (size_t)blockIdx.y * y_rs * F::LIMBS;
  if (r2) r2 += (size_t)blockIdx.y * r2_rs * F::LIMBS;
  for_each_pack<VEC>(N, [&](auto w, size_t i) { dot_at<F, w>(ctx, d, x, x_ts, y, y_ts, r2, nterms, i); });
}

// the output tile a lane owns: what the registers hold without scratch (docs/kernels/ip.md has the figures)
template <class F>
struct Tile {
  enum { TI = F::LIMBS == 1 ? 4 : 2, TL = F::LIMBS == 4 ? 2 : 4 };
};

// tile t0 + blockIdx.z of batch blockIdx.y: output rows [i0, i0 + TI), columns [l0, l0 + TL)
template <class F, int TI, int TL>
__global__ __launch_bounds__(BLOCK) void k_ip_matmul(typename F::Ctx ctx, u64* D, size_t ds, size_t dbs, const u64* X, size_t xs, size_t xbs,
                                                     const u64* Y, size_t ys, size_t ybs, const u64* R2, size_t rs, size_t rbs, size_t t0,
                                                     int tiles_l, int a, int K, int b, size_t N) {
  const size_t tile = t0 + blockIdx.z;
  const int i0 = (int)(tile / tiles_l) * TI, l0 = (int)(tile % tiles_l) * TL;
  D += (size_t)blockIdx.y * dbs * F::LIMBS;
  X += (size_t)blockIdx.y * xbs * F::LIMBS;
  Y += (size_t)blockIdx.y * ybs * F::LIMBS;
  if (R2) R2 += (size_t)blockIdx.y * rbs * F::LIMBS;
  // clamp: rows and columns past the edge repeat the last one and are discarded below
  size_t xrow[TI], ycol[TL];
#pragma unroll
  for (int i = 0; i < TI; ++i) xrow[i] = (size_t)(i0 + i < a ? i0 + i : a - 1) * K * xs;
#pragma unroll
  for (int l = 0; l < TL; ++l) ycol[l] = (size_t)(l0 + l < b ? l0 + l : b - 1) * ys;
  for (size_t s = (size_t)blockIdx.x * BLOCK + threadIdx.x; s < N; s += (size_t)gridDim.x * BLOCK) {
    MatAcc<F> acc[TI][TL];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int l = 0; l < TL; ++l) acc[i][l].zero();
    int terms = 0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
      typename F::E xv[TI], yv[TL];
#pragma unroll
      for (int i = 0; i < TI; ++i) xv[i] = load_pack<F, 1, false>(X + (xrow[i] + (size_t)k * xs + s) * F::LIMBS).v[0];
#pragma unroll
      for (int l = 0; l < TL; ++l) yv[l] = load_pack<F, 1, false>(Y + ((size_t)k * b * ys + ycol[l] + s) * F::LIMBS).v[0];
      ip_take_term<F, TI * TL>(ctx, &acc[0][0], terms);  // one count for all accumulators: they fold together
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int l = 0; l < TL; ++l) acc[i][l].mac(ctx, xv[i], yv[l]);
    }
    if (R2) ip_take_term<F, TI * TL>(ctx, &acc[0][0], terms);  // the addend is a term, for the whole tile at once
    // entry (i0, l0) of D and of R2 in this lane's column; the tile is walked from there
    const size_t e0 = (size_t)i0 * b + l0;
    u64* dp = D + (e0 * ds + s) * F::LIMBS;
    const u64* rp = R2 ? R2 + (e0 * rs + s) * F::LIMBS : nullptr;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
#pragma unroll
      for (int l = 0; l < TL; ++l) {
        if (i0 + i < a && l0 + l < b) {  // past the edge: computed from clamped operands, discarded
          typename F::E r = F::zero();
          if (R2) r = load_pack<F, 1, true>(rp + (size_t)l * rs * F::LIMBS).v[0];
          Pack<F, 1> o;
          o.v[0] = ip_add_fold<F>(ctx, acc[i][l], R2 != nullptr, r);
          store_pack<F, 1, true>(dp + (size_t)l * ds * F::LIMBS, o);
        }
      }
      dp += (size_t)b * ds * F::LIMBS;
      if (R2) rp += (size_t)b * rs * F::LIMBS;
    }
  }
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#include "unit_host.hpp"

namespace {

constexpr size_t DIM_MAX = 65535;  // a, K and b of a matrix product

// d against the inputs (alias::conflict names the pair), then d against r2, which it may be exactly (`same`)
int alias_check(const char* who, size_t esz, const void* d, size_t de, const void* x, size_t xe, const void* y, size_t ye, const void* r2, size_t re,
                bool same) {
  std::string msg;
  const alias::Operand ops[3] = {alias::vec("d_dev", d, de, esz, true), alias::vec("x_dev", x, xe, esz, false), alias::vec("y_dev", y, ye, esz, false)};
  if (alias::conflict(who, ops, 3, &msg) != alias::DISJOINT) return fail(SCL_ERR_BAD_ARG, msg);
  const alias::Operand pr[2] = {ops[0], alias::vec("r2_dev", same ? nullptr : r2, re, esz, false)};
  if (alias::conflict(who, pr, 2, &msg) != alias::DISJOINT)
    return fail(SCL_ERR_BAD_ARG, msg + (msg.find("overlaps") != std::string::npos ? " (they may coincide -- the same pointer and strides -- and not overlap otherwise)" : ""));
  return SCL_OK;
}

// rows [0, rows) of the dot kernel, one launch per 65535; every operand with its own row stride
template <class F>
int launch_dot(const typename F::Ctx& ctx, bool two, uint64_t* d, size_t d_rs, const uint64_t* x, size_t x_ts, size_t x_rs, const uint64_t* y,
               size_t y_ts, size_t y_rs, const uint64_t* r2, size_t r2_rs, size_t terms, size_t rows, size_t N, void* stream) {
  constexpr size_t L = F::LIMBS;
  for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
    const size_t r = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
    uint64_t* o = d + r0 * d_rs * L;
    const uint64_t *xx = x + r0 * x_rs * L, *yy = y + r0 * y_rs * L, *rr = r2 ? r2 + r0 * r2_rs * L : nullptr;
    PACK_LAUNCH((k_ip_dot, F), two, dim3(grid_for_packs(two, N), (unsigned)r), S(stream), ctx, o, d_rs, xx, x_ts, x_rs, yy, y_ts, y_rs, rr, r2_rs,
                terms, N);
  }
  return SCL_OK;
}
}  // namespace

extern "C" {

int scl_ip_abi_version(void) { return SCL_IP_ABI_VERSION; }
const char* scl_ip_last_error(void) { return g_err.c_str(); }

void scl_ip_matmul_tile(int field, int* ti, int* tl) {
  int i = 0, l = 0;
  switch (limbs_of(field)) {
    case 1: i = Tile<M61>::TI, l = Tile<M61>::TL; break;
    case 2: i = Tile<M127>::TI, l = Tile<M127>::TL; break;
    case 4: i = Tile<Secp256k1Scalar>::TI, l = Tile<Secp256k1Scalar>::TL; break;
    default: break;
  }
  if (ti) *ti = i;
  if (tl) *tl = l;
}

int scl_ip_dot_mask(int field, uint64_t* d_dev, size_t d_stride, const uint64_t* x_dev, size_t x_term_stride, const uint64_t* y_dev,
                    size_t y_term_stride, const uint64_t* r2_dev, size_t op_stride, size_t terms, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field);
  if (terms == 0) return fail(SCL_ERR_BAD_ARG, "dot_mask: terms must be at least 1");
  if (!d_dev || !x_dev || !y_dev) return fail(SCL_ERR_BAD_ARG, "dot_mask: NULL operand (only r2_dev may be NULL: no addend)");
  if (const int rc = check_align("dot_mask", L, {d_dev, x_dev, y_dev, r2_dev})) return rc;
  if (d_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "dot_mask: d_stride < N");
  if (op_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "dot_mask: op_stride < N");
  size_t de = 0, xe = 0, ye = 0, re = 0;
  if (!extent_of({{rows, d_stride}}, N, &de)) return fail(SCL_ERR_BAD_ARG, "dot_mask: the extent of d_dev overflows");
  if (!extent_of({{terms, x_term_stride}, {rows, op_stride}}, N, &xe)) return fail(SCL_ERR_BAD_ARG, "dot_mask: the extent of x_dev overflows");
  if (!extent_of({{terms, y_term_stride}, {rows, op_stride}}, N, &ye)) return fail(SCL_ERR_BAD_ARG, "dot_mask: the extent of y_dev overflows");
  if (!extent_of({{rows, op_stride}}, N, &re)) return fail(SCL_ERR_BAD_ARG, "dot_mask: the extent of r2_dev overflows");
  const bool same = r2_dev == d_dev && (rows == 1 || d_stride == op_stride);
  if (const int rc = alias_check("dot_mask", 8 * L, d_dev, de, x_dev, xe, y_dev, ye, r2_dev, re, same)) return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    const bool two = two_per_lane(L, {d_dev, x_dev, y_dev, r2_dev},
                                  {rows > 1 ? d_stride : 0, rows > 1 ? op_stride : 0, terms > 1 ? x_term_stride : 0, terms > 1 ? y_term_stride : 0});
    return launch_dot<F>(ctx, two, d_dev, d_stride, x_dev, x_term_stride, op_stride, y_dev, y_term_stride, op_stride, r2_dev, op_stride, terms, rows,
                         N, stream);
  });
}

int scl_ip_matmul_mask(int field, uint64_t* d_dev, size_t d_stride, size_t d_batch_stride, const uint64_t* x_dev, size_t x_stride,
                       size_t x_batch_stride, const uint64_t* y_dev, size_t y_stride, size_t y_batch_stride, const uint64_t* r2_dev,
                       size_t r2_stride, size_t r2_batch_stride, size_t a, size_t K, size_t b, size_t batch, size_t N, void* stream) {
  if (N == 0 || batch == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field);
  if (a == 0 || K == 0 || b == 0 || a > DIM_MAX || K > DIM_MAX || b > DIM_MAX)
    return fail(SCL_ERR_BAD_ARG, "matmul_mask: a, K and b must be at least 1 and at most 65535");
  if (!d_dev || !x_dev || !y_dev) return fail(SCL_ERR_BAD_ARG, "matmul_mask: NULL operand (only r2_dev may be NULL: no addend)");
  if (const int rc = check_align("matmul_mask", L, {d_dev, x_dev, y_dev, r2_dev})) return rc;
  if (d_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "matmul_mask: d_stride < N");
  if (x_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "matmul_mask: x_stride < N");
  if (y_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "matmul_mask: y_stride < N");
  if (r2_dev && r2_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "matmul_mask: r2_stride < N");
  if (batch == 1) d_batch_stride = x_batch_stride = y_batch_stride = r2_batch_stride = 0;
  size_t de = 0, xe = 0, ye = 0, re = 0, one = 0;
  if (!extent_of({{a * b, d_stride}}, N, &one) || !extent_of({{batch, d_batch_stride}, {a * b, d_stride}}, N, &de))
    return fail(SCL_ERR_BAD_ARG, "matmul_mask: the extent of d_dev overflows");
  if (batch > 1 && d_batch_stride < one)
    return fail(SCL_ERR_BAD_ARG, "matmul_mask: d_batch_stride is too small to keep the batches of d_dev apart (" + std::to_string(one) +
                                     " elements at the least)");
  if (!extent_of({{batch, x_batch_stride}, {a * K, x_stride}}, N, &xe)) return fail(SCL_ERR_BAD_ARG, "matmul_mask: the extent of x_dev overflows");
  if (!extent_of({{batch, y_batch_stride}, {K * b, y_stride}}, N, &ye)) return fail(SCL_ERR_BAD_ARG, "matmul_mask: the extent of y_dev overflows");
  if (!extent_of({{batch, r2_batch_stride}, {a * b, r2_stride}}, N, &re)) return fail(SCL_ERR_BAD_ARG, "matmul_mask: the extent of r2_dev overflows");
  const bool same = r2_dev == d_dev && (a * b == 1 || d_stride == r2_stride) && (batch == 1 || d_batch_stride == r2_batch_stride);
  if (const int rc = alias_check("matmul_mask", 8 * L, d_dev, de, x_dev, xe, y_dev, ye, r2_dev, re, same)) return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    if (a == 1 && b == 1) {  // the inner product: one streaming form (rows = batches, terms = K)
      const bool two = two_per_lane(L, {d_dev, x_dev, y_dev, r2_dev},
                                    {d_batch_stride, x_batch_stride, y_batch_stride, r2_dev ? r2_batch_stride : 0, K > 1 ? x_stride : 0, K > 1 ? y_stride : 0});
      return launch_dot<F>(ctx, two, d_dev, d_batch_stride, x_dev, x_stride, x_batch_stride, y_dev, y_stride, y_batch_stride, r2_dev, r2_batch_stride, K,
                           batch, N, stream);
    }
    constexpr int TI = Tile<F>::TI, TL = Tile<F>::TL;
    const size_t tiles_i = (a + TI - 1) / TI, tiles_l = (b + TL - 1) / TL, tiles = tiles_i * tiles_l;
    for (size_t q0 = 0; q0 < batch; q0 += GRID_Y_MAX) {
      const size_t nq = batch - q0 < GRID_Y_MAX ? batch - q0 : GRID_Y_MAX;
      for (size_t t0 = 0; t0 < tiles; t0 += GRID_Y_MAX) {
        const size_t nt = tiles - t0 < GRID_Y_MAX ? tiles - t0 : GRID_Y_MAX;
        hipLaunchKernelGGL((k_ip_matmul<F, TI, TL>), dim3(grid_for(N), (unsigned)nq, (unsigned)nt), dim3(BLOCK), 0, S(stream), ctx,
                           d_dev + q0 * d_batch_stride * L, d_stride, d_batch_stride, x_dev + q0 * x_batch_stride * L, x_stride, x_batch_stride,
                           y_dev + q0 * y_batch_stride * L, y_stride, y_batch_stride, r2_dev ? r2_dev + q0 * r2_batch_stride * L : nullptr, r2_stride,
                           r2_batch_stride, t0, (int)tiles_l, (int)a, (int)K, (int)b, N);
        HIP_TRY(hipGetLastError());
      }
    }
    return SCL_OK;
  });
}

}  // extern "C"
