// csrc/fx_unit.hip -- probabilistic truncation of Shamir sharings: the bounded random value composed from planes of shared bits,
// the mask c = x + 2^(k-1) + r with r' beside it, and the fused finish that opens c, reduces it modulo 2^shift as an integer and
// writes y = (x + r' - c') 2^-shift for every row; the kernels and the C ABI of libscl_hip_fx.so (include/scl_hip_fx.h), an
// extension library beside the engine.  One translation unit, the five prime fields.  The per-element arithmetic is
// include/scl_hip/detail/fx.hpp; the constants are kernel arguments.
//
//   k_fx_compose   one lane = one column of row blockIdx.y (Mersenne61: two where bases and strides allow): Horner from the top
//                  plane down, acc = 2 acc + b_i, no field product
//   k_fx_mask      the same walk with a second accumulator from plane shift - 1 down for r'; c and r' written in one launch
//   k_fx_finish    one lane = one column: the opening (lambda read from the kernel arguments with a wave-uniform index), the
//                  canonical integer (one from_mont for the Montgomery fields), the limb-wise mask, the range check, the rows
// The plane loop is rolled (B is a run-time value) in groups of FX_GROUP planes whose loads are issued before their arithmetic.
// No LDS, no atomics, no allocation, no synchronisation.  256-lane blocks, grid-stride loops, 16-byte non-temporal accesses, the
// odd last element of a Mersenne61 row taken by the lane after the last pair (the conventions of csrc/unit_device.hpp, whose
// open_at is the opening).  The engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_fx.h"
#include "../../include/scl_hip/detail/fx.hpp"
#include "kernels.hpp"
#include "unit_device.hpp"

namespace sclhip {
namespace {

constexpr int FX_GROUP = 4;  // planes whose loads are in flight together

// The planes B - 1 .. 0 of columns [i, i + W) of one row: r into acc, and -- LOW -- the planes below `shift` into low.  `bits`
// points at plane 0 of the row.  Lazy sums (fx_step): the caller canonicalises.
template <class F, int W, bool LOW>
__device__ __forceinline__ void planes_at(const typename F::Ctx& ctx, const u64* bits, size_t plane_stride, int B, int shift, size_t i,
                                          typename F::E (&acc)[W], typename F::E (&low)[W]) {
#pragma unroll
  for (int v = 0; v < W; ++v) {
    acc[v] = F::zero();
    low[v] = F::zero();
  }
  const u64* p = bits + i * F::LIMBS;
  int top = B;  // planes [0, top) are still to come
#pragma unroll 1
  for (; top >= FX_GROUP; top -= FX_GROUP) {
    Pack<F, W> b[FX_GROUP];
#pragma unroll
    for (int g = 0; g < FX_GROUP; ++g) b[g] = load_pack<F, W, true>(p + (size_t)(top - 1 - g) * plane_stride * F::LIMBS);
#pragma unroll
    for (int g = 0; g < FX_GROUP; ++g) {
#pragma unroll
      for (int v = 0; v < W; ++v) acc[v] = fx_step<F>(ctx, acc[v], b[g].v[v]);
      if constexpr (LOW) {
        if (top - 1 - g < shift) {  // (the same in every lane)
#pragma unroll
          for (int v = 0; v < W; ++v) low[v] = fx_step<F>(ctx, low[v], b[g].v[v]);
        }
      }
    }
  }
#pragma unroll 1
  for (; top > 0; --top) {
    const Pack<F, W> b = load_pack<F, W, true>(p + (size_t)(top - 1) * plane_stride * F::LIMBS);
#pragma unroll
    for (int v = 0; v < W; ++v) acc[v] = fx_step<F>(ctx, acc[v], b.v[v]);
    if constexpr (LOW) {
      if (top - 1 < shift) {
#pragma unroll
        for (int v = 0; v < W; ++v) low[v] = fx_step<F>(ctx, low[v], b.v[v]);
      }
    }
  }
}

template <class F, int W>
__device__ __forceinline__ void compose_at(const typename F::Ctx& ctx, u64* out, const u64* bits, size_t plane_stride, int B, size_t i) {
  typename F::E acc[W], low[W];
  planes_at<F, W, false>(ctx, bits, plane_stride, B, 0, i, acc, low);
  Pack<F, W> o;
#pragma unroll
  for (int v = 0; v < W; ++v) o.v[v] = fx_canon<F>(acc[v]);
  store_pack<F, W, true>(out + i * F::LIMBS, o);
}

// row blockIdx.y
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_fx_compose(typename F::Ctx ctx, u64* out, size_t out_stride, const u64* bits, size_t plane_stride,
                                                      size_t row_stride, int B, size_t N) {
  out += (size_t)blockIdx.y * out_stride * F::LIMBS;
  bits += (size_t)blockIdx.y * row_stride * F::LIMBS;
  for_each_pack<VEC>(N, [&](auto w, size_t i) { compose_at<F, w>(ctx, out, bits, plane_stride, B, i); });
}

// a lane reads its x before it writes its c, so c may be x
template <class F, int W>
__device__ __forceinline__ void mask_at(const typename F::Ctx& ctx, const FxMask<F>& prm, u64* c, u64* rlow, const u64* x, const u64* bits,
                                        size_t plane_stride, int B, int shift, size_t i) {
  const Pack<F, W> xv = load_pack<F, W, true>(x + i * F::LIMBS);
  typename F::E acc[W], low[W];
  planes_at<F, W, true>(ctx, bits, plane_stride, B, shift, i, acc, low);
  Pack<F, W> oc, ol;
#pragma unroll
  for (int v = 0; v < W; ++v) {
    oc.v[v] = fx_mask_one<F>(ctx, prm, xv.v[v], fx_canon<F>(acc[v]));
    ol.v[v] = fx_canon<F>(low[v]);
  }
  store_pack<F, W, true>(c + i * F::LIMBS, oc);
  store_pack<F, W, true>(rlow + i * F::LIMBS, ol);
}

template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_fx_mask(typename F::Ctx ctx, FxMask<F> prm, u64* c, size_t c_stride, u64* rlow, size_t rlow_stride,
                                                   const u64* x, size_t x_stride, const u64* bits, size_t plane_stride, size_t row_stride, int B,
                                                   int shift, size_t N) {
  c += (size_t)blockIdx.y * c_stride * F::LIMBS;
  rlow += (size_t)blockIdx.y * rlow_stride * F::LIMBS;
  x += (size_t)blockIdx.y * x_stride * F::LIMBS;
  bits += (size_t)blockIdx.y * row_stride * F::LIMBS;
  for_each_pack<VEC>(N, [&](auto w, size_t i) { mask_at<F, w>(ctx, prm, c, rlow, x, bits, plane_stride, B, shift, i); });
}

// y[r][i .. i + W) for every row r: the opened value once, its low bits and status, each row's x and r' read and its y written
// where it lies (a lane reads its elements before it writes them, so y may be x or r')
template <class F, int W>
__device__ __forceinline__ void finish_at(const typename F::Ctx& ctx, const FxFinish<F>& prm, u64* y, size_t y_stride, unsigned char* status,
                                          const u64* csh, size_t c_stride, const OpenTable<F>& lam, int m, const u64* x, size_t x_stride,
                                          const u64* rlow, size_t rlow_stride, size_t rows, size_t i) {
  typename F::E opened[W], cp[W];
  open_at<F, W>(ctx, csh, c_stride, lam.v, m, i, opened);  // (the table where it lies: the kernel arguments)
  int st[W];
#pragma unroll
  for (int v = 0; v < W; ++v) cp[v] = fx_finish_col<F>(ctx, prm, opened[v], st[v]);
#pragma unroll 1
  for (size_t r = 0; r < rows; ++r) {
    const Pack<F, W> xv = load_pack<F, W, true>(x + (r * x_stride + i) * F::LIMBS), lv = load_pack<F, W, true>(rlow + (r * rlow_stride + i) * F::LIMBS);
    Pack<F, W> o;
#pragma unroll
    for (int v = 0; v < W; ++v) o.v[v] = fx_finish_one<F>(ctx, prm, cp[v], st[v], xv.v[v], lv.v[v]);
    store_pack<F, W, true>(y + (r * y_stride + i) * F::LIMBS, o);
  }
#pragma unroll
  for (int v = 0; v < W; ++v) status[i + v] = (unsigned char)st[v];
}

template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_fx_finish(typename F::Ctx ctx, FxFinish<F> prm, u64* y, size_t y_stride, unsigned char* status,
                                                     const u64* csh, size_t c_stride, OpenTable<F> lam, int m, const u64* x, size_t x_stride,
                                                     const u64* rlow, size_t rlow_stride, size_t rows, size_t N) {
  for_each_pack<VEC>(N, [&](auto w, size_t i) {
    finish_at<F, w>(ctx, prm, y, y_stride, status, csh, c_stride, lam, m, x, x_stride, rlow, rlow_stride, rows, i);
  });
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#include "unit_host.hpp"

namespace {

// the tags this library refuses, each with its reason; SCL_OK for the five prime fields
int check_tag(const std::string& w, int field) {
  return check_prime_field(w, field, "GF(2^128) has no integers below a prime, there is nothing to reduce modulo 2^shift",
                           "a ring Z2k is not a field, it has no 2^-shift and no Shamir sharing");
}

// |p| - 2 of an accepted tag (`mont`: what mont_latch yielded)
size_t max_bits(int field, const Mont128::Ctx& mont) {
  switch (field) {
    case SCL_M61: return 59;
    case SCL_M127: return 125;
    case SCL_MONT128: return (size_t)fx_prime_bits<Mont128>(mont) - 2;
    default: return 254;
  }
}

// the planes as one operand (`extent`): the elements from plane 0 of row 0 to the end of plane B - 1 of row rows - 1
int check_planes(const std::string& w, size_t plane_stride, size_t row_stride, size_t B, size_t rows, size_t N, size_t* extent) {
  if (B > 1 && plane_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": plane_stride < N");
  if (rows > 1 && row_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": row_stride < N");
  if (!extent_of({{B, plane_stride}, {rows, row_stride}}, N, extent)) return fail(SCL_ERR_BAD_ARG, w + ": the extent of bits_dev overflows");
  return SCL_OK;
}

}  // namespace

extern "C" {

int scl_fx_abi_version(void) { return SCL_FX_ABI_VERSION; }
const char* scl_fx_last_error(void) { return g_err.c_str(); }

size_t scl_fx_max_bits(int field) {
  if (check_tag("max_bits", field) != SCL_OK) return 0;
  Mont128::Ctx mont = {};
  if (mont_latch(field, mont) != SCL_OK) return 0;
  return max_bits(field, mont);
}

int scl_fx_compose(int field, uint64_t* out_dev, size_t out_stride, const uint64_t* bits_dev, size_t plane_stride, size_t row_stride, size_t B,
                   size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "compose";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L, top = max_bits(field, mont);
  if (B == 0 || B > top) return fail(SCL_ERR_BAD_ARG, w + ": B must be in 1.." + std::to_string(top) + " for this field (|p| - 2: the composed value stays below p)");
  if (const int rc = check_ptr(w, L, "out_dev", out_dev)) return rc;
  if (const int rc = check_ptr(w, L, "bits_dev", bits_dev)) return rc;
  if (out_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": out_stride < N");
  size_t extent = 0;
  if (const int rc = check_planes(w, plane_stride, row_stride, B, rows, N, &extent)) return rc;
  if (const int rc = alias_check("compose", {alias::mat("out_dev", out_dev, rows, out_stride, N, esz, true), alias::vec("bits_dev", bits_dev, extent, esz, false)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!fx_has_trunc(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const bool two = two_per_lane(L, {out_dev, bits_dev}, {rows > 1 ? out_stride : 0, rows > 1 ? row_stride : 0, B > 1 ? plane_stride : 0});
      for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
        const size_t nr = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
        uint64_t* o = out_dev + r0 * out_stride * L;
        const uint64_t* b = bits_dev + r0 * row_stride * L;
        PACK_LAUNCH((k_fx_compose, F), two, dim3(grid_for_packs(two, N), (unsigned)nr), S(stream), ctx, o, out_stride, b, plane_stride, row_stride,
                    (int)B, N);
      }
      return SCL_OK;
    }
  });
}

int scl_fx_trunc_mask(int field, uint64_t* c_dev, size_t c_stride, uint64_t* rlow_dev, size_t rlow_stride, const uint64_t* x_dev, size_t x_stride,
                      const uint64_t* bits_dev, size_t plane_stride, size_t row_stride, size_t k, size_t shift, size_t B, size_t rows, size_t N,
                      void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "trunc_mask";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L, top = max_bits(field, mont);
  if (shift == 0) return fail(SCL_ERR_BAD_ARG, w + ": shift == 0: there is nothing to truncate");
  if (shift >= k) return fail(SCL_ERR_BAD_ARG, w + ": shift >= k: every bit of a k-bit value would be dropped");
  if (k > B) return fail(SCL_ERR_BAD_ARG, w + ": k > B: the B random bits do not cover the k bits of the value");
  if (B > top) return fail(SCL_ERR_BAD_ARG, w + ": B > scl_fx_max_bits: B must be at most " + std::to_string(top) + " for this field (|p| - 2: the masked value stays below p)");
  if (const int rc = check_ptr(w, L, "c_dev", c_dev)) return rc;
  if (const int rc = check_ptr(w, L, "rlow_dev", rlow_dev)) return rc;
  if (const int rc = check_ptr(w, L, "x_dev", x_dev)) return rc;
  if (const int rc = check_ptr(w, L, "bits_dev", bits_dev)) return rc;
  if (c_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": c_stride < N");
  if (rlow_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": rlow_stride < N");
  if (x_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": x_stride < N");
  size_t extent = 0;
  if (const int rc = check_planes(w, plane_stride, row_stride, B, rows, N, &extent)) return rc;
  if (const int rc = alias_check("trunc_mask", {alias::mat("c_dev", c_dev, rows, c_stride, N, esz, true, 1), alias::mat("x_dev", x_dev, rows, x_stride, N, esz, false, 1),
                                               alias::mat("rlow_dev", rlow_dev, rows, rlow_stride, N, esz, true), alias::vec("bits_dev", bits_dev, extent, esz, false)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!fx_has_trunc(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const FxMask<F> prm = fx_make_mask<F>(ctx, (int)k);
      const bool two = two_per_lane(L, {c_dev, rlow_dev, x_dev, bits_dev}, {rows > 1 ? c_stride : 0, rows > 1 ? rlow_stride : 0, rows > 1 ? x_stride : 0,
                                                                            rows > 1 ? row_stride : 0, B > 1 ? plane_stride : 0});
      for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
        const size_t nr = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
        uint64_t *c = c_dev + r0 * c_stride * L, *lo = rlow_dev + r0 * rlow_stride * L;
        const uint64_t *x = x_dev + r0 * x_stride * L, *b = bits_dev + r0 * row_stride * L;
        PACK_LAUNCH((k_fx_mask, F), two, dim3(grid_for_packs(two, N), (unsigned)nr), S(stream), ctx, prm, c, c_stride, lo, rlow_stride, x, x_stride, b,
                    plane_stride, row_stride, (int)B, (int)shift, N);
      }
      return SCL_OK;
    }
  });
}

int scl_fx_trunc_finish(int field, uint64_t* y_dev, size_t y_stride, unsigned char* status_dev, const uint64_t* csh_dev, size_t c_stride,
                        const uint64_t* lambda_host, size_t m, const uint64_t* x_dev, size_t x_stride, const uint64_t* rlow_dev, size_t rlow_stride,
                        size_t shift, size_t B, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "trunc_finish";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L, top = max_bits(field, mont);
  if (shift == 0) return fail(SCL_ERR_BAD_ARG, w + ": shift == 0: there is nothing to truncate");
  if (shift >= B) return fail(SCL_ERR_BAD_ARG, w + ": shift >= B: shift is below k and k at most B");
  if (B > top) return fail(SCL_ERR_BAD_ARG, w + ": B > scl_fx_max_bits: B must be at most " + std::to_string(top) + " for this field (|p| - 2: the opened value stays below p)");
  if (m == 0 || m > (size_t)OPEN_M_MAX)
    return fail(SCL_ERR_BAD_ARG, w + ": m must be in 1..64 (lambda travels with the launch); beyond that open with scl_hip_shamir_recover and pass m = 1, lambda = {1}");
  if (const int rc = check_ptr(w, L, "y_dev", y_dev)) return rc;
  if (!status_dev) return fail(SCL_ERR_BAD_ARG, w + ": status_dev is NULL");
  if (const int rc = check_ptr(w, L, "csh_dev", csh_dev)) return rc;
  if (!lambda_host) return fail(SCL_ERR_BAD_ARG, w + ": lambda_host is NULL");
  if (const int rc = check_ptr(w, L, "x_dev", x_dev)) return rc;
  if (const int rc = check_ptr(w, L, "rlow_dev", rlow_dev)) return rc;
  if (y_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": y_stride < N");
  if (c_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": c_stride < N");
  if (x_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": x_stride < N");
  if (rlow_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": rlow_stride < N");
  if (const int rc = alias_check("trunc_finish", {alias::mat("y_dev", y_dev, rows, y_stride, N, esz, true, 1), alias::mat("x_dev", x_dev, rows, x_stride, N, esz, false, 1),
                                                 alias::mat("rlow_dev", rlow_dev, rows, rlow_stride, N, esz, false, 1),
                                                 alias::mat("csh_dev", csh_dev, m, c_stride, N, esz, false), alias::vec("status_dev", status_dev, N, 1, true)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!fx_has_trunc(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const FxFinish<F> prm = fx_make_finish<F>(ctx, (int)shift, (int)B);
      const bool two = two_per_lane(L, {y_dev, csh_dev, x_dev, rlow_dev}, {rows > 1 ? y_stride : 0, rows > 1 ? x_stride : 0, rows > 1 ? rlow_stride : 0, m > 1 ? c_stride : 0});
      PACK_LAUNCH((k_fx_finish, F), two, dim3(grid_for_packs(two, N)), S(stream), ctx, prm, y_dev, y_stride, status_dev, csh_dev, c_stride,
                  make_open_table<F>(lambda_host, m), (int)m, x_dev, x_stride, rlow_dev, rlow_stride, rows, N);
      return SCL_OK;
    }
  });
}

}  // extern "C"
