// csrc/rb_unit.hip -- random shared bits: batched modular square roots with a per-element status, and the fused finish that
// turns opened squares u = r^2 and the parties' shares of r into shares of a bit, b = (r / sqrt(u) + 1) / 2; the kernels and the
// C ABI of libscl_hip_rb.so (include/scl_hip_rb.h), an extension library beside the engine.  One translation unit, the five
// prime fields.  The per-element arithmetic is include/scl_hip/detail/rb.hpp: one exponentiation of about the field's bit
// length per element (constant-time Tonelli-Shanks), its constants kernel arguments.
//
//   k_rb_sqrt          one lane = one element: the root or its inverse, and the status byte
//   k_rb_bits_finish   one lane = one column (Mersenne61: two where bases and strides allow): the chain once, then every row's
//                      b = h r + 2^-1.  Mersenne61 with rows <= 16 issues the row loads before the chain, so that they are in
//                      flight during it; elsewhere a row is loaded when it is used
// No LDS, no atomics, no allocation, no synchronisation: a lane's chain is 70 to about 385 dependent products, independent work
// comes from the other waves of the SIMD.  256-lane blocks, 16-byte non-temporal accesses, the odd last element of a Mersenne61
// row taken by the lane after the last pair (the conventions of csrc/unit_device.hpp).  The engine is reached through the
// prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_rb.h"
#include "../../include/scl_hip/detail/rb.hpp"
#include "kernels.hpp"
#include "unit_device.hpp"

namespace sclhip {
namespace {

constexpr int RB_PRELOAD_ROWS = 16;

template <class F>
__global__ __launch_bounds__(BLOCK) void k_rb_sqrt(typename F::Ctx ctx, RbParams<F> prm, u64* out, unsigned char* status, const u64* a, size_t N,
                                                   unsigned flags) {
  for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < N; q += (size_t)gridDim.x * BLOCK) {
    const RbRoot<F> r = rb_sqrt_one<F>(ctx, prm, load_pack<F, 1, true>(a + q * F::LIMBS).v[0], (flags & RB_ODD_ROOT) != 0);
    Pack<F, 1> o;
    o.v[0] = rb_sel<F>((flags & RB_INVERSE) != 0, r.inv, r.root);
    store_pack<F, 1, true>(out + q * F::LIMBS, o);
    status[q] = (unsigned char)r.status;
  }
}

// columns [i, i + W): PRE, the rows (at most RB_PRELOAD_ROWS) are loaded before the chain
template <class F, int W, bool PRE>
__device__ __forceinline__ void bits_at(const typename F::Ctx& ctx, const RbParams<F>& prm, u64* b, size_t b_stride, unsigned char* status, const u64* u,
                                        const u64* r, size_t r_stride, size_t rows, size_t i) {
  const Pack<F, W> uv = load_pack<F, W, true>(u + i * F::LIMBS);
  Pack<F, W> rv[PRE ? RB_PRELOAD_ROWS : 1];
  if constexpr (PRE) {
#pragma unroll
    for (int k = 0; k < RB_PRELOAD_ROWS; ++k)
      if ((size_t)k < rows) rv[k] = load_pack<F, W, true>(r + ((size_t)k * r_stride + i) * F::LIMBS);
  }
  typename F::E h[W];
  int st[W];
#pragma unroll
  for (int v = 0; v < W; ++v) h[v] = rb_bit_factor<F>(ctx, prm, uv.v[v], st[v]);
  if constexpr (PRE) {
#pragma unroll
    for (int k = 0; k < RB_PRELOAD_ROWS; ++k) {
      if ((size_t)k < rows) {
        Pack<F, W> o;
#pragma unroll
        for (int v = 0; v < W; ++v) o.v[v] = rb_bit_one<F>(ctx, prm, h[v], st[v], rv[k].v[v]);
        store_pack<F, W, true>(b + ((size_t)k * b_stride + i) * F::LIMBS, o);
      }
    }
  } else {
#pragma unroll 1
    for (size_t k = 0; k < rows; ++k) {
      rv[0] = load_pack<F, W, true>(r + (k * r_stride + i) * F::LIMBS);
      Pack<F, W> o;
#pragma unroll
      for (int v = 0; v < W; ++v) o.v[v] = rb_bit_one<F>(ctx, prm, h[v], st[v], rv[0].v[v]);
      store_pack<F, W, true>(b + (k * b_stride + i) * F::LIMBS, o);
    }
  }
#pragma unroll
  for (int v = 0; v < W; ++v) status[i + v] = (unsigned char)st[v];
}

template <class F, int VEC, bool PRE>
__global__ __launch_bounds__(BLOCK) void k_rb_bits_finish(typename F::Ctx ctx, RbParams<F> prm, u64* b, size_t b_stride, unsigned char* status,
                                                          const u64* u, const u64* r, size_t r_stride, size_t rows, size_t N) {
  if constexpr (PRE) {
    // the preloading form keeps the loop spelled out: through for_each_pack's callable the compiler schedules the sixteen row
    // loads and the chain differently (some instructions more for one column per lane, some fewer for two)
    const size_t pairs = N / VEC, items = pack_items<VEC>(N);
    for (size_t q = (size_t)blockIdx.x * BLOCK + threadIdx.x; q < items; q += (size_t)gridDim.x * BLOCK) {
      if (VEC == 1 || q < pairs) bits_at<F, VEC, true>(ctx, prm, b, b_stride, status, u, r, r_stride, rows, q * VEC);
      else bits_at<F, 1, true>(ctx, prm, b, b_stride, status, u, r, r_stride, rows, N - 1);  // the odd element after the last pair
    }
  } else {
    for_each_pack<VEC>(N, [&](auto w, size_t i) { bits_at<F, w, false>(ctx, prm, b, b_stride, status, u, r, r_stride, rows, i); });
  }
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#include "unit_host.hpp"

namespace {

// The constants of a field: made once per process where the field fixes its prime; for Mont128 kept with the modulus they were
// derived from, per thread like the latch, and made again when mont_latch hands over another one.  Host arithmetic only.
template <class F>
RbParams<F> params_for(const typename F::Ctx& ctx) {
  if constexpr (F::TAG == Mont128::TAG) {
    static thread_local u128 prime = 0;
    static thread_local RbParams<Mont128> cached;
    if (prime != ctx.p) {
      cached = rb_make_params<Mont128>(ctx);
      prime = ctx.p;
    }
    return cached;
  } else {
    static const RbParams<F> made = rb_make_params<F>(ctx);
    return made;
  }
}

// the tags this library refuses, each with its reason; SCL_OK for the five prime fields
int check_tag(const std::string& w, int field) {
  return check_prime_field(w, field, "squaring is a bijection of GF(2^128), every element has one root and r / sqrt(r^2) is always 1",
                           "a ring Z2k is not a field, square roots and Shamir sharings need one");
}

}  // namespace

extern "C" {

int scl_rb_abi_version(void) { return SCL_RB_ABI_VERSION; }
const char* scl_rb_last_error(void) { return g_err.c_str(); }

int scl_rb_sqrt(int field, uint64_t* out_dev, unsigned char* status_dev, const uint64_t* a_dev, size_t N, unsigned flags, void* stream) {
  if (N == 0) return SCL_OK;
  const std::string w = "sqrt";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  if (flags & ~(SCL_RB_ODD_ROOT | SCL_RB_INVERSE)) return fail(SCL_ERR_BAD_ARG, w + ": unknown flags bit (bit 0, the odd root, and bit 1, the inverse, are defined)");
  const size_t L = limbs_of(field), esz = 8 * L;
  if (const int rc = check_ptr(w, L, "out_dev", out_dev)) return rc;
  if (const int rc = check_ptr(w, L, "a_dev", a_dev)) return rc;
  if (!status_dev) return fail(SCL_ERR_BAD_ARG, w + ": status_dev is NULL");
  if (const int rc = alias_check("sqrt", {alias::vec("out_dev", out_dev, N, esz, true, 1), alias::vec("a_dev", a_dev, N, esz, false, 1),
                                         alias::vec("status_dev", status_dev, N, 1, true)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!rb_has_roots(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const RbParams<F> prm = params_for<F>(ctx);
      hipLaunchKernelGGL((k_rb_sqrt<F>), dim3(grid_for(N)), dim3(BLOCK), 0, S(stream), ctx, prm, out_dev, status_dev, a_dev, N, flags);
      HIP_TRY(hipGetLastError());
      return SCL_OK;
    }
  });
}

int scl_rb_bits_finish(int field, uint64_t* b_dev, size_t b_stride, unsigned char* status_dev, const uint64_t* u_dev, const uint64_t* r_dev,
                       size_t r_stride, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "bits_finish";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L;
  if (const int rc = check_ptr(w, L, "b_dev", b_dev)) return rc;
  if (const int rc = check_ptr(w, L, "u_dev", u_dev)) return rc;
  if (const int rc = check_ptr(w, L, "r_dev", r_dev)) return rc;
  if (!status_dev) return fail(SCL_ERR_BAD_ARG, w + ": status_dev is NULL");
  if (b_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": b_stride < N");
  if (r_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": r_stride < N");
  if (const int rc = alias_check("bits_finish", {alias::mat("b_dev", b_dev, rows, b_stride, N, esz, true, 1), alias::mat("r_dev", r_dev, rows, r_stride, N, esz, false, 1),
                                                alias::vec("u_dev", u_dev, N, esz, false), alias::vec("status_dev", status_dev, N, 1, true)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!rb_has_roots(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const RbParams<F> prm = params_for<F>(ctx);
      const bool two = two_per_lane(L, {b_dev, u_dev, r_dev}, {rows > 1 ? b_stride : 0, rows > 1 ? r_stride : 0});
      const dim3 grid(grid_for_packs(two, N));
      if constexpr (F::LIMBS == 1) {  // (the preloading form exists for the one-limb field only)
        if (rows <= (size_t)RB_PRELOAD_ROWS) {
          PACK_LAUNCH((k_rb_bits_finish, F, true), two, grid, S(stream), ctx, prm, b_dev, b_stride, status_dev, u_dev, r_dev, r_stride, rows, N);
          return SCL_OK;
        }
      }
      PACK_LAUNCH((k_rb_bits_finish, F, false), two, grid, S(stream), ctx, prm, b_dev, b_stride, status_dev, u_dev, r_dev, r_stride, rows, N);
      return SCL_OK;
    }
  });
}

}  // extern "C"
