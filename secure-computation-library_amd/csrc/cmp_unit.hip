// csrc/cmp_unit.hip -- the bitwise less-than of an opened value against shared bits, and the exact results on top of it: the first
// level of the comparison tree fused with the opening of c, a later level, and the local finish (x mod 2^w, floor(x / 2^w),
// [x < 0]); the kernels and the C ABI of libscl_hip_cmp.so (include/scl_hip_cmp.h), an extension library beside the engine.  One
// translation unit, the five prime fields.  The per-element arithmetic is include/scl_hip/detail/cmp.hpp; the constants are kernel
// arguments.
//
//   k_cmp_open     one lane = one column (Mersenne61: two where bases and strides allow): the opening (lambda read from the kernel
//                  arguments with a wave-uniform index), the canonical integer, its status and low w bits: cmod, written once
//   k_cmp_first    one lane = one column of the pair of bit planes blockIdx.y: the two public bits from cmod (a per-lane select,
//                  the plane index the same in every lane), then the lane walks its rows: the leaves from the shares, the combined
//                  node + r2 -> d.  The leaves are never written.  Both launches are one entry point, scl_cmp_first_mask.
//   k_cmp_level    one lane = one column of row blockIdx.y of output node blockIdx.z: eq_hi lt_lo + lt_hi + r2 and eq_hi eq_lo +
//                  r2, one product each, folded once; a lone last node passes through as node + r2
//   k_cmp_finish   one lane = one column: cmod and the status once, then the rows
// No LDS, no atomics, no allocation, no synchronisation.  256-lane blocks, grid-stride loops, 16-byte non-temporal accesses, the
// odd last element of a Mersenne61 row taken by the lane after the last pair (the conventions of csrc/unit_device.hpp, whose
// open_at is the opening).  The engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_cmp.h"
#include "../../include/scl_hip/detail/cmp.hpp"
#include "kernels.hpp"
#include "unit_device.hpp"

namespace sclhip {
namespace {

// a node array (or the bit planes) on the device: plane q, row r at p + (q * plane + r * row) * LIMBS
struct Planes {
  size_t plane, row;
};

// limb l of a lane's integer, l the same in every lane: masks over registers, no indexed access
template <int L>
__device__ __forceinline__ u64 limb_at(const u64 (&w)[L], int l) {
  u64 r = 0;
#pragma unroll
  for (int i = 0; i < L; ++i) r |= w[i] & ((u64)0 - (u64)(l == i));
  return r;
}

// the opening, once per column: cmod and the status
template <class F, int W>
__device__ __forceinline__ void open_col_at(const typename F::Ctx& ctx, const FxFinish<F>& prm, u64* cmod, unsigned char* status, const u64* csh,
                                            size_t c_stride, const OpenTable<F>& lam, int m, size_t i) {
  typename F::E opened[W];
  open_at<F, W>(ctx, csh, c_stride, lam.v, m, i, opened);
  Pack<F, W> cm;
#pragma unroll
  for (int v = 0; v < W; ++v) {
    u64 cw[F::LIMBS];
    int st;
    cm.v[v] = cmp_open_col<F>(ctx, prm, opened[v], cw, st);
    status[i + v] = (unsigned char)st;
  }
  store_pack<F, W, true>(cmod + i * F::LIMBS, cm);
}

template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_cmp_open(typename F::Ctx ctx, FxFinish<F> prm, u64* cmod, unsigned char* status, const u64* csh,
                                                    size_t c_stride, OpenTable<F> lam, int m, size_t N) {
  for_each_pack<VEC>(N, [&](auto pw, size_t i) { open_col_at<F, pw>(ctx, prm, cmod, status, csh, c_stride, lam, m, i); });
}

// pair j of columns [i, i + W): the two public bits from cmod (read through the cache: every pair of the column reads it), then
// the rows.  b_lo, r_lt, d_lt: plane 2j of row 0 (the partner's plane, the eq plane: one plane on).
template <class F, int W, bool lt_only>
__device__ __forceinline__ void first_at(const typename F::Ctx& ctx, u64* d_lt, Planes dp, const u64* cmod, const u64* b_lo, Planes bp, const u64* r_lt,
                                         Planes rp, int j, bool has_hi, size_t rows, size_t i) {
  const Pack<F, W> cm = load_pack<F, W, false>(cmod + i * F::LIMBS);
  u64 m_lo[W], m_hi[W];  // all ones where the public bit is set
#pragma unroll
  for (int v = 0; v < W; ++v) {
    u64 cw[F::LIMBS];
    fx_limbs<F>(ctx, cm.v[v], cw);
    const u64 limb = limb_at<F::LIMBS>(cw, j >> 5) >> ((2 * j) & 63);  // bits 2j and 2j + 1 share a limb
    m_lo[v] = (u64)0 - (limb & 1);
    m_hi[v] = (u64)0 - ((limb >> 1) & 1);
  }
  const typename F::E zero = F::zero(), one = F::one(ctx);
  // the lane's own pointers, advanced row by row
  const u64 *b = b_lo + i * F::LIMBS, *rr = r_lt + i * F::LIMBS;
  u64* o = d_lt + i * F::LIMBS;
#pragma unroll 1
  for (size_t r = 0; r < rows; ++r, b += bp.row * F::LIMBS, rr += rp.row * F::LIMBS, o += dp.row * F::LIMBS) {
    const Pack<F, W> lo = load_pack<F, W, true>(b), rl = load_pack<F, W, true>(rr);
    Pack<F, W> hi, re, o_lt, o_eq;
    if (has_hi) hi = load_pack<F, W, true>(b + bp.plane * F::LIMBS);
    if constexpr (!lt_only) re = load_pack<F, W, true>(rr + rp.plane * F::LIMBS);
#pragma unroll
    for (int v = 0; v < W; ++v) {
      typename F::E lt_lo, eq_lo, lt_hi = zero, eq_hi = one;  // no partner: the identity
      cmp_leaf<F>(ctx, m_lo[v], lo.v[v], lt_lo, eq_lo);
      if (has_hi) cmp_leaf<F>(ctx, m_hi[v], hi.v[v], lt_hi, eq_hi);
      o_lt.v[v] = cmp_combine_lt<F>(ctx, lt_hi, eq_hi, lt_lo, rl.v[v]);
      if constexpr (!lt_only) o_eq.v[v] = cmp_combine_eq<F>(ctx, eq_hi, eq_lo, re.v[v]);
    }
    store_pack<F, W, true>(o, o_lt);
    if constexpr (!lt_only) store_pack<F, W, true>(o + dp.plane * F::LIMBS, o_eq);
  }
}

// pair blockIdx.y; LT_ONLY: the lt plane alone (w <= 2)
template <class F, int VEC, bool LT_ONLY>
__global__ __launch_bounds__(BLOCK) void k_cmp_first(typename F::Ctx ctx, u64* d, Planes dp, const u64* cmod, const u64* bits, Planes bp, const u64* r2,
                                                     Planes rp, int w, size_t rows, size_t N) {
  const int j = blockIdx.y;
  const bool has_hi = 2 * j + 1 < w;
  d += (size_t)(2 * j) * dp.plane * F::LIMBS;
  bits += (size_t)(2 * j) * bp.plane * F::LIMBS;
  r2 += (size_t)(2 * j) * rp.plane * F::LIMBS;
  for_each_pack<VEC>(N, [&](auto pw, size_t i) { first_at<F, pw, LT_ONLY>(ctx, d, dp, cmod, bits, bp, r2, rp, j, has_hi, rows, i); });
}

// lo, hi: the lt plane of node 2j and of node 2j + 1 in this row (the eq plane one plane on); o, rr likewise for the output node
template <class F, int W>
__device__ __forceinline__ void level_at(const typename F::Ctx& ctx, u64* o, size_t o_plane, const u64* lo, const u64* hi, size_t n_plane,
                                         const u64* rr, size_t r_plane, bool has_hi, bool lt_only, size_t i) {
  const Pack<F, W> lt_lo = load_pack<F, W, true>(lo + i * F::LIMBS), rl = load_pack<F, W, true>(rr + i * F::LIMBS);
  Pack<F, W> eq_lo, lt_hi, eq_hi, re, o_lt, o_eq;
  if (!lt_only) {
    eq_lo = load_pack<F, W, true>(lo + (n_plane + i) * F::LIMBS);
    re = load_pack<F, W, true>(rr + (r_plane + i) * F::LIMBS);
  }
  if (has_hi) {
    lt_hi = load_pack<F, W, true>(hi + i * F::LIMBS);
    eq_hi = load_pack<F, W, true>(hi + (n_plane + i) * F::LIMBS);
  } else {  // no partner: the identity
#pragma unroll
    for (int v = 0; v < W; ++v) {
      lt_hi.v[v] = F::zero();
      eq_hi.v[v] = F::one(ctx);
    }
  }
#pragma unroll
  for (int v = 0; v < W; ++v) {
    o_lt.v[v] = cmp_combine_lt<F>(ctx, lt_hi.v[v], eq_hi.v[v], lt_lo.v[v], rl.v[v]);
    if (!lt_only) o_eq.v[v] = cmp_combine_eq<F>(ctx, eq_hi.v[v], eq_lo.v[v], re.v[v]);
  }
  store_pack<F, W, true>(o + i * F::LIMBS, o_lt);
  if (!lt_only) store_pack<F, W, true>(o + (o_plane + i) * F::LIMBS, o_eq);
}

// row blockIdx.y, output node blockIdx.z
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_cmp_level(typename F::Ctx ctx, u64* d, Planes dp, const u64* nodes, Planes np, const u64* r2, Planes rp,
                                                     int cnt, bool lt_only, size_t N) {
  const size_t j = blockIdx.z, r = blockIdx.y;
  const bool has_hi = 2 * j + 1 < (size_t)cnt;
  u64* o = d + (2 * j * dp.plane + r * dp.row) * F::LIMBS;
  const u64* lo = nodes + (4 * j * np.plane + r * np.row) * F::LIMBS;
  const u64* hi = lo + 2 * np.plane * F::LIMBS;
  const u64* rr = r2 + (2 * j * rp.plane + r * rp.row) * F::LIMBS;
  for_each_pack<VEC>(N, [&](auto pw, size_t i) { level_at<F, pw>(ctx, o, dp.plane, lo, hi, np.plane, rr, rp.plane, has_hi, lt_only, i); });
}

// a lane reads its elements before it writes them, so out may be x, rlow or lt
template <class F, int W>
__device__ __forceinline__ void finish_at(const typename F::Ctx& ctx, const CmpFinish<F>& prm, u64* out, size_t out_stride, const u64* lt, size_t lt_stride,
                                          const u64* cmod, const unsigned char* status, const u64* rlow, size_t rlow_stride, const u64* x,
                                          size_t x_stride, size_t rows, size_t i) {
  const Pack<F, W> cm = load_pack<F, W, true>(cmod + i * F::LIMBS);
  int st[W];
#pragma unroll
  for (int v = 0; v < W; ++v) st[v] = status[i + v];
#pragma unroll 1
  for (size_t r = 0; r < rows; ++r) {
    const Pack<F, W> lv = load_pack<F, W, true>(lt + (r * lt_stride + i) * F::LIMBS), rv = load_pack<F, W, true>(rlow + (r * rlow_stride + i) * F::LIMBS);
    Pack<F, W> xv, o;
    if (prm.what != CMP_MOD) xv = load_pack<F, W, true>(x + (r * x_stride + i) * F::LIMBS);
    else xv = cm;  // (not looked at)
#pragma unroll
    for (int v = 0; v < W; ++v) o.v[v] = cmp_finish_one<F>(ctx, prm, cm.v[v], st[v], lv.v[v], rv.v[v], xv.v[v]);
    store_pack<F, W, true>(out + (r * out_stride + i) * F::LIMBS, o);
  }
}

template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_cmp_finish(typename F::Ctx ctx, CmpFinish<F> prm, u64* out, size_t out_stride, const u64* lt, size_t lt_stride,
                                                      const u64* cmod, const unsigned char* status, const u64* rlow, size_t rlow_stride,
                                                      const u64* x, size_t x_stride, size_t rows, size_t N) {
  for_each_pack<VEC>(N, [&](auto pw, size_t i) {
    finish_at<F, pw>(ctx, prm, out, out_stride, lt, lt_stride, cmod, status, rlow, rlow_stride, x, x_stride, rows, i);
  });
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#include "unit_host.hpp"

namespace {

// the tags this library refuses, each with its reason; SCL_OK for the five prime fields
int check_tag(const std::string& w, int field) {
  return check_prime_field(w, field, "GF(2^128) has no integers below a prime, there are no bits of an opened value to compare",
                           "a ring Z2k is not a field, it has no 2^-w and no Shamir sharing");
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

// `count` planes of rows x N as one operand (`extent`): the elements from plane 0 of row 0 to the end of the last plane of the last row
int check_planes(const std::string& w, const char* name, const char* plane_name, size_t plane_stride, const char* row_name, size_t row_stride,
                 size_t count, size_t rows, size_t N, size_t* extent) {
  if (plane_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": " + plane_name + " < N");
  if (row_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": " + row_name + " < N");
  if (!extent_of({{count, plane_stride}, {rows, row_stride}}, N, extent)) return fail(SCL_ERR_BAD_ARG, w + ": the extent of " + name + " overflows");
  return SCL_OK;
}

int check_flags(const std::string& w, unsigned flags, size_t out_nodes, const char* when) {
  if (flags & ~SCL_CMP_LT_ONLY) return fail(SCL_ERR_BAD_ARG, w + ": unknown flag");
  if ((flags & SCL_CMP_LT_ONLY) && out_nodes != 1)
    return fail(SCL_ERR_BAD_ARG, w + ": SCL_CMP_LT_ONLY is for the level that leaves a single node (" + when + ")");
  return SCL_OK;
}

}  // namespace

extern "C" {

int scl_cmp_abi_version(void) { return SCL_CMP_ABI_VERSION; }
const char* scl_cmp_last_error(void) { return g_err.c_str(); }

size_t scl_cmp_levels(size_t w) { return w ? cmp_levels(w) : 0; }
size_t scl_cmp_planes(size_t w) { return w ? cmp_planes(w) : 0; }

int scl_cmp_first_mask(int field, uint64_t* d_dev, size_t d_plane_stride, size_t d_row_stride, uint64_t* cmod_dev, unsigned char* status_dev,
                       const uint64_t* csh_dev, size_t c_stride, const uint64_t* lambda_host, size_t m, const uint64_t* bits_dev,
                       size_t bits_plane_stride, size_t bits_row_stride, const uint64_t* r2_dev, size_t r2_plane_stride, size_t r2_row_stride, size_t w_bits,
                       size_t B, size_t rows, size_t N, unsigned flags, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "first_mask";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L, top = max_bits(field, mont);
  if (w_bits == 0) return fail(SCL_ERR_BAD_ARG, w + ": w == 0: there are no bits to compare");
  if (w_bits >= B) return fail(SCL_ERR_BAD_ARG, w + ": w >= B: w is below k and k at most B");
  if (B > top) return fail(SCL_ERR_BAD_ARG, w + ": B > |p| - 2: B must be at most " + std::to_string(top) + " for this field (the opened value stays below p)");
  if (m == 0 || m > (size_t)OPEN_M_MAX)
    return fail(SCL_ERR_BAD_ARG, w + ": m must be in 1..64 (lambda travels with the launch); beyond that open with scl_hip_shamir_recover and pass m = 1, lambda = {1}");
  const size_t nodes = (w_bits + 1) / 2;
  if (const int rc = check_flags(w, flags, nodes, "w <= 2")) return rc;
  const bool lt_only = flags & SCL_CMP_LT_ONLY;
  const size_t out_planes = lt_only ? 1 : 2 * nodes;
  if (const int rc = check_ptr(w, L, "d_dev", d_dev)) return rc;
  if (const int rc = check_ptr(w, L, "cmod_dev", cmod_dev)) return rc;
  if (!status_dev) return fail(SCL_ERR_BAD_ARG, w + ": status_dev is NULL");
  if (const int rc = check_ptr(w, L, "csh_dev", csh_dev)) return rc;
  if (!lambda_host) return fail(SCL_ERR_BAD_ARG, w + ": lambda_host is NULL");
  if (const int rc = check_ptr(w, L, "bits_dev", bits_dev)) return rc;
  if (const int rc = check_ptr(w, L, "r2_dev", r2_dev)) return rc;
  if (c_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": c_stride < N");
  size_t d_ext = 0, b_ext = 0, r_ext = 0;
  if (const int rc = check_planes(w, "d_dev", "d_plane_stride", d_plane_stride, "d_row_stride", d_row_stride, out_planes, rows, N, &d_ext)) return rc;
  if (const int rc = check_planes(w, "bits_dev", "bits_plane_stride", bits_plane_stride, "bits_row_stride", bits_row_stride, w_bits, rows, N, &b_ext)) return rc;
  if (const int rc = check_planes(w, "r2_dev", "r2_plane_stride", r2_plane_stride, "r2_row_stride", r2_row_stride, out_planes, rows, N, &r_ext)) return rc;
  if (const int rc = alias_check("first_mask", {alias::vec("d_dev", d_dev, d_ext, esz, true), alias::vec("cmod_dev", cmod_dev, N, esz, true),
                                               alias::vec("status_dev", status_dev, N, 1, true), alias::mat("csh_dev", csh_dev, m, c_stride, N, esz, false),
                                               alias::vec("bits_dev", bits_dev, b_ext, esz, false), alias::vec("r2_dev", r2_dev, r_ext, esz, false)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!fx_has_trunc(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const FxFinish<F> prm = fx_make_finish<F>(ctx, (int)w_bits, (int)B);
      const bool two = two_per_lane(L, {d_dev, cmod_dev, bits_dev, r2_dev},
                                    {d_plane_stride, d_row_stride, bits_plane_stride, bits_row_stride, r2_plane_stride, r2_row_stride});
      const bool two_open = two_per_lane(L, {cmod_dev, csh_dev}, {m > 1 ? c_stride : 0});
      PACK_LAUNCH((k_cmp_open, F), two_open, dim3(grid_for_packs(two_open, N)), S(stream), ctx, prm, cmod_dev, status_dev, csh_dev, c_stride,
                  make_open_table<F>(lambda_host, m), (int)m, N);
      const dim3 grid(grid_for_packs(two, N), (unsigned)nodes);
      const Planes dp{d_plane_stride, d_row_stride}, bp{bits_plane_stride, bits_row_stride}, rp{r2_plane_stride, r2_row_stride};
      if (lt_only) PACK_LAUNCH((k_cmp_first, F, true), two, grid, S(stream), ctx, d_dev, dp, cmod_dev, bits_dev, bp, r2_dev, rp, (int)w_bits, rows, N);
      else PACK_LAUNCH((k_cmp_first, F, false), two, grid, S(stream), ctx, d_dev, dp, cmod_dev, bits_dev, bp, r2_dev, rp, (int)w_bits, rows, N);
      return SCL_OK;
    }
  });
}

int scl_cmp_level_mask(int field, uint64_t* d_dev, size_t d_plane_stride, size_t d_row_stride, const uint64_t* nodes_dev, size_t n_plane_stride,
                       size_t n_row_stride, const uint64_t* r2_dev, size_t r2_plane_stride, size_t r2_row_stride, size_t cnt, size_t rows, size_t N,
                       unsigned flags, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "level_mask";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L;
  if (cnt < 2) return fail(SCL_ERR_BAD_ARG, w + ": cnt < 2: a level combines at least two nodes");
  if (cnt > 256) return fail(SCL_ERR_BAD_ARG, w + ": cnt > 256: no field here has that many bits");
  const size_t nodes = (cnt + 1) / 2;
  if (const int rc = check_flags(w, flags, nodes, "cnt == 2")) return rc;
  const bool lt_only = flags & SCL_CMP_LT_ONLY;
  const size_t out_planes = lt_only ? 1 : 2 * nodes;
  if (const int rc = check_ptr(w, L, "d_dev", d_dev)) return rc;
  if (const int rc = check_ptr(w, L, "nodes_dev", nodes_dev)) return rc;
  if (const int rc = check_ptr(w, L, "r2_dev", r2_dev)) return rc;
  size_t d_ext = 0, n_ext = 0, r_ext = 0;
  if (const int rc = check_planes(w, "d_dev", "d_plane_stride", d_plane_stride, "d_row_stride", d_row_stride, out_planes, rows, N, &d_ext)) return rc;
  if (const int rc = check_planes(w, "nodes_dev", "n_plane_stride", n_plane_stride, "n_row_stride", n_row_stride, 2 * cnt, rows, N, &n_ext)) return rc;
  if (const int rc = check_planes(w, "r2_dev", "r2_plane_stride", r2_plane_stride, "r2_row_stride", r2_row_stride, out_planes, rows, N, &r_ext)) return rc;
  if (const int rc = alias_check("level_mask", {alias::vec("d_dev", d_dev, d_ext, esz, true), alias::vec("nodes_dev", nodes_dev, n_ext, esz, false),
                                               alias::vec("r2_dev", r2_dev, r_ext, esz, false)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!fx_has_trunc(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const bool two = two_per_lane(L, {d_dev, nodes_dev, r2_dev}, {d_plane_stride, d_row_stride, n_plane_stride, n_row_stride, r2_plane_stride, r2_row_stride});
      for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
        const size_t nr = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
        uint64_t* d = d_dev + r0 * d_row_stride * L;
        const uint64_t *nd = nodes_dev + r0 * n_row_stride * L, *r2 = r2_dev + r0 * r2_row_stride * L;
        PACK_LAUNCH((k_cmp_level, F), two, dim3(grid_for_packs(two, N), (unsigned)nr, (unsigned)nodes), S(stream), ctx, d, Planes{d_plane_stride, d_row_stride},
                    nd, Planes{n_plane_stride, n_row_stride}, r2, Planes{r2_plane_stride, r2_row_stride}, (int)cnt, lt_only, N);
      }
      return SCL_OK;
    }
  });
}

int scl_cmp_finish(int field, uint64_t* out_dev, size_t out_stride, const uint64_t* lt_dev, size_t lt_stride, const uint64_t* cmod_dev,
                   const unsigned char* status_dev, const uint64_t* rlow_dev, size_t rlow_stride, const uint64_t* x_dev, size_t x_stride, size_t w_bits,
                   int what, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  const std::string w = "finish";
  if (const int rc = check_tag(w, field)) return rc;
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field), esz = 8 * L, top = max_bits(field, mont);
  if (w_bits == 0) return fail(SCL_ERR_BAD_ARG, w + ": w == 0: there are no bits to compare");
  if (w_bits >= top) return fail(SCL_ERR_BAD_ARG, w + ": w >= |p| - 2: w is below B and B at most " + std::to_string(top) + " for this field");
  if (what != SCL_CMP_MOD && what != SCL_CMP_TRUNC && what != SCL_CMP_LTZ)
    return fail(SCL_ERR_BAD_ARG, w + ": unknown `what`: SCL_CMP_MOD, SCL_CMP_TRUNC or SCL_CMP_LTZ");
  const bool need_x = what != SCL_CMP_MOD;
  if (const int rc = check_ptr(w, L, "out_dev", out_dev)) return rc;
  if (const int rc = check_ptr(w, L, "lt_dev", lt_dev)) return rc;
  if (const int rc = check_ptr(w, L, "cmod_dev", cmod_dev)) return rc;
  if (!status_dev) return fail(SCL_ERR_BAD_ARG, w + ": status_dev is NULL");
  if (const int rc = check_ptr(w, L, "rlow_dev", rlow_dev)) return rc;
  if (need_x) {
    if (const int rc = check_ptr(w, L, "x_dev", x_dev)) return rc;
  }
  if (out_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": out_stride < N");
  if (lt_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": lt_stride < N");
  if (rlow_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": rlow_stride < N");
  if (need_x && x_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": x_stride < N");
  const uint64_t* xp = need_x ? x_dev : nullptr;  // (a NULL operand covers nothing)
  if (const int rc = alias_check("finish", {alias::mat("out_dev", out_dev, rows, out_stride, N, esz, true, 1), alias::mat("x_dev", xp, rows, x_stride, N, esz, false, 1),
                                           alias::mat("rlow_dev", rlow_dev, rows, rlow_stride, N, esz, false, 1),
                                           alias::mat("lt_dev", lt_dev, rows, lt_stride, N, esz, false, 1), alias::vec("cmod_dev", cmod_dev, N, esz, false),
                                           alias::vec("status_dev", status_dev, N, 1, false)}))
    return rc;
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if constexpr (!fx_has_trunc(F::TAG)) {
      return fail(SCL_ERR_BAD_ARG, w + ": internal tag");
    } else {
      if (const int rc = need_device()) return rc;
      const CmpFinish<F> prm = cmp_make_finish<F>(ctx, (int)w_bits, what);
      const bool two = two_per_lane(L, {out_dev, lt_dev, cmod_dev, rlow_dev, xp},
                                    {rows > 1 ? out_stride : 0, rows > 1 ? lt_stride : 0, rows > 1 ? rlow_stride : 0, rows > 1 && need_x ? x_stride : 0});
      PACK_LAUNCH((k_cmp_finish, F), two, dim3(grid_for_packs(two, N)), S(stream), ctx, prm, out_dev, out_stride, lt_dev, lt_stride, cmod_dev, status_dev,
                  rlow_dev, rlow_stride, xp, x_stride, rows, N);
      return SCL_OK;
    }
  });
}

}  // extern "C"
