// csrc/hm_unit.hip -- honest-majority (Damgard-Nielsen) multiplication: one dealer's double sharings in the reference's PRG
// order, the small matrix applied across sharings (the extraction with a hyper-invertible matrix) and the two local steps of a
// product; the kernels and the C ABI of libscl_hip_hm.so (include/scl_hip_hm.h), an extension library beside the engine.  One
// translation unit, all six fields.  The per-element arithmetic is include/scl_hip/detail/hm.hpp.
//
//   k_double_share_prg   one lane = one double sharing: r, then the degree-t and the degree-2t polynomial one after another (at
//                        most 2t + 1 <= 7 coefficients live), the parties in a rolled loop, Horner at the small node i + 1;
//                        one kernel per threshold 0..3, on the four-table AES of kernels.hpp as k_triples_shamir_prg
//                        (csrc/triples_unit.hip; the draws of both are csrc/prg_deal.hpp)
//   k_double_coeff_rows  the first of two passes: r and the 3t coefficient rows into the caller's scratch; the engine's
//                        explicit-coefficient scl_hip_shamir_share evaluates them (two calls)
//   k_hm_apply           one lane = one column (Mersenne61: two), R output rows in lazy accumulators, the n input rows walked
//                        once per row group; the tile of M staged in LDS once per workgroup as prepared constants (F::KC)
//   k_hm_apply_thin      the extraction's own shapes, n <= 16: a lane keeps the n inputs of its column in registers and walks the
//                        m rows of M (whole in LDS) with one accumulator: in read once, out written once
//   k_hm_mask            x y + r2, row blockIdx.y
//   k_hm_finish          sum_j lambda_j dsh[j] once per column, minus each row of r; lambda staged in LDS from kernel arguments
// The streaming kernels keep the conventions of csrc/unit_device.hpp: 256-lane blocks, 16-byte non-temporal accesses, the pack
// width of Mersenne61 chosen on the host per call, the odd last element taken by the lane after the last pair.  The engine is
// reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_hm.h"
#include "../../include/scl_hip/detail/hm.hpp"
#include "kernels.hpp"
#include "prg_deal.hpp"
#include "unit_device.hpp"

namespace sclhip {
namespace {

// ---- the dealer ------------------------------------------------------------------------------------------------------------
// Fused: double sharing s at blocks counter0 + s*B, B = BPE + Bs(T) + Bs(2T).  One kernel per threshold T, so that the
// coefficients stay in registers and Horner has no tests in it.  Fields with F::muladd_small_lazy on 16-bit nodes (the Mersenne
// fields, GF(2^128)).
template <class F, int T>
__global__ __launch_bounds__(ABLOCK) void k_double_share_prg(typename F::Ctx ctx, u64* lo_out, u64* hi_out, size_t stride, AesKey key,
                                                             u64 counter0, int n, size_t N) {
  SCL_AES4_PROLOGUE(key)
  constexpr int BPE = bpe<F>();
  constexpr u64 B1 = poly_blocks<F>(T), B = BPE + B1 + poly_blocks<F>(2 * T);
  SCL_AES4_GRID_STRIDE(s, N) {
    const u64 c0 = counter0 + s * B;
    const typename F::E r = draw_elem<F>(ctx, aes, key, c0);
    {
      typename F::E c[T + 1];
      c[0] = r;
      draw_poly<F, T>(ctx, aes, key, c0 + BPE, c);
      eval_rows<F, T>(ctx, c, lo_out + s * F::LIMBS, stride, n);
    }
    {
      typename F::E c[2 * T + 1];
      c[0] = r;
      draw_poly<F, 2 * T>(ctx, aes, key, c0 + BPE + B1, c);
      eval_rows<F, 2 * T>(ctx, c, hi_out + s * F::LIMBS, stride, n);
    }
  }
}

// Two-pass, first pass: row 0 of the scratch is r; rows 1..t are coefficients 1..t of the degree-t polynomial, rows t+1..3t
// coefficients 1..2t of the degree-2t polynomial.  Rows are N elements apart.
template <class F>
__global__ __launch_bounds__(ABLOCK) void k_double_coeff_rows(typename F::Ctx ctx, u64* rows, AesKey key, u64 counter0, int t, size_t N) {
  SCL_AES4_PROLOGUE(key)
  constexpr int BPE = bpe<F>();
  const u64 B1 = poly_blocks<F>((u64)t), B = BPE + B1 + poly_blocks<F>(2 * (u64)t);
  SCL_AES4_GRID_STRIDE(s, N) {
    const u64 c0 = counter0 + s * B;
    F::st(rows + s * F::LIMBS, draw_elem<F>(ctx, aes, key, c0));
#pragma unroll 1
    for (int m = 0; m < 2; ++m) {
      const int d = m ? 2 * t : t;
      const u64 p0 = c0 + BPE + (m ? B1 : 0);
      u64* base = rows + ((size_t)(1 + (m ? t : 0)) * N + s) * F::LIMBS;  // coefficient 1 of polynomial m
      if constexpr (F::LIMBS == 1) {
#pragma unroll 1
        for (int j = 0; 2 * j <= d; ++j) {  // block j = coefficients 2j (low 8 bytes) and 2j+1 (high 8 bytes)
          u64 lo, hi;
          aes.block(key, p0 + j, lo, hi);
          if (j > 0) base[(size_t)(2 * j - 1) * N] = F::from_le_word(ctx, lo);
          if (2 * j + 1 <= d) base[(size_t)(2 * j) * N] = F::from_le_word(ctx, hi);
        }
      } else {
#pragma unroll 1
        for (int k = 1; k <= d; ++k) {
          u64 lo[BPE], hi[BPE];
#pragma unroll
          for (int bb = 0; bb < BPE; ++bb) aes.block(key, p0 + (u64)k * BPE + bb, lo[bb], hi[bb]);
          F::st(base + (size_t)(k - 1) * N * F::LIMBS, elem_from_blocks<F>(ctx, lo, hi));
        }
      }
    }
  }
}

// ---- apply -----------------------------------------------------------------------------------------------------------------
// output rows a lane accumulates at once: what the registers hold without scratch (docs/kernels/hm.md has the figures)
template <class F>
constexpr int apply_rows() {
  return F::LIMBS == 4 ? 4 : 8;
}
// columns of M per LDS tile: the tile holds PREPARED constants (F::KC: 24 bytes for Mersenne61, 96 for Mersenne127, the element
// elsewhere) and stays at 8 to 12 KiB
template <class F>
constexpr int apply_tile_cols() {
  return F::TAG == M127::TAG ? 16 : 64;
}

// Rows [k0, k0 + R) of batch blockIdx.y, k0 = R * (g0 + blockIdx.z).  The tile of M is staged once per workgroup when n fits
// one tile, else once per tile and column block; rows past m are staged as zeros and not stored.
template <class F, int VEC, int R>
__global__ __launch_bounds__(BLOCK) void k_hm_apply(typename F::Ctx ctx, u64* out, size_t out_stride, size_t out_bstride, const u64* in,
                                                    size_t in_stride, size_t in_bstride, const u64* M, size_t ldm, size_t g0, size_t m,
                                                    int n, size_t N) {
  constexpr int APPLY_NC = apply_tile_cols<F>();
  __shared__ typename F::KC tile[R][APPLY_NC];
  const size_t k0 = (g0 + blockIdx.z) * R;
  out += ((size_t)blockIdx.y * out_bstride + k0 * out_stride) * F::LIMBS;
  in += (size_t)blockIdx.y * in_bstride * F::LIMBS;
  const size_t items = pack_items<VEC>(N);  // (the loop is the block's, not the lane's: every lane stages the tiles)
  const bool one_tile = n <= APPLY_NC;
  bool staged = false;
  for (size_t base = (size_t)blockIdx.x * BLOCK; base < items; base += (size_t)gridDim.x * BLOCK) {
    const size_t q = base + threadIdx.x;
    const bool active = q < items, pair = VEC == 2 && q < N / VEC;
    const size_t col = (VEC == 1 || pair) ? q * VEC : N - 1;  // the odd element after the last pair
    typename F::KAcc acc[R][VEC];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[r][v] = F::kacc_zero();
    int terms = 0;
    for (int i0 = 0; i0 < n; i0 += APPLY_NC) {
      const int nc = n - i0 < APPLY_NC ? n - i0 : APPLY_NC;
      if (!(one_tile && staged)) {  // (the same in every lane)
        __syncthreads();
        for (int e = threadIdx.x; e < R * nc; e += BLOCK) {
          const int r = e / nc, i = e % nc;
          tile[r][i] = F::kc_make(ctx, k0 + r < m ? F::ld(M + ((k0 + r) * ldm + i0 + i) * F::LIMBS) : F::zero());
        }
        __syncthreads();
        staged = true;
      }
      if (!active) continue;
#pragma unroll 1
      for (int i = 0; i < nc; ++i) {
        const u64* p = in + ((size_t)(i0 + i) * in_stride + col) * F::LIMBS;
        typename F::E x[VEC];
        if (VEC == 1 || pair) {
          const Pack<F, VEC> pk = load_pack<F, VEC, true>(p);
#pragma unroll
          for (int v = 0; v < VEC; ++v) x[v] = pk.v[v];
        } else {
          x[0] = load_pack<F, 1, true>(p).v[0];
#pragma unroll
          for (int v = 1; v < VEC; ++v) x[v] = F::zero();
        }
        if (terms + 1 > (int)F::K_TERMS) {  // one count for all accumulators: they fold together (hm_kmac_step, R x VEC wide)
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < VEC; ++v) hm_krefold<F>(ctx, acc[r][v]);
          terms = 1;
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int v = 0; v < VEC; ++v) F::kmac(ctx, acc[r][v], tile[r][i], x[v]);
        ++terms;
      }
    }
    if (!active) continue;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (k0 + r >= m) break;
      u64* o = out + ((size_t)r * out_stride + col) * F::LIMBS;
      if (VEC == 1 || pair) {
        Pack<F, VEC> pk;
#pragma unroll
        for (int v = 0; v < VEC; ++v) pk.v[v] = F::kacc_fold(ctx, acc[r][v]);
        store_pack<F, VEC, true>(o, pk);
      } else {
        Pack<F, 1> pk;
        pk.v[0] = F::kacc_fold(ctx, acc[r][0]);
        store_pack<F, 1, true>(o, pk);
      }
    }
  }
}

// A thin matrix (n <= KMAX <= 16 columns, m n elements within 16 KiB of LDS -- the extraction's own shapes): the n input elements
// of a column stay in registers, so `in` is read once and `out` written once whatever m is, (n + m) N elements in all; M sits
// in LDS whole and is read as broadcasts; every output is one sum of n <= 16 products on the matrix kernels' accumulator
// (kernels.hpp: MatAcc -- the field's Acc, column sums for Mersenne127), folded once.  KMAX is the next multiple of four.
constexpr int THIN_NMAX = 16;
constexpr int THIN_LDS_WORDS = 2048;  // 16 KiB of u64
static_assert(THIN_NMAX <= (int)M61::ACC_TERMS, "a thin row never folds on the way");

template <class F, int W, int KMAX>
__device__ __forceinline__ void thin_at(const typename F::Ctx& ctx, u64* out, size_t out_stride, const u64* in, size_t in_stride,
                                        const typename F::E* Ms, int m, int n, size_t col) {
  Pack<F, W> b[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < n) b[k] = load_pack<F, W, true>(in + ((size_t)k * in_stride + col) * F::LIMBS);
#pragma unroll 1
  for (int r = 0; r < m; ++r) {
    MatAcc<F> acc[W];
#pragma unroll
    for (int v = 0; v < W; ++v) acc[v].zero();
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < n) {
        const typename F::E a = Ms[r * n + k];
#pragma unroll
        for (int v = 0; v < W; ++v) acc[v].mac(ctx, a, b[k].v[v]);
      }
    }
    Pack<F, W> y;
#pragma unroll
    for (int v = 0; v < W; ++v) y.v[v] = acc[v].fold(ctx);
    store_pack<F, W, true>(out + ((size_t)r * out_stride + col) * F::LIMBS, y);
  }
}

template <class F, int VEC, int KMAX>
__global__ __launch_bounds__(BLOCK) void k_hm_apply_thin(typename F::Ctx ctx, u64* out, size_t out_stride, size_t out_bstride, const u64* in,
                                                         size_t in_stride, size_t in_bstride, const u64* M, size_t ldm, int m, int n, size_t N) {
  __shared__ typename F::E Ms[THIN_LDS_WORDS / F::LIMBS];
  for (int i = threadIdx.x; i < m * n; i += BLOCK) Ms[i] = F::ld(M + ((size_t)(i / n) * ldm + (i % n)) * F::LIMBS);
  __syncthreads();
  out += (size_t)blockIdx.y * out_bstride * F::LIMBS;
  in += (size_t)blockIdx.y * in_bstride * F::LIMBS;
  for_each_pack<VEC>(N, [&](auto w, size_t i) { thin_at<F, w, KMAX>(ctx, out, out_stride, in, in_stride, Ms, m, n, i); });
}

// ---- mask and finish -------------------------------------------------------------------------------------------------------
// d[i .. i + W) = x y + r2
template <class F, int W>
__device__ __forceinline__ void mask_at(const typename F::Ctx& ctx, u64* d, const u64* x, const u64* y, const u64* r2, size_t i) {
  const Pack<F, W> xv = load_pack<F, W, true>(x + i * F::LIMBS), yv = load_pack<F, W, true>(y + i * F::LIMBS),
                   rv = load_pack<F, W, true>(r2 + i * F::LIMBS);
  Pack<F, W> o;
#pragma unroll
  for (int v = 0; v < W; ++v) o.v[v] = hm_mask_one<F>(ctx, xv.v[v], yv.v[v], rv.v[v]);
  store_pack<F, W, true>(d + i * F::LIMBS, o);
}

// row blockIdx.y; a lane reads its elements before it writes them, so d may be r2
template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_hm_mask(typename F::Ctx ctx, u64* d, size_t d_stride, const u64* x, const u64* y, const u64* r2,
                                                   size_t op_stride, size_t N) {
  const size_t in_row = (size_t)blockIdx.y * op_stride * F::LIMBS;
  d += (size_t)blockIdx.y * d_stride * F::LIMBS;
  x += in_row;
  y += in_row;
  r2 += in_row;
  for_each_pack<VEC>(N, [&](auto w, size_t i) { mask_at<F, w>(ctx, d, x, y, r2, i); });
}

// z[r][i .. i + W) for every row r: the opened value once, each row's r read and its z written where it lies
template <class F, int W>
__device__ __forceinline__ void finish_at(const typename F::Ctx& ctx, u64* z, size_t z_stride, const u64* dsh, size_t d_stride,
                                          const typename F::E* lam, int m, const u64* rr, size_t r_stride, size_t rows, size_t i) {
  typename F::E opened[W];
  open_at<F, W>(ctx, dsh, d_stride, lam, m, i, opened);
#pragma unroll 1
  for (size_t r = 0; r < rows; ++r) {
    const Pack<F, W> rv = load_pack<F, W, true>(rr + (r * r_stride + i) * F::LIMBS);
    Pack<F, W> o;
#pragma unroll
    for (int v = 0; v < W; ++v) o.v[v] = hm_finish_one<F>(ctx, opened[v], rv.v[v]);
    store_pack<F, W, true>(z + (r * z_stride + i) * F::LIMBS, o);
  }
}

template <class F, int VEC>
__global__ __launch_bounds__(BLOCK) void k_hm_finish(typename F::Ctx ctx, u64* z, size_t z_stride, const u64* dsh, size_t d_stride,
                                                     OpenTable<F> tab, int m, const u64* rr, size_t r_stride, size_t rows, size_t N) {
  __shared__ typename F::E lam[OPEN_M_MAX];
  for (int j = threadIdx.x; j < m; j += BLOCK) lam[j] = tab.v[j];
  __syncthreads();
  for_each_pack<VEC>(N, [&](auto w, size_t i) { finish_at<F, w>(ctx, z, z_stride, dsh, d_stride, lam, m, rr, r_stride, rows, i); });
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#define SCL_UNIT_AES
#include "unit_host.hpp"

namespace {

constexpr size_t FUSED_TMAX = 3;        // the fused kernel keeps 2t + 1 <= 7 coefficients in registers

bool fused_double(int field, size_t t, unsigned flags) {
  return !(flags & SCL_HM_TWO_PASS) && t <= FUSED_TMAX && (field == SCL_M61 || field == SCL_M127 || field == SCL_GF2_128);
}
size_t deg_blocks(size_t limbs, size_t d) { return ((d + 1) * 8 * limbs + 15) / 16; }
size_t double_blocks(size_t limbs, size_t t) { return bpe_of(limbs) + deg_blocks(limbs, t) + deg_blocks(limbs, 2 * t); }
bool double_nt_ok(size_t limbs, size_t n, size_t t) { return n <= PARTY_MAX && t <= deg_max(limbs) / 2 && n > 2 * t; }

constexpr size_t EXTENT_MAX = (size_t)1 << 60;  // elements a matrix may span: no extent below wraps
}  // namespace

extern "C" {

int scl_hm_abi_version(void) { return SCL_HM_ABI_VERSION; }
const char* scl_hm_last_error(void) { return g_err.c_str(); }

size_t scl_hm_double_blocks(int field, size_t n, size_t t) {
  const size_t L = limbs_of(field);
  return L && double_nt_ok(L, n, t) ? double_blocks(L, t) : 0;
}

size_t scl_hm_double_scratch_bytes(int field, size_t N, size_t n, size_t t, unsigned flags) {
  const size_t L = limbs_of(field);
  if (!L || !double_nt_ok(L, n, t) || (flags & ~SCL_HM_TWO_PASS) || fused_double(field, t, flags)) return 0;
  const size_t per = (1 + 3 * t) * 8 * L;
  return N > ((size_t)1 << 62) / per ? 0 : N * per;
}

int scl_hm_double_share_prg(int field, uint64_t* lo_dev, uint64_t* hi_dev, size_t stride, size_t N, size_t t, size_t n,
                            const unsigned char* seed_host, size_t seed_len, uint64_t counter0, uint64_t* scratch_dev, unsigned flags,
                            void* stream) {
  if (N == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  if (flags & ~SCL_HM_TWO_PASS) return fail(SCL_ERR_BAD_ARG, "double_share_prg: unknown flags bit (only bit 0, two-pass, is defined)");
  const size_t L = limbs_of(field);
  if (n > PARTY_MAX) return fail(SCL_ERR_BAD_ARG, "double_share_prg: n must be at most 65535");
  if (t > deg_max(L) / 2)
    return fail(SCL_ERR_BAD_ARG, "double_share_prg: the degree 2t must be at most " + std::to_string(deg_max(L)) +
                                     " for this field (beyond it the engine's share call synchronises the stream)");
  if (n <= 2 * t) return fail(SCL_ERR_BAD_ARG, "double_share_prg: n must be larger than 2t (a degree-2t sharing among n <= 2t parties cannot be opened)");
  if (!lo_dev || !hi_dev) return fail(SCL_ERR_BAD_ARG, "double_share_prg: NULL operand");
  if (const int rc = check_align("double_share_prg", L, {lo_dev, hi_dev})) return rc;
  if (stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "double_share_prg: stride < N");
  if (n > EXTENT_MAX / stride / L) return fail(SCL_ERR_BAD_ARG, "double_share_prg: n * stride overflows");
  const Span sl = span_of(lo_dev, n, stride, N, L), sh = span_of(hi_dev, n, stride, N, L);
  if (overlap(sl, sh)) return fail(SCL_ERR_BAD_ARG, "double_share_prg: the share matrices overlap");
  const uint64_t B = double_blocks(L, t);
  if (const int rc = check_counter_range("double_share_prg", counter0, N, B)) return rc;
  const bool fused = fused_double(field, t, flags);
  if (!fused) {
    const size_t need = scl_hm_double_scratch_bytes(field, N, n, t, flags);
    if (!need) return fail(SCL_ERR_BAD_ARG, "double_share_prg: (1 + 3t) * N overflows");
    if (!scratch_dev)
      return fail(SCL_ERR_BAD_ARG, "double_share_prg: this case takes the two-pass path and needs " + std::to_string(need) +
                                       " bytes of scratch (scl_hm_double_scratch_bytes); scratch_dev is NULL");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15) return fail(SCL_ERR_BAD_ARG, "double_share_prg: scratch pointer not 16-byte aligned");
    const Span ss = {scratch_dev, scratch_dev + need / 8};
    if (overlap(ss, sl) || overlap(ss, sh)) return fail(SCL_ERR_BAD_ARG, "double_share_prg: the scratch overlaps a share matrix");
  }
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    AesKey key;
    make_aes_key(seed_host, seed_len, key);
    aes_key_range(key, counter0, (u64)N * B);
    if constexpr (F::TAG == 0 || F::TAG == 1 || F::TAG == 3) {
      if (fused) {
#define DOUBLE_CASE(TT) \
  case TT: AES4_LAUNCH((k_double_share_prg<F, TT>), N, S(stream), ctx, lo_dev, hi_dev, stride, key, (u64)counter0, (int)n, N); break;
        switch (t) {
          DOUBLE_CASE(0) DOUBLE_CASE(1) DOUBLE_CASE(2) DOUBLE_CASE(3)
          default: return fail(SCL_ERR_BAD_ARG, "double_share_prg: internal threshold");
        }
#undef DOUBLE_CASE
        return SCL_OK;
      }
    }
    AES4_LAUNCH((k_double_coeff_rows<F>), N, S(stream), ctx, scratch_dev, key, (u64)counter0, (int)t, N);
    uint64_t* outs[2] = {lo_dev, hi_dev};
    for (size_t m = 0; m < 2; ++m) {
      const size_t d = m ? 2 * t : t;
      const uint64_t* coeffs = t ? scratch_dev + (1 + (m ? t : 0)) * N * F::LIMBS : nullptr;
      const int rc = scl_hip_shamir_share(field, outs[m], stride, scratch_dev, coeffs, t ? N : 0, N, d, n, nullptr, stream);
      if (rc != SCL_OK) return fail(rc, std::string("double_share_prg: scl_hip_shamir_share: ") + scl_hip_last_error());
    }
    return SCL_OK;
  });
}

int scl_hm_apply(int field, uint64_t* out_dev, size_t out_stride, size_t out_batch_stride, const uint64_t* in_dev, size_t in_stride,
                 size_t in_batch_stride, const uint64_t* M_dev, size_t ldm, size_t m, size_t n, size_t batch, size_t N, void* stream) {
  if (N == 0 || batch == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field);
  if (m == 0 || n == 0 || n > PARTY_MAX) return fail(SCL_ERR_BAD_ARG, "apply: m and n must be at least 1 and n at most 65535");
  if (!out_dev || !in_dev || !M_dev) return fail(SCL_ERR_BAD_ARG, "apply: NULL operand");
  if (const int rc = check_align("apply", L, {out_dev, in_dev, M_dev})) return rc;
  if (out_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "apply: out_stride < N");
  if (in_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "apply: in_stride < N");
  if (ldm < n) return fail(SCL_ERR_SIZE_MISMATCH, "apply: ldm < n");
  if (batch == 1) out_batch_stride = in_batch_stride = 0;
  if (m > EXTENT_MAX / out_stride / L || n > EXTENT_MAX / in_stride / L || m > EXTENT_MAX / ldm / L ||
      (batch > 1 && (batch > EXTENT_MAX / (out_batch_stride ? out_batch_stride : 1) / L || batch > EXTENT_MAX / (in_batch_stride ? in_batch_stride : 1) / L)))
    return fail(SCL_ERR_BAD_ARG, "apply: an extent overflows");
  // the words all batches cover, from the first word of batch 0 to the last of batch - 1
  const Span so = {out_dev, out_dev + ((batch - 1) * out_batch_stride + (m - 1) * out_stride + N) * L};
  const Span si = {in_dev, in_dev + ((batch - 1) * in_batch_stride + (n - 1) * in_stride + N) * L};
  if (overlap(so, si)) return fail(SCL_ERR_BAD_ARG, "apply: out overlaps in");
  if (overlap(so, span_of(M_dev, m, ldm, n, L))) return fail(SCL_ERR_BAD_ARG, "apply: out overlaps M");
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    constexpr int R = apply_rows<F>();
    const size_t groups = (m + R - 1) / R;
    const bool two = two_per_lane(L, {out_dev, in_dev}, {m > 1 ? out_stride : 0, n > 1 ? in_stride : 0, out_batch_stride, in_batch_stride});
    const bool thin = n <= (size_t)THIN_NMAX && m <= (size_t)THIN_LDS_WORDS / L / n;
    for (size_t b0 = 0; b0 < batch; b0 += GRID_Y_MAX) {
      const size_t nb = batch - b0 < GRID_Y_MAX ? batch - b0 : GRID_Y_MAX;
      uint64_t* o = out_dev + b0 * out_batch_stride * L;
      const uint64_t* in = in_dev + b0 * in_batch_stride * L;
      if (thin) {
#define THIN_CASE(KK)                                                                                                              \
  case KK:                                                                                                                         \
    PACK_LAUNCH((k_hm_apply_thin, F, KK), two, dim3(grid_for_packs(two, N), (unsigned)nb), S(stream), ctx, o, out_stride, out_batch_stride, in, \
                in_stride, in_batch_stride, M_dev, ldm, (int)m, (int)n, N);                                                         \
    break;
        switch ((n + 3) / 4 * 4) {
          THIN_CASE(4) THIN_CASE(8) THIN_CASE(12) THIN_CASE(16)
          default: return fail(SCL_ERR_BAD_ARG, "apply: internal width");
        }
#undef THIN_CASE
        continue;
      }
      for (size_t g0 = 0; g0 < groups; g0 += GRID_Y_MAX) {
        const size_t ng = groups - g0 < GRID_Y_MAX ? groups - g0 : GRID_Y_MAX;
        PACK_LAUNCH((k_hm_apply, F, R), two, dim3(grid_for_packs(two, N), (unsigned)nb, (unsigned)ng), S(stream), ctx, o, out_stride,
                    out_batch_stride, in, in_stride, in_batch_stride, M_dev, ldm, g0, m, (int)n, N);
      }
    }
    return SCL_OK;
  });
}

int scl_hm_mul_mask(int field, uint64_t* d_dev, size_t d_stride, const uint64_t* x_dev, const uint64_t* y_dev, const uint64_t* r2_dev,
                    size_t op_stride, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field);
  if (!d_dev || !x_dev || !y_dev || !r2_dev) return fail(SCL_ERR_BAD_ARG, "mul_mask: NULL operand");
  if (const int rc = check_align("mul_mask", L, {d_dev, x_dev, y_dev, r2_dev})) return rc;
  if (d_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "mul_mask: d_stride < N");
  if (op_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "mul_mask: op_stride < N");
  if (rows > EXTENT_MAX / (d_stride > op_stride ? d_stride : op_stride) / L) return fail(SCL_ERR_BAD_ARG, "mul_mask: rows * stride overflows");
  const Span out = span_of(d_dev, rows, d_stride, N, L);
  if (overlap(out, span_of(x_dev, rows, op_stride, N, L)) || overlap(out, span_of(y_dev, rows, op_stride, N, L)))
    return fail(SCL_ERR_BAD_ARG, "mul_mask: d overlaps x or y");
  if (!(d_dev == r2_dev && d_stride == op_stride) && overlap(out, span_of(r2_dev, rows, op_stride, N, L)))
    return fail(SCL_ERR_BAD_ARG, "mul_mask: d overlaps r2 (only d == r2 with d_stride == op_stride is allowed)");
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    const bool two = two_per_lane(L, {d_dev, x_dev, y_dev, r2_dev}, {rows > 1 ? d_stride : 0, rows > 1 ? op_stride : 0});
    for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
      const size_t r = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
      uint64_t* o = d_dev + r0 * d_stride * L;
      const size_t in0 = r0 * op_stride * L;
      PACK_LAUNCH((k_hm_mask, F), two, dim3(grid_for_packs(two, N), (unsigned)r), S(stream), ctx, o, d_stride, x_dev + in0, y_dev + in0,
                  r2_dev + in0, op_stride, N);
    }
    return SCL_OK;
  });
}

int scl_hm_mul_finish(int field, uint64_t* z_dev, size_t z_stride, const uint64_t* dsh_dev, size_t d_stride, const uint64_t* lambda_host,
                      size_t m, const uint64_t* r_dev, size_t r_stride, size_t rows, size_t N, void* stream) {
  if (N == 0 || rows == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const size_t L = limbs_of(field);
  if (m == 0 || m > (size_t)OPEN_M_MAX)
    return fail(SCL_ERR_BAD_ARG, "mul_finish: m must be in 1..64 (lambda travels with the launch); beyond that open with scl_hip_shamir_recover "
                                 "and subtract with scl_hip_ew");
  if (!z_dev || !dsh_dev || !lambda_host || !r_dev) return fail(SCL_ERR_BAD_ARG, "mul_finish: NULL operand");
  if (const int rc = check_align("mul_finish", L, {z_dev, dsh_dev, r_dev})) return rc;
  if (z_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "mul_finish: z_stride < N");
  if (d_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "mul_finish: d_stride < N");
  if (r_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "mul_finish: r_stride < N");
  if (rows > EXTENT_MAX / (z_stride > r_stride ? z_stride : r_stride) / L || m > EXTENT_MAX / d_stride / L)
    return fail(SCL_ERR_BAD_ARG, "mul_finish: rows * stride overflows");
  const Span out = span_of(z_dev, rows, z_stride, N, L);
  if (overlap(out, span_of(dsh_dev, m, d_stride, N, L))) return fail(SCL_ERR_BAD_ARG, "mul_finish: z overlaps dsh");
  if (!(z_dev == r_dev && z_stride == r_stride) && overlap(out, span_of(r_dev, rows, r_stride, N, L)))
    return fail(SCL_ERR_BAD_ARG, "mul_finish: z overlaps r (only z == r with z_stride == r_stride is allowed)");
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    const bool two = two_per_lane(L, {z_dev, dsh_dev, r_dev}, {rows > 1 ? z_stride : 0, rows > 1 ? r_stride : 0, m > 1 ? d_stride : 0});
    PACK_LAUNCH((k_hm_finish, F), two, dim3(grid_for_packs(two, N)), S(stream), ctx, z_dev, z_stride, dsh_dev, d_stride,
                make_open_table<F>(lambda_host, m), (int)m, r_dev, r_stride, rows, N);
    return SCL_OK;
  });
}

}  // extern "C"
