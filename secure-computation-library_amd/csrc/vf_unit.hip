// csrc/vf_unit.hip -- batch verification: random linear combinations of sharings along N,
//   out[r][j] = sum_s rho_j[s] x[r][s] (y[r][s]);
// the kernels and the C ABI of libscl_hip_vf.so (include/scl_hip_vf.h), an extension library beside the engine.  One translation
// unit, all six fields.  The per-element arithmetic and the launch geometry are include/scl_hip/detail/vf.hpp, on the matrix
// kernels' accumulator (kernels.hpp: MatAcc -- the field's Acc, column sums for Mersenne127).
//
//   k_vf_combine_prg    the fused form: 1024-lane workgroups on kernels.hpp's four-table AES, one per CU.  A lane draws the
//                       coefficients of its packs from the AES-CTR stream in registers, in k_vector_random's block-to-element
//                       order, and uses them for the R rows of group blockIdx.y.
//   k_vf_combine_rows   the streaming form: 256-lane workgroups, the coefficients loaded from rows.
//   k_vf_finish         one workgroup per (row, repetition): the sum of the per-workgroup partial sums.
// The first two share one body: per trip a lane obtains reps x U coefficient packs, then for each row of the group issues the U
// loads of x (and y) before the first product is consumed and takes the terms into R x reps accumulators; a lane folds at the end
// of its trips, the workgroup reduces with wavefront shuffles and one LDS slot per wave, and one lane per value stores the
// partial.  No atomics, no counters in memory.  Every load is non-temporal: every byte is touched once.  A column past N is a
// zero of x: its term counts and adds nothing.
// The engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/scl_hip_vf.h"
#include "../../include/scl_hip/detail/vf.hpp"
#include "kernels.hpp"

namespace sclhip {
namespace {

template <class F>
constexpr int pack_w() {
  return F::LIMBS == 1 ? 2 : 1;
}

// fn(integral_constant<int, I>) for I0 <= I < I1, each call its own instantiation
template <int I0, int I1, class Fn>
__device__ __forceinline__ void static_for(Fn&& fn) {
  if constexpr (I0 < I1) {
    fn(std::integral_constant<int, I0>{});
    static_for<I0 + 1, I1>(fn);
  }
}

// pack q of a row: the columns from q * W on, zeros past N.  AL: a Mersenne61 pair in one 16-byte access.
template <class F, bool AL>
__device__ __forceinline__ Pack<F, pack_w<F>()> load_cols(const u64* row, size_t q, size_t N) {
  Pack<F, pack_w<F>()> r;
  if constexpr (F::LIMBS == 1) {
    const size_t c = 2 * q;
    r.v[0] = r.v[1] = 0;
    if (c + 1 < N) {
      if constexpr (AL) {
        r = load_pack<F, 2, true>(row + c);
      } else {
        r.v[0] = ldg<true>(row + c);
        r.v[1] = ldg<true>(row + c + 1);
      }
    } else if (c < N) {
      r.v[0] = ldg<true>(row + c);  // the odd last column
    }
  } else {
    if (q < N) r = load_pack<F, 1, true>(row + q * F::LIMBS);
    else r.v[0] = F::zero();
  }
  return r;
}

// the coefficients of packs q0 + u * Gt, u < U, for REPS repetitions: rows of rho_j ...
template <class F, bool AL>
struct CoeffRows {
  const u64* rho;
  size_t stride;  // in limbs
  template <int REPS, int U>
  __device__ __forceinline__ void get(size_t q0, size_t Gt, size_t N, Pack<F, pack_w<F>()> (&c)[REPS][U]) const {
#pragma unroll
    for (int j = 0; j < REPS; ++j)
#pragma unroll
      for (int u = 0; u < U; ++u) c[j][u] = load_cols<F, AL>(rho + (size_t)j * stride, q0 + (size_t)u * Gt, N);
  }
};

// ... or the AES-CTR stream: repetition j is Vector::random(N) at block counter0 + j B, and pack q of a Mersenne61 vector is
// block q (the low and the high 8 bytes), element q of a 16-byte field block q, of a 32-byte field blocks 2q and 2q + 1
// (k_vector_random).  Packs past N draw blocks past the vector's: they meet zeros of x.  (The dealers' order, one secret's
// polynomials after another, is another one: csrc/prg_deal.hpp.)
template <class F>
struct CoeffPrg {
  const typename F::Ctx& ctx;
  const Aes4& aes;
  const AesKey& key;
  u64 counter0, B;
  template <int REPS, int U>
  __device__ __forceinline__ void get(size_t q0, size_t Gt, size_t, Pack<F, pack_w<F>()> (&c)[REPS][U]) const {
#pragma unroll
    for (int j = 0; j < REPS; ++j) {
      const u64 base = counter0 + (u64)j * B;
      if constexpr (F::LIMBS == 4) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          u64 ctr[2], lo[2], hi[2];
          ctr[0] = base + 2 * (q0 + (size_t)u * Gt);
          ctr[1] = ctr[0] + 1;
          aes4_blocks<2>(aes, key, ctr, lo, hi);
          c[j][u].v[0] = elem_from_blocks<F>(ctx, lo, hi);
        }
      } else {
        // two blocks abreast: left alone the compiler runs all REPS * U draws abreast and runs out of the 128 registers a
        // 1024-lane workgroup has (as csrc/prg_deal.hpp's draw_poly).  The empty statement makes the next pair's counters wait
        // for this pair's result.
        constexpr int NB = U < 2 ? U : 2;
#pragma unroll
        for (int u0 = 0; u0 < U; u0 += NB) {
          u64 ctr[NB], lo[NB], hi[NB];
#pragma unroll
          for (int b = 0; b < NB; ++b) ctr[b] = base + q0 + (size_t)(u0 + b) * Gt;
          aes4_blocks<NB>(aes, key, ctr, lo, hi);
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            if constexpr (F::LIMBS == 1) {
              c[j][u0 + b].v[0] = F::from_le_word(ctx, lo[b]);
              c[j][u0 + b].v[1] = F::from_le_word(ctx, hi[b]);
            } else {
              c[j][u0 + b].v[0] = elem_from_blocks<F>(ctx, lo + b, hi + b);
            }
          }
#if defined(__HIP_DEVICE_COMPILE__)
          asm volatile("" : "+v"(q0) : "v"((u32)lo[0]));
#endif
        }
      }
    }
  }
};

// The workgroup's K values, one per lane each, summed: wavefront shuffles, one LDS slot per wave and value, then lane k adds the
// slots of value k and stores it where k < nvalid.  `lds` holds K * THREADS / 64 elements.  Value k = r * REPS + j goes to
// part + (r * reps_all + j) * G elements: the call's reps_all repetitions of a row lie together, this launch's REPS among them.
template <class F, int THREADS, int K, int REPS>
__device__ __forceinline__ void reduce_store(const typename F::Ctx& ctx, typename F::E (&v)[K], typename F::E* lds, u64* part, size_t G, size_t reps_all,
                                             int nvalid) {
  constexpr int NW = THREADS / 64;
  static_assert(K <= 64, "one lane of the first wave per value");
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v[k] = F::add(ctx, v[k], shfl_xor_elem<F>(v[k], m));
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[k * NW + (threadIdx.x >> 6)] = v[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < nvalid) {
    const int k = threadIdx.x;
    typename F::E tot = lds[k * NW];
    for (int w = 1; w < NW; ++w) tot = F::add(ctx, tot, lds[k * NW + w]);
    F::st(part + ((size_t)(k / REPS) * reps_all + k % REPS) * G * F::LIMBS, tot);
  }
}

// Rows [blockIdx.y * R, .. + R) of x (and y), the packs of workgroup blockIdx.x: partial (r, j) of workgroup b at
// part + ((r * reps_all + j) * G + b) elements, G = gridDim.x.
template <class F, bool AL, int R, int REPS, int U, bool PROD, int THREADS, class Coeff>
__device__ __forceinline__ void combine_body(const typename F::Ctx& ctx, u64* part, const u64* x, const u64* y, size_t op_stride, size_t rows, size_t N,
                                             size_t reps_all, const Coeff& cf, typename F::E* lds) {
  constexpr int W = pack_w<F>();
  const size_t r0 = (size_t)blockIdx.y * R;
  const int nr = rows - r0 < (size_t)R ? (int)(rows - r0) : R;
  x += r0 * op_stride * F::LIMBS;
  if (PROD) y += r0 * op_stride * F::LIMBS;
  MatAcc<F> acc[R * REPS];
  int terms[R];  // one count per row: the REPS accumulators of a row take their terms together
#pragma unroll
  for (int k = 0; k < R * REPS; ++k) acc[k].zero();
#pragma unroll
  for (int r = 0; r < R; ++r) terms[r] = 0;
  const size_t items = N / W + (N % W != 0), Gt = (size_t)gridDim.x * THREADS, rstep = op_stride * F::LIMBS;
  for (size_t q0 = (size_t)blockIdx.x * THREADS + threadIdx.x; q0 < items; q0 += (size_t)U * Gt) {
    Pack<F, W> c[REPS][U];
    cf.template get<REPS, U>(q0, Gt, N, c);
    const u64 *xr = x, *yr = y;  // the row's base, stepped row by row (R uniform offsets cost the AES form its scalar registers)
    // rows and trips are unrolled by instantiation, not by the optimiser: the accumulators are registers whatever the
    // body's size (a `#pragma unroll` the optimiser declines puts them, and the packs, into scratch memory)
    static_for<0, R>([&](auto rc) __attribute__((always_inline)) {
      constexpr int r = decltype(rc)::value;
      if (r < nr) {  // (uniform)
        Pack<F, W> xv[U], yv[U];
        static_for<0, U>([&](auto uc) __attribute__((always_inline)) {  // the loads of the trip before the first product is consumed
          constexpr int u = decltype(uc)::value;
          xv[u] = load_cols<F, AL>(xr, q0 + (size_t)u * Gt, N);
          if constexpr (PROD) yv[u] = load_cols<F, AL>(yr, q0 + (size_t)u * Gt, N);
        });
        static_for<0, U * W>([&](auto tc) __attribute__((always_inline)) {
          constexpr int u = decltype(tc)::value / W, v = decltype(tc)::value % W;
          typename F::E cv[REPS];
#pragma unroll
          for (int j = 0; j < REPS; ++j) cv[j] = c[j][u].v[v];
          vf_take<F, REPS, PROD>(ctx, acc + r * REPS, terms[r], cv, xv[u].v[v], PROD ? yv[u].v[v] : xv[u].v[v]);
        });
      }
      xr += rstep;
      if (PROD) yr += rstep;
    });
  }
  typename F::E v[R * REPS];
#pragma unroll
  for (int k = 0; k < R * REPS; ++k) v[k] = acc[k].fold(ctx);
  reduce_store<F, THREADS, R * REPS, REPS>(ctx, v, lds, part + (r0 * reps_all * gridDim.x + blockIdx.x) * F::LIMBS, gridDim.x, reps_all, nr * REPS);
}

template <class F, bool AL, int REPS, bool PROD>
__global__ __launch_bounds__(BLOCK) void k_vf_combine_rows(typename F::Ctx ctx, u64* part, const u64* x, const u64* y, size_t op_stride,
                                                           const u64* rho, size_t rho_stride, size_t rows, size_t N, size_t reps_all) {
  constexpr int R = vf_rows_per_group(F::LIMBS, false, REPS);
  __shared__ typename F::E red[R * REPS * (BLOCK / 64)];
  const CoeffRows<F, AL> cf{rho, rho_stride * F::LIMBS};
  combine_body<F, AL, R, REPS, vf_unroll(F::LIMBS, false, REPS), PROD, BLOCK>(ctx, part, x, y, op_stride, rows, N, reps_all, cf, red);
}

template <class F, bool AL, int REPS, bool PROD>
__global__ __launch_bounds__(ABLOCK) void k_vf_combine_prg(typename F::Ctx ctx, u64* part, const u64* x, const u64* y, size_t op_stride, AesKey key,
                                                           u64 counter0, u64 B, size_t rows, size_t N, size_t reps_all) {
  constexpr int R = vf_rows_per_group(F::LIMBS, true, REPS);
  static_assert(R * REPS * (ABLOCK / 64) * sizeof(typename F::E) <= AES4_EXTRA_BYTES, "the reduction's slots lie above the AES tables");
  SCL_AES4_PROLOGUE(key)
  const CoeffPrg<F> cf{ctx, aes, key, counter0, B};
  combine_body<F, AL, R, REPS, vf_unroll(F::LIMBS, true, REPS), PROD, ABLOCK>(ctx, part, x, y, op_stride, rows, N, reps_all, cf, reinterpret_cast<typename F::E*>(aes4_extra));
}

// value k0 + blockIdx.x = r * reps + j: the sum of its G partials, to out[r][j]
template <class F>
__global__ __launch_bounds__(BLOCK) void k_vf_finish(typename F::Ctx ctx, u64* out, size_t out_stride, const u64* part, size_t G, size_t k0, size_t reps) {
  const size_t k = k0 + blockIdx.x;
  MatAcc<F> acc;
  acc.zero();
  int terms = 0;
  for (size_t g = threadIdx.x; g < G; g += BLOCK) vf_take_partial<F>(ctx, acc, terms, load_pack<F, 1, true>(part + (k * G + g) * F::LIMBS).v[0]);
  const typename F::E tot = block_reduce_add<F>(ctx, acc.fold(ctx));
  if (threadIdx.x == 0) F::st(out + ((k / reps) * out_stride + k % reps) * F::LIMBS, tot);
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#define SCL_UNIT_AES
#include "unit_host.hpp"

namespace {

static_assert(VF_THREADS_STREAM == BLOCK && VF_THREADS_AES == ABLOCK && VF_GRID_AES == AES4_GRID_CAP, "vf.hpp restates the launch constants of kernels.hpp");

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }
// columns between the coefficient rows of the two-pass path: a Mersenne61 row starts 16-byte aligned
size_t rho_pitch(size_t limbs, size_t N) { return limbs == 1 ? N + (N & 1) : N; }

// bytes of the partial sums; false on overflow
bool partial_bytes(size_t L, bool aes, size_t rows, size_t reps, size_t N, size_t* out) {
  size_t b = 0;
  if (__builtin_mul_overflow(rows, reps, &b) || __builtin_mul_overflow(b, vf_groups(L, aes, reps, N), &b) || __builtin_mul_overflow(b, 8 * L, &b) ||
      b > ((size_t)1 << 62))
    return false;
  *out = round16(b);
  return true;
}

// which instantiation: the kernel for (AL, REPS, PROD) through a generic lambda that takes them as integral constants
template <class Fn>
int with_shape(bool al, size_t reps, bool prod, Fn&& fn) {
#define VF_SHAPE(A, RP)                                                                            \
  if (al == A && reps == RP)                                                                       \
    return prod ? fn(std::integral_constant<bool, A>{}, std::integral_constant<int, RP>{}, std::true_type{}) \
                : fn(std::integral_constant<bool, A>{}, std::integral_constant<int, RP>{}, std::false_type{});
  VF_SHAPE(true, 1) VF_SHAPE(true, 2) VF_SHAPE(true, 3) VF_SHAPE(true, 4)
  VF_SHAPE(false, 1) VF_SHAPE(false, 2) VF_SHAPE(false, 3) VF_SHAPE(false, 4)
#undef VF_SHAPE
  return fail(SCL_ERR_BAD_ARG, "combine: internal shape");
}

// The shared tail of both entry points.  rho_dev == nullptr: the coin from the PRG (fused, or rows filled in scratch first).
int combine_common(const char* who, bool prg, int field, uint64_t* out_dev, size_t out_stride, const uint64_t* x_dev, const uint64_t* y_dev,
                   size_t op_stride, const uint64_t* rho_dev, size_t rho_stride, size_t rows, size_t N, size_t reps, const unsigned char* seed_host,
                   size_t seed_len, uint64_t counter0, uint64_t* scratch_dev, size_t scratch_bytes, void* stream) {
  if (rows == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  const std::string w = who;
  const size_t L = limbs_of(field), esz = 8 * L;
  if (reps == 0 || reps > VF_REPS_MAX) return fail(SCL_ERR_BAD_ARG, w + ": reps must be at least 1 and at most 4");
  if (!out_dev) return fail(SCL_ERR_BAD_ARG, w + ": out_dev is NULL");
  if (!scratch_dev) return fail(SCL_ERR_BAD_ARG, w + ": scratch_dev is NULL");
  if (N && !x_dev) return fail(SCL_ERR_BAD_ARG, w + ": x_dev is NULL (only y_dev may be NULL: the plain form)");
  if (N && !prg && !rho_dev) return fail(SCL_ERR_BAD_ARG, w + ": rho_dev is NULL");
  if (prg && !seed_host && seed_len) return fail(SCL_ERR_BAD_ARG, w + ": seed_host is NULL");
  const uintptr_t mask = L == 1 ? 7 : 15;
  const struct { const char* name; const void* p; } ptrs[4] = {{"out_dev", out_dev}, {"x_dev", x_dev}, {"y_dev", y_dev}, {"rho_dev", rho_dev}};
  for (const auto& q : ptrs)
    if (reinterpret_cast<uintptr_t>(q.p) & mask)
      return fail(SCL_ERR_BAD_ARG, w + ": " + q.name + (L == 1 ? " not 8-byte aligned" : " not 16-byte aligned"));
  if (reinterpret_cast<uintptr_t>(scratch_dev) & 15) return fail(SCL_ERR_BAD_ARG, w + ": scratch_dev not 16-byte aligned");
  if (out_stride < reps) return fail(SCL_ERR_SIZE_MISMATCH, w + ": out_stride < reps");
  if (op_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": op_stride < N");
  if (!prg && rho_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": rho_stride < N");
  const bool fused = prg && vf_fused(field);
  uint64_t B = 0;
  if (prg) {  // reps * B blocks from counter0 (and the slack aes_key_range adds) must not wrap the 64-bit counter
    B = scl_vf_coin_blocks(field, N);
    const uint64_t room = ~(uint64_t)0 - 128;
    if (counter0 > room || (B && reps > (room - counter0) / B)) return fail(SCL_ERR_BAD_ARG, w + ": counter0 + reps * B wraps the 64-bit counter");
  }
  const size_t need = scl_vf_scratch_bytes(field, rows, reps, N, prg ? SCL_VF_PRG : 0);
  size_t pbytes = 0;
  if (!need || !partial_bytes(L, fused, rows, reps, N, &pbytes)) return fail(SCL_ERR_BAD_ARG, w + ": the extent of scratch_dev overflows (rows * reps * N)");
  if (scratch_bytes < need)
    return fail(SCL_ERR_BAD_ARG, w + ": scratch_bytes is " + std::to_string(scratch_bytes) + ", this call needs " + std::to_string(need) +
                                     " (scl_vf_scratch_bytes)");
  {
    std::string msg;
    const alias::Operand ops[5] = {alias::mat("out_dev", out_dev, rows, out_stride, reps, esz, true),
                                   alias::vec("scratch_dev", scratch_dev, need, 1, true),
                                   alias::mat("x_dev", x_dev, rows, op_stride, N, esz, false),
                                   alias::mat("y_dev", y_dev, rows, op_stride, N, esz, false),
                                   alias::mat("rho_dev", rho_dev, reps, rho_stride, N, esz, false)};
    if (alias::conflict(who, ops, 5, &msg) != alias::DISJOINT) return fail(SCL_ERR_BAD_ARG, msg);
  }
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    const size_t G = vf_groups(L, fused, reps, N);
    const uint64_t* rho = rho_dev;
    size_t rstride = rho_stride;
    AesKey key;
    if (prg) make_aes_key(seed_host, seed_len, key);
    if (prg && !fused) {  // two-pass: the coefficient rows first, with the kernel of scl_hip_vector_random
      uint64_t* rows_dev = scratch_dev + pbytes / 8;
      rstride = rho_pitch(L, N);
      rho = rows_dev;
      const size_t work = F::LIMBS == 4 ? (N + 1) / 2 : ((F::LIMBS == 1 ? (N + 1) / 2 : N) + 3) / 4;
      for (size_t j = 0; j < reps && N; ++j) {
        aes_key_range(key, counter0 + j * B, B);
        AES4_LAUNCH_GRID((k_vector_random<F, true>), dim3(grid_aes4(work)), S(stream), ctx, rows_dev + j * rstride * F::LIMBS, key,
                         (u64)(counter0 + j * B), N);
      }
    }
    // a Mersenne61 pair in one access: every base 16-byte aligned, every stride that separates rows even
    bool al = true;
    if (F::LIMBS == 1) {
      for (const void* p : {(const void*)x_dev, (const void*)y_dev, (const void*)rho})
        if (reinterpret_cast<uintptr_t>(p) & 15) al = false;
      if ((rows > 1 && (op_stride & 1)) || (rho && reps > 1 && (rstride & 1))) al = false;
    }
    // the 32-byte fields hold two repetitions' accumulators and coefficients without spilling: three and four repetitions are
    // two launches, which read x twice
    const size_t cap = vf_reps_per_launch(L);
    for (size_t j0 = 0; j0 < reps; j0 += cap) {
      const size_t lr = reps - j0 < cap ? reps - j0 : cap;
      for (size_t r0 = 0; r0 < rows;) {
        const int rc = with_shape(al, lr, y_dev != nullptr, [&](auto AL, auto RP, auto PR) -> int {
          constexpr bool A = F::LIMBS == 1 ? decltype(AL)::value : true;
          constexpr int REPS = (size_t)decltype(RP)::value <= vf_reps_per_launch(F::LIMBS) ? decltype(RP)::value : 1;
          constexpr bool PROD = decltype(PR)::value;
          const uint64_t *xx = x_dev + r0 * op_stride * L, *yy = y_dev ? y_dev + r0 * op_stride * L : nullptr;
          uint64_t* pp = scratch_dev + (r0 * reps + j0) * G * L;
          if constexpr (vf_fused(F::TAG)) {
            if (fused) {
              constexpr size_t R = vf_rows_per_group(F::LIMBS, true, REPS);
              const size_t span = GRID_Y_MAX * R, nrows = rows - r0 < span ? rows - r0 : span;
              aes_key_range(key, counter0 + j0 * B, lr * B);
              AES4_LAUNCH_GRID((k_vf_combine_prg<F, A, REPS, PROD>), dim3((unsigned)G, (unsigned)((nrows + R - 1) / R)), S(stream), ctx, pp, xx, yy,
                               op_stride, key, (u64)(counter0 + j0 * B), (u64)B, nrows, N, reps);
              r0 += nrows;
              return SCL_OK;
            }
          }
          constexpr size_t R = vf_rows_per_group(F::LIMBS, false, REPS);
          const size_t span = GRID_Y_MAX * R, nrows = rows - r0 < span ? rows - r0 : span;
          hipLaunchKernelGGL((k_vf_combine_rows<F, A, REPS, PROD>), dim3((unsigned)G, (unsigned)((nrows + R - 1) / R)), dim3(BLOCK), 0, S(stream), ctx, pp, xx,
                             yy, op_stride, rho ? rho + j0 * rstride * L : nullptr, rstride, nrows, N, reps);
          HIP_TRY(hipGetLastError());
          r0 += nrows;
          return SCL_OK;
        });
        if (rc != SCL_OK) return rc;
      }
    }
    const size_t vals = rows * reps;
    for (size_t k0 = 0; k0 < vals; k0 += 0x7fffffffu) {
      const size_t nk = vals - k0 < 0x7fffffffu ? vals - k0 : 0x7fffffffu;
      hipLaunchKernelGGL((k_vf_finish<F>), dim3((unsigned)nk), dim3(BLOCK), 0, S(stream), ctx, out_dev, out_stride, scratch_dev, G, k0, reps);
      HIP_TRY(hipGetLastError());
    }
    return SCL_OK;
  });
}
}  // namespace

extern "C" {

int scl_vf_abi_version(void) { return SCL_VF_ABI_VERSION; }
const char* scl_vf_last_error(void) { return g_err.c_str(); }

size_t scl_vf_coin_blocks(int field, size_t N) {
  const size_t L = limbs_of(field);
  if (!L) return 0;
  return L == 1 ? N / 2 + (N & 1) : N > ((size_t)1 << 62) ? 0 : N * (L / 2);
}

size_t scl_vf_scratch_bytes(int field, size_t rows, size_t reps, size_t N, unsigned flags) {
  const size_t L = limbs_of(field);
  if (!L || reps == 0 || reps > VF_REPS_MAX || (flags & ~SCL_VF_PRG)) return 0;
  const bool prg = flags & SCL_VF_PRG, fused = prg && vf_fused(field);
  size_t b = 0;
  if (!partial_bytes(L, fused, rows, reps, N, &b)) return 0;
  if (prg && !fused) {
    size_t rb = 0;
    if (N > ((size_t)1 << 62) || __builtin_mul_overflow(rho_pitch(L, N), reps * 8 * L, &rb) || __builtin_add_overflow(b, round16(rb), &b)) return 0;
  }
  return b > ((size_t)1 << 62) ? 0 : b;
}

void scl_vf_launch_shape(int field, size_t reps, int prg, int* rows_per_group, size_t* cols_per_trip, size_t* max_groups, int* fused) {
  const size_t L = limbs_of(field);
  const bool ok = L && reps >= 1 && reps <= VF_REPS_MAX, aes = ok && prg && vf_fused(field);
  if (rows_per_group) *rows_per_group = ok ? vf_rows_per_group(L, aes, reps) : 0;
  if (cols_per_trip) *cols_per_trip = ok ? vf_cols_per_trip(L, aes, reps) : 0;
  if (max_groups) *max_groups = ok ? (aes ? VF_GRID_AES : VF_GRID_STREAM) : 0;
  if (fused) *fused = aes ? 1 : 0;
}

int scl_vf_combine_prg(int field, uint64_t* out_dev, size_t out_stride, const uint64_t* x_dev, const uint64_t* y_dev, size_t op_stride, size_t rows,
                       size_t N, size_t reps, const unsigned char* seed_host, size_t seed_len, uint64_t counter0, uint64_t* scratch_dev,
                       size_t scratch_bytes, void* stream) {
  return combine_common("combine_prg", true, field, out_dev, out_stride, x_dev, y_dev, op_stride, nullptr, 0, rows, N, reps, seed_host, seed_len, counter0,
                        scratch_dev, scratch_bytes, stream);
}

int scl_vf_combine(int field, uint64_t* out_dev, size_t out_stride, const uint64_t* x_dev, const uint64_t* y_dev, size_t op_stride,
                   const uint64_t* rho_dev, size_t rho_stride, size_t rows, size_t N, size_t reps, uint64_t* scratch_dev, size_t scratch_bytes,
                   void* stream) {
  return combine_common("combine", false, field, out_dev, out_stride, x_dev, y_dev, op_stride, rho_dev, rho_stride, rows, N, reps, nullptr, 0, 0,
                        scratch_dev, scratch_bytes, stream);
}

}  // extern "C"
