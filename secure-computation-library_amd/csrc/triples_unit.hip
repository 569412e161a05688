// csrc/triples_unit.hip -- the trusted dealer of multiplication triples in the reference's PRG order: the kernels and the C ABI
// of libscl_hip_prep.so (include/scl_hip_prep.h), an extension library beside the engine.  One translation unit, all fields.
//
// The reference deals a triple by randomTriple2 (test/scl/protocol/triple.h:37-48): a, b, then the sharings of a, of b and of
// c = a b, all drawn from one util::PRG before the next triple begins.  Every PRG-driven entry point of the engine puts secret
// s at counter0 + s * (its own block count), so no composition of them reaches that order; the AES blocks are counter-addressed,
// though, so a lane that deals triple s encrypts the blocks [counter0 + s B, counter0 + (s+1) B) itself (the header states B
// and the order of the draws; the draws themselves are csrc/prg_deal.hpp, which hm_unit.hip shares).  Three kernels, all on
// the four-table AES of kernels.hpp (1024-lane workgroups, the 128 KiB of tables at the bottom of 132 KiB of dynamic LDS, one
// workgroup per CU behind a grid-stride loop):
//   k_triples_additive_prg  one lane = one triple (Mersenne61 on 16-byte bases and an even stride: two): B blocks, one product,
//                           3 n row elements from three running differences
//   k_triples_shamir_prg    one lane = one triple, the three polynomials one after another (at most t + 1 coefficients live),
//                           the parties in a rolled loop, Horner at the small node i + 1 (F::muladd_small_lazy steps, one
//                           F::canon at the end); one kernel per threshold 0..7
//   k_triple_coeff_rows     the first of two passes: a, b, c and the 3 t coefficient rows into the caller's scratch; the engine's
//                           explicit-coefficient scl_hip_shamir_share evaluates them (three calls)
// None of them reads device memory.  The engine is reached through the prototypes of scl_hip.h only.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip_prep.h"
#include "kernels.hpp"
#include "prg_deal.hpp"

namespace sclhip {
namespace {

// additive: triple s = q*VEC + v at blocks counter0 + s*B, B = (2 + 3(n-1)) BPE; matrix m (0 a, 1 b, 2 c) draws its n-1 random
// shares at element index 2 + m(n-1) + i of the triple, the last row is the secret minus their sum
template <class F, int VEC>
__global__ __launch_bounds__(ABLOCK) void k_triples_additive_prg(typename F::Ctx ctx, u64* a_out, u64* b_out, u64* c_out,
                                                                 size_t stride, AesKey key, u64 counter0, int n, size_t npacks) {
  SCL_AES4_PROLOGUE(key)
  constexpr int BPE = bpe<F>();
  const u64 B = (u64)(2 + 3 * (u64)(n - 1)) * BPE;
  SCL_AES4_GRID_STRIDE(q, npacks) {
    const size_t off = q * VEC * F::LIMBS;
    Pack<F, VEC> last[3];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const u64 c0 = counter0 + (q * VEC + v) * B;
      last[0].v[v] = draw_elem<F>(ctx, aes, key, c0);
      last[1].v[v] = draw_elem<F>(ctx, aes, key, c0 + BPE);
      last[2].v[v] = F::mul(ctx, last[0].v[v], last[1].v[v]);
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      u64* out = (m == 0 ? a_out : m == 1 ? b_out : c_out) + off;
#pragma unroll 1
      for (int i = 0; i + 1 < n; ++i) {
        Pack<F, VEC> r;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          r.v[v] = draw_elem<F>(ctx, aes, key, counter0 + (q * VEC + v) * B + (u64)(2 + (u64)m * (n - 1) + i) * BPE);
          last[m].v[v] = F::sub(ctx, last[m].v[v], r.v[v]);
        }
        store_pack<F, VEC, true>(out + (size_t)i * stride * F::LIMBS, r);
      }
      store_pack<F, VEC, true>(out + (size_t)(n - 1) * stride * F::LIMBS, last[m]);
    }
  }
}

// every triple of the launch at threshold T: the three polynomials one after another, the parties in a rolled loop
template <class F, int T>
__device__ __forceinline__ void deal_shamir(const typename F::Ctx& ctx, const Aes4& aes, const AesKey& key, u64* a_out, u64* b_out,
                                            u64* c_out, size_t stride, u64 counter0, int n, size_t N) {
  constexpr int BPE = bpe<F>();
  constexpr u64 Bs = poly_blocks<F>(T), B = 2 * BPE + 3 * Bs;
  SCL_AES4_GRID_STRIDE(s, N) {
    const u64 c0 = counter0 + s * B;
    const typename F::E a = draw_elem<F>(ctx, aes, key, c0), b = draw_elem<F>(ctx, aes, key, c0 + BPE);
    const typename F::E ab = F::mul(ctx, a, b);
#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
      typename F::E c[T + 1];
      c[0] = m == 0 ? a : m == 1 ? b : ab;
      draw_poly<F, T>(ctx, aes, key, c0 + 2 * BPE + (u64)m * Bs, c);
      eval_rows<F, T>(ctx, c, (m == 0 ? a_out : m == 1 ? b_out : c_out) + s * F::LIMBS, stride, n);
    }
  }
}

// Shamir, fused: triple s at blocks counter0 + s*B, B = 2 BPE + 3 Bs.  One kernel per threshold T, so that the coefficients
// stay in registers and Horner has no tests in it.  Fields with F::muladd_small_lazy (the Mersenne fields, GF(2^128)): node
// i+1 < 2^16.
template <class F, int T>
__global__ __launch_bounds__(ABLOCK) void k_triples_shamir_prg(typename F::Ctx ctx, u64* a_out, u64* b_out, u64* c_out,
                                                               size_t stride, AesKey key, u64 counter0, int n, size_t N) {
  SCL_AES4_PROLOGUE(key)
  deal_shamir<F, T>(ctx, aes, key, a_out, b_out, c_out, stride, counter0, n, N);
}

// Two-pass, first pass: rows 0, 1, 2 of the scratch are a, b, c = a b; row 3 + m t + (k-1) is coefficient k of polynomial m.
// Rows are N elements apart.
template <class F>
__global__ __launch_bounds__(ABLOCK) void k_triple_coeff_rows(typename F::Ctx ctx, u64* rows, AesKey key, u64 counter0, int t,
                                                              size_t N) {
  SCL_AES4_PROLOGUE(key)
  constexpr int BPE = bpe<F>();
  const u64 Bs = poly_blocks<F>((u64)t), B = 2 * BPE + 3 * Bs;
  SCL_AES4_GRID_STRIDE(s, N) {
    const u64 c0 = counter0 + s * B;
    const typename F::E a = draw_elem<F>(ctx, aes, key, c0), b = draw_elem<F>(ctx, aes, key, c0 + BPE);
    F::st(rows + s * F::LIMBS, a);
    F::st(rows + (N + s) * F::LIMBS, b);
    F::st(rows + (2 * N + s) * F::LIMBS, F::mul(ctx, a, b));
#pragma unroll 1
    for (int m = 0; m < 3; ++m) {
      const u64 p0 = c0 + 2 * BPE + (u64)m * Bs;
      u64* base = rows + ((size_t)(3 + (size_t)m * t) * N + s) * F::LIMBS;  // coefficient 1 of polynomial m
      if constexpr (F::LIMBS == 1) {
#pragma unroll 1
        for (int j = 0; 2 * j <= t; ++j) {  // block j = coefficients 2j (low 8 bytes) and 2j+1 (high 8 bytes)
          u64 lo, hi;
          aes.block(key, p0 + j, lo, hi);
          if (j > 0) base[(size_t)(2 * j - 1) * N] = F::from_le_word(ctx, lo);
          if (2 * j + 1 <= t) base[(size_t)(2 * j) * N] = F::from_le_word(ctx, hi);
        }
      } else {
#pragma unroll 1
        for (int k = 1; k <= t; ++k) {
          u64 lo[BPE], hi[BPE];
#pragma unroll
          for (int bb = 0; bb < BPE; ++bb) aes.block(key, p0 + (u64)k * BPE + bb, lo[bb], hi[bb]);
          F::st(base + (size_t)(k - 1) * N * F::LIMBS, elem_from_blocks<F>(ctx, lo, hi));
        }
      }
    }
  }
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#define SCL_UNIT_AES
#include "unit_host.hpp"

namespace {

constexpr size_t FUSED_TMAX = 7;        // the fused Shamir kernel keeps t + 1 <= 8 coefficients in registers

bool fused_shamir(int field, size_t t, unsigned flags) {
  return !(flags & SCL_PREP_TWO_PASS) && t <= FUSED_TMAX && (field == SCL_M61 || field == SCL_M127 || field == SCL_GF2_128);
}

size_t additive_blocks(size_t limbs, size_t n) { return (2 + 3 * (n - 1)) * bpe_of(limbs); }
size_t shamir_blocks(size_t limbs, size_t t) { return 2 * bpe_of(limbs) + 3 * (((t + 1) * 8 * limbs + 15) / 16); }
bool additive_n_ok(size_t n) { return n >= 2 && n <= 0x7fffffffu / 4; }
bool shamir_nt_ok(size_t limbs, size_t n, size_t t) { return n >= 1 && n <= PARTY_MAX && t <= deg_max(limbs); }

// what both deal calls check alike, in the order the header lists it; B = blocks per triple
int check_matrices(const char* who, size_t limbs, uint64_t* a, uint64_t* b, uint64_t* c, size_t stride, size_t N, size_t n, uint64_t B,
                   uint64_t counter0) {
  const std::string w(who);
  if (!a || !b || !c) return fail(SCL_ERR_BAD_ARG, w + ": NULL operand");
  if (const int rc = check_align(who, limbs, {a, b, c})) return rc;
  if (stride < N) return fail(SCL_ERR_SIZE_MISMATCH, w + ": stride < N");
  if (n > ((size_t)1 << 60) / stride / limbs) return fail(SCL_ERR_BAD_ARG, w + ": n * stride overflows");
  const Span sa = span_of(a, n, stride, N, limbs), sb = span_of(b, n, stride, N, limbs), sc = span_of(c, n, stride, N, limbs);
  if (overlap(sa, sb) || overlap(sa, sc) || overlap(sb, sc)) return fail(SCL_ERR_BAD_ARG, w + ": the share matrices overlap");
  return check_counter_range(w, counter0, N, B);
}

}  // namespace

extern "C" {

int scl_prep_abi_version(void) { return SCL_PREP_ABI_VERSION; }
const char* scl_prep_last_error(void) { return g_err.c_str(); }

size_t scl_prep_triple_blocks(int field, int scheme, size_t n, size_t t) {
  const size_t L = limbs_of(field, true);
  if (scheme == SCL_PREP_ADDITIVE) return L && additive_n_ok(n) ? additive_blocks(L, n) : 0;
  if (scheme == SCL_PREP_SHAMIR) return is_field(field) && shamir_nt_ok(L, n, t) ? shamir_blocks(L, t) : 0;
  return 0;
}

size_t scl_prep_triples_scratch_bytes(int field, size_t N, size_t n, size_t t, unsigned flags) {
  if (!is_field(field) || !shamir_nt_ok(limbs_of(field), n, t) || (flags & ~SCL_PREP_TWO_PASS) || fused_shamir(field, t, flags)) return 0;
  const size_t per = (3 + 3 * t) * 8 * limbs_of(field);
  return N > ((size_t)1 << 62) / per ? 0 : N * per;
}

int scl_prep_triples_additive_prg(int field, uint64_t* a_dev, uint64_t* b_dev, uint64_t* c_dev, size_t stride, size_t N, size_t n,
                                  const unsigned char* seed_host, size_t seed_len, uint64_t counter0, void* stream) {
  if (N == 0) return SCL_OK;
  const size_t L = limbs_of(field, true);
  if (!L) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  if (!additive_n_ok(n)) return fail(SCL_ERR_BAD_ARG, "triples_additive_prg: n must be >= 2 (and below 2^29)");
  const uint64_t B = additive_blocks(L, n);
  if (const int rc = check_matrices("triples_additive_prg", L, a_dev, b_dev, c_dev, stride, N, n, B, counter0)) return rc;
  return with_ring_or_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    AesKey key;
    make_aes_key(seed_host, seed_len, key);
    aes_key_range(key, counter0, (u64)N * B);
    // two one-limb triples per lane: 16-byte aligned bases and an even stride; an odd N leaves one triple to a launch of its own
    bool two = F::LIMBS == 1 && !(stride & 1);
    for (const uint64_t* p : {a_dev, b_dev, c_dev}) two = two && !(reinterpret_cast<uintptr_t>(p) & 15);
    size_t first = 0;
    if constexpr (F::LIMBS == 1) {
      if (two && N >= 2) {
        AES4_LAUNCH((k_triples_additive_prg<F, 2>), N / 2, S(stream), ctx, a_dev, b_dev, c_dev, stride, key, (u64)counter0, (int)n, N / 2);
        first = N & ~(size_t)1;
      }
    }
    if (first < N)
      AES4_LAUNCH((k_triples_additive_prg<F, 1>), N - first, S(stream), ctx, a_dev + first * F::LIMBS, b_dev + first * F::LIMBS,
                  c_dev + first * F::LIMBS, stride, key, (u64)(counter0 + first * B), (int)n, N - first);
    return SCL_OK;
  });
}

int scl_prep_triples_shamir_prg(int field, uint64_t* a_dev, uint64_t* b_dev, uint64_t* c_dev, size_t stride, size_t N, size_t t,
                                size_t n, const unsigned char* seed_host, size_t seed_len, uint64_t counter0, uint64_t* scratch_dev,
                                unsigned flags, void* stream) {
  if (N == 0) return SCL_OK;
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  Mont128::Ctx mont = {};
  if (const int rc = mont_latch(field, mont)) return rc;
  if (flags & ~SCL_PREP_TWO_PASS) return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: unknown flags bit (only bit 0, two-pass, is defined)");
  const size_t L = limbs_of(field);
  if (!shamir_nt_ok(L, n, t))
    return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: n must be in 1..65535 and the threshold t at most " + std::to_string(deg_max(L)) +
                                     " for this field (beyond it the engine's share call synchronises the stream)");
  const uint64_t B = shamir_blocks(L, t);
  if (const int rc = check_matrices("triples_shamir_prg", L, a_dev, b_dev, c_dev, stride, N, n, B, counter0)) return rc;
  const bool fused = fused_shamir(field, t, flags);
  if (!fused) {
    const size_t need = scl_prep_triples_scratch_bytes(field, N, n, t, flags);
    if (!need) return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: (3 + 3t) * N overflows");
    if (!scratch_dev)
      return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: this case takes the two-pass path and needs " + std::to_string(need) +
                                       " bytes of scratch (scl_prep_triples_scratch_bytes); scratch_dev is NULL");
    if (reinterpret_cast<uintptr_t>(scratch_dev) & 15) return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: scratch pointer not 16-byte aligned");
    const Span ss = {scratch_dev, scratch_dev + need / 8};
    for (const uint64_t* p : {a_dev, b_dev, c_dev})
      if (overlap(ss, span_of(p, n, stride, N, L))) return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: the scratch overlaps a share matrix");
  }
  return with_field(field, mont, [&](auto f, auto ctx) -> int {
    using F = decltype(f);
    if (const int rc = need_device()) return rc;
    AesKey key;
    make_aes_key(seed_host, seed_len, key);
    aes_key_range(key, counter0, (u64)N * B);
    if constexpr (F::TAG == 0 || F::TAG == 1 || F::TAG == 3) {
      if (fused) {
#define TRIPLES_CASE(TT) \
  case TT: AES4_LAUNCH((k_triples_shamir_prg<F, TT>), N, S(stream), ctx, a_dev, b_dev, c_dev, stride, key, (u64)counter0, (int)n, N); break;
        switch (t) {
          TRIPLES_CASE(0) TRIPLES_CASE(1) TRIPLES_CASE(2) TRIPLES_CASE(3) TRIPLES_CASE(4) TRIPLES_CASE(5) TRIPLES_CASE(6) TRIPLES_CASE(7)
          default: return fail(SCL_ERR_BAD_ARG, "triples_shamir_prg: internal threshold");
        }
#undef TRIPLES_CASE
        return SCL_OK;
      }
    }
    AES4_LAUNCH((k_triple_coeff_rows<F>), N, S(stream), ctx, scratch_dev, key, (u64)counter0, (int)t, N);
    uint64_t* outs[3] = {a_dev, b_dev, c_dev};
    for (size_t m = 0; m < 3; ++m) {
      const uint64_t* coeffs = t ? scratch_dev + (3 + m * t) * N * F::LIMBS : nullptr;
      const int rc = scl_hip_shamir_share(field, outs[m], stride, scratch_dev + m * N * F::LIMBS, coeffs, t ? N : 0, N, t, n, nullptr, stream);
      if (rc != SCL_OK) return fail(rc, std::string("triples_shamir_prg: scl_hip_shamir_share: ") + scl_hip_last_error());
    }
    return SCL_OK;
  });
}

}  // extern "C"
