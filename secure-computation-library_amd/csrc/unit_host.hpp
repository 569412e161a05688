// csrc/unit_host.hpp -- the host side every translation unit of csrc/ shares: what stands between a unit's kernels and its
// extern "C" block.  Host code only, everything in an anonymous namespace: include it ONCE per unit, after the kernels and
// before the entry points.  Two macros, defined before the include, say what the unit is:
//
//   SCL_UNIT_ENGINE   a unit of libscl_hip.so (capi.hip, ec_, ecdsa_, pedersen_, hash_unit.hip, merkle_leaves.hip): the
//                     diagnostics go to the engine's slot, sclhip_state::g_err (engine_state.hpp; capi.hip's common unit defines it); the generic part only.
//                     Without it the unit is an extension library beside the engine (libscl_hip_mpc / _prep / _hm / _ip / _vf / _rb / _fx):
//                     it owns its slot and, serving every field from one unit, takes the field part too: the dispatch on the
//                     field tag and the latch rule, the checks the entry points share (check_align, check_ptr,
//                     check_prime_field, extent_of), and the host half of unit_device.hpp -- the launch rule of the pack
//                     kernels (two_per_lane, grid_for_packs, PACK_LAUNCH, rows in chunks of GRID_Y_MAX) and make_open_table.
//                     For BLOCK and OpenTable the field part includes unit_device.hpp itself, and with it kernels.hpp: every
//                     extension unit has both whether it names them or not, and a unit includes them before its kernels only
//                     because its kernels use them.
//   SCL_UNIT_AES      the unit launches four-table AES kernels: the AES part -- the launch, and for the dealers of prg_deal.hpp
//                     the limits on the parties and the degree and the check of the counter range.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/scl_hip.h"
#include "../../include/scl_hip/detail/span.hpp"

// ---- the generic part ------------------------------------------------------------------------------------------------------
#ifdef SCL_UNIT_ENGINE
namespace sclhip_state {
extern thread_local std::string g_err;  // the thread's last diagnostic (engine_state.hpp; defined in the common unit of capi.hip)
}  // namespace sclhip_state
#endif

namespace {

#ifdef SCL_UNIT_ENGINE
int fail(int code, const std::string& msg) {
  sclhip_state::g_err = msg;
  return code;
}
#else
thread_local std::string g_err;  // the thread's last diagnostic of THIS library

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#endif

#define HIP_TRY(expr)                                                                                                        \
  do {                                                                                                                       \
    hipError_t e_ = (expr);                                                                                                  \
    if (e_ != hipSuccess)                                                                                                    \
      return fail(e_ == hipErrorNoDevice ? SCL_ERR_NO_DEVICE : SCL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define SCL_TRY(expr)            \
  do {                           \
    int s_ = (expr);             \
    if (s_ != SCL_OK) return s_; \
  } while (0)

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int need_device() {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  return SCL_OK;
}

// the aliasing rule of scl_hip.h (Conventions), checked before anything is enqueued: the call's device operands as bounding
// spans (detail/span.hpp); an overlap the entry point does not permit is refused with the message that names the pair
int alias_check(const char* who, std::initializer_list<sclhip::alias::Operand> ops) {
  std::string msg;
  if (sclhip::alias::conflict(who, ops.begin(), ops.size(), &msg) != sclhip::alias::DISJOINT) return fail(SCL_ERR_BAD_ARG, msg);
  return SCL_OK;
}

}  // namespace

// ---- the field part --------------------------------------------------------------------------------------------------------
#ifndef SCL_UNIT_ENGINE
#include <utility>

#include "../../include/scl_hip/detail/field.hpp"
#include "unit_device.hpp"  // BLOCK, OpenTable

namespace {
using namespace sclhip;

constexpr size_t GRID_Y_MAX = 65535;  // rows (and, with a third dimension, tiles or groups) one launch takes: the sites chunk by it

unsigned grid_for(size_t items) {  // one pack per lane; past 2^31 - 1 blocks the kernels' grid-stride loops take over
  const size_t blocks = (items + BLOCK - 1) / BLOCK;
  return (unsigned)(blocks < 1 ? 1 : blocks > 0x7fffffffu ? 0x7fffffffu : blocks);
}

bool is_ring(int field) { return field > 0x100 && field <= 0x100 + 128; }
bool is_field(int field) { return field >= SCL_M61 && field <= SCL_SECP256K1_FIELD; }
// 0: not one of the six fields -- nor, where the entry point serves them (`rings`), a ring Z2k<K>
size_t limbs_of(int field, bool rings = false) {
  if (rings && is_ring(field)) return field - 0x100 <= 64 ? 1 : 2;
  switch (field) {
    case SCL_M61: return 1;
    case SCL_M127: case SCL_MONT128: case SCL_GF2_128: return 2;
    case SCL_SECP256K1_SCALAR: case SCL_SECP256K1_FIELD: return 4;
    default: return 0;
  }
}
size_t bpe_of(size_t limbs) { return limbs >= 2 ? limbs / 2 : 1; }  // AES blocks one FF::random burns

// The calling thread's Mont128 parameters: the modulus is the engine's (scl_hip_mont128_get_prime), the constants are rebuilt
// when it changes.  The engine's stale-latch check runs first.  No prototype of scl_hip.h performs that check alone, so it is
// reached through the cheapest host-only entry point that does: scl_hip_lagrange_basis on ONE node (two small host vectors, no
// device work -- the one place where a call of an extension library allocates, on the host and for Mont128 only).  That the
// entry point keeps the check in front of its work is pinned from this side, once per library, by
// test_mont128_honours_the_latch_rule of tests/test_mpc_abi.py, test_prep_abi.py, test_hm_abi.py, test_ip_abi.py,
// test_vf_abi.py, test_rb_abi.py and test_fx_abi.py, which fail the day it does not.
int mont_ctx(Mont128::Ctx& out) {
  uint64_t one_node[2];
  const int rc = scl_hip_lagrange_basis(SCL_MONT128, one_node, nullptr, 1, nullptr);
  if (rc != SCL_OK) return fail(rc, scl_hip_last_error());
  uint64_t p[2];
  scl_hip_mont128_get_prime(p);
  static thread_local Mont128::Ctx cached = {0, 0, 0, 0, 0, 0};
  const u128 prime = ((u128)p[1] << 64) | p[0];
  if (cached.p != prime) cached = Mont128::make_ctx(prime);
  out = cached;
  return SCL_OK;
}

// The latch rule comes first among a call's checks, as in the engine: a stale thread learns of it whatever else is wrong.
// The context it yields is the call's: the dispatchers below take it, so a call asks the engine once.
int mont_latch(int field, Mont128::Ctx& ctx) { return field == SCL_MONT128 ? mont_ctx(ctx) : SCL_OK; }

template <class Fn>
int with_field(int field, const Mont128::Ctx& mont, Fn&& fn) {  // `mont`: what mont_latch yielded for this call
  switch (field) {
    case SCL_M61: return fn(M61{}, M61::Ctx{});
    case SCL_M127: return fn(M127{}, M127::Ctx{});
    case SCL_MONT128: return fn(Mont128{}, mont);
    case SCL_GF2_128: return fn(Gf128{}, Gf128::Ctx{});
    case SCL_SECP256K1_SCALAR: return fn(Secp256k1Scalar{}, Secp256k1Scalar::Ctx{});
    case SCL_SECP256K1_FIELD: return fn(Secp256k1Field{}, Secp256k1Field::Ctx{});
    default: return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  }
}
template <class Fn>
int with_ring_or_field(int field, const Mont128::Ctx& mont, Fn&& fn) {
  if (is_ring(field)) {
    const int K = field - 0x100;
    if (K <= 64) return fn(Z2k64{}, Z2k64::make_ctx(K));
    return fn(Z2k128{}, Z2k128::make_ctx(K));
  }
  return with_field(field, mont, fn);
}

struct Span {  // the words a matrix of `rows` rows of N elements, `stride` elements apart, covers: [lo, hi)
  const uint64_t *lo, *hi;
};
Span span_of(const uint64_t* p, size_t rows, size_t stride, size_t N, size_t limbs) { return {p, p + ((rows - 1) * stride + N) * limbs}; }
bool overlap(const Span& a, const Span& b) { return a.lo < b.hi && b.lo < a.hi; }

// `who`: the entry point the message names first; nullptr: the bare message
int check_align(const char* who, size_t limbs, std::initializer_list<const void*> ptrs) {
  const uintptr_t mask = limbs == 1 ? 7 : 15;
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & mask)
      return fail(SCL_ERR_BAD_ARG, (who ? std::string(who) + ": " : std::string()) + (limbs == 1 ? "pointer not 8-byte aligned" : "pointer not 16-byte aligned"));
  return SCL_OK;
}

// `w`: the entry point; `name`: the parameter the message names
int check_ptr(const std::string& w, size_t L, const char* name, const void* p) {
  if (!p) return fail(SCL_ERR_BAD_ARG, w + ": " + name + " is NULL");
  if (reinterpret_cast<uintptr_t>(p) & (L == 1 ? 7 : 15)) return fail(SCL_ERR_BAD_ARG, w + ": " + name + (L == 1 ? " not 8-byte aligned" : " not 16-byte aligned"));
  return SCL_OK;
}

// a library of the five prime fields: the tags it refuses, GF(2^128) and the rings each with the library's own reason
int check_prime_field(const std::string& w, int field, const char* gf_reason, const char* ring_reason) {
  if (field == SCL_GF2_128) return fail(SCL_ERR_BAD_ARG, w + ": SCL_GF2_128 is refused: " + gf_reason);
  if (is_ring(field)) return fail(SCL_ERR_BAD_ARG, w + ": a ring tag is refused: " + ring_reason);
  if (!is_field(field)) return fail(SCL_ERR_BAD_ARG, w + ": unknown field tag");
  return SCL_OK;
}

// An operand addressed with several strides, as span.hpp sees it: ONE row of its bounding extent
// sum_j (count_j - 1) stride_j + N elements.  false: the extent does not fit size_t.
bool extent_of(std::initializer_list<std::pair<size_t, size_t>> dims, size_t N, size_t* out) {
  size_t e = N;
  for (const auto& d : dims) {
    size_t part = 0;
    if (d.first == 0) continue;
    if (__builtin_mul_overflow(d.first - 1, d.second, &part) || __builtin_add_overflow(e, part, &e)) return false;
  }
  *out = e;
  return true;
}

// ---- the pack kernels (unit_device.hpp: for_each_pack) ----
// two one-limb elements per lane: every base 16-byte aligned, every stride that separates rows or terms even
bool two_per_lane(size_t limbs, std::initializer_list<const void*> ptrs, std::initializer_list<size_t> strides) {
  if (limbs != 1) return false;
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  for (size_t s : strides)
    if (s & 1) return false;
  return true;
}

// blocks along x for a row of N elements: one lane per pair and one for the odd element after the last pair, or one per element
unsigned grid_for_packs(bool two, size_t N) { return grid_for(two ? N / 2 + (N & 1) : N); }

// Launch a pack kernel, KERNEL<F, VEC, further template arguments...> with VEC = 2 where `TWO` (what two_per_lane said) and 1
// elsewhere, on GRID -- dim3(grid_for_packs(TWO, N), rows, ...) -- with the remaining arguments.  KSPEC names the kernel in
// parentheses, (KERNEL, F) or (KERNEL, F, further...).  The two-per-lane form exists for the one-limb fields only.  As in
//   PACK_LAUNCH((k_hm_mask, F), two, dim3(grid_for_packs(two, N), (unsigned)rows), S(stream), ctx, d, d_stride, x, y, r2, op_stride, N);
//   PACK_LAUNCH((k_hm_apply, F, R), two, dim3(grid_for_packs(two, N), nb, ng), S(stream), ctx, ...);   // k_hm_apply<F, VEC, R>
// (KSPEC is taken apart by the helper macros below; with no further arguments the comma before them goes by the compilers'
// `, ##__VA_ARGS__`.  A KSPEC without its parentheses fails in the helpers' expansion, not at the kernel's name.)
#define PACK_KERNEL_(VEC, KERNEL, F, ...) KERNEL<F, VEC, ##__VA_ARGS__>
#define PACK_KERNEL_2_(...) PACK_KERNEL_(2, __VA_ARGS__)
#define PACK_KERNEL_1_(...) PACK_KERNEL_(1, __VA_ARGS__)
#define PACK_FIELD_(KERNEL, F, ...) F
#define PACK_LAUNCH(KSPEC, TWO, GRID, ST, ...)                                                        \
  do {                                                                                                \
    bool one_ = true;                                                                                 \
    if constexpr (PACK_FIELD_ KSPEC::LIMBS == 1) {                                                    \
      if (TWO) {                                                                                      \
        hipLaunchKernelGGL((PACK_KERNEL_2_ KSPEC), GRID, dim3(BLOCK), 0, ST, __VA_ARGS__);            \
        one_ = false;                                                                                 \
      }                                                                                               \
    }                                                                                                 \
    if (one_) hipLaunchKernelGGL((PACK_KERNEL_1_ KSPEC), GRID, dim3(BLOCK), 0, ST, __VA_ARGS__);      \
    HIP_TRY(hipGetLastError());                                                                       \
  } while (0)

// the recombination vector of an opening inside a finish kernel (m <= OPEN_M_MAX, which the entry point has checked)
template <class F>
OpenTable<F> make_open_table(const uint64_t* lambda_host, size_t m) {
  OpenTable<F> tab;
  for (size_t j = 0; j < (size_t)OPEN_M_MAX; ++j) tab.v[j] = j < m ? F::ld(lambda_host + j * F::LIMBS) : F::zero();
  return tab;
}

}  // namespace
#endif  // !SCL_UNIT_ENGINE

// ---- the AES part ----------------------------------------------------------------------------------------------------------
#ifdef SCL_UNIT_AES
#include "aes_key_host.hpp"  // make_aes_key

namespace {

// ---- the dealers (prg_deal.hpp) ----
constexpr size_t PARTY_MAX = 65535;  // the node i + 1 as a small integer (GF(2^128): F::muladd_small takes 16 bits)
// The largest degree the two-pass path of a dealer takes: beyond it scl_hip_shamir_share evaluates chunk by chunk, staging each
// chunk's power table from host memory and synchronising the stream before it returns -- a call of these libraries never
// synchronises
constexpr size_t DEG_MAX_NARROW = 48;  // 8- and 16-byte elements
constexpr size_t DEG_MAX_WIDE = 16;    // 32-byte elements
size_t deg_max(size_t limbs) { return limbs == 4 ? DEG_MAX_WIDE : DEG_MAX_NARROW; }

// N * B blocks from counter0 (and the slack aes_key_range adds) must not wrap the 64-bit counter
int check_counter_range(const std::string& who, uint64_t counter0, size_t N, uint64_t B) {
  const uint64_t room = ~(uint64_t)0 - 128;
  if (counter0 > room || N > (room - counter0) / B) return fail(SCL_ERR_BAD_ARG, who + ": the block range wraps the 64-bit counter");
  return SCL_OK;
}

unsigned grid_aes4(size_t work_items) {  // one 1024-lane workgroup per CU; the kernels grid-stride
  const size_t blocks = (work_items + sclhip::ABLOCK - 1) / sclhip::ABLOCK;
  return (unsigned)(blocks < 1 ? 1 : blocks > (size_t)sclhip::AES4_GRID_CAP ? (size_t)sclhip::AES4_GRID_CAP : blocks);
}
// launch KERN (a four-table AES kernel) with its 128 KiB of tables in dynamic LDS on the grid GRID, or on grid_aes4(WORK)
#define AES4_LAUNCH_GRID(KERN, GRID, ST, ...)                                                                       \
  do {                                                                                                              \
    auto kern_ = &KERN;                                                                                             \
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern_), hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                AES4_LDS_BYTES));                                                                   \
    hipLaunchKernelGGL(kern_, GRID, dim3(ABLOCK), AES4_LDS_BYTES, ST, __VA_ARGS__);                                 \
    HIP_TRY(hipGetLastError());                                                                                     \
  } while (0)
#define AES4_LAUNCH(KERN, WORK, ST, ...) AES4_LAUNCH_GRID(KERN, dim3(grid_aes4(WORK)), ST, __VA_ARGS__)

}  // namespace
#endif  // SCL_UNIT_AES
