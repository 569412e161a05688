// csrc/unit_host.hpp -- the host side every translation unit of csrc/ shares: what stands between a unit's kernels and its
// extern "C" block.  Host code only, everything in an anonymous namespace: include it ONCE per unit, after the kernels and
// before the entry points.  Two macros, defined before the include, say what the unit is:
//
//   SCL_UNIT_ENGINE   a unit of libscl_hip.so (capi.hip, ec_, ecdsa_, pedersen_, hash_unit.hip, merkle_leaves.hip): the
//                     diagnostics go to the engine's slot, sclhip_state::g_err, which capi.hip defines; the generic part only.
//                     Without it the unit is an extension library beside the engine (libscl_hip_mpc / _prep / _hm / _ip / _vf / _rb / _fx):
//                     it owns its slot and, serving every field from one unit, takes the field part too, which wants
//                     sclhip::BLOCK declared -- kernels.hpp's, or the unit's own (beaver_unit.hip).
//   SCL_UNIT_AES      the unit launches four-table AES kernels: the AES part, which needs kernels.hpp.
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
extern thread_local std::string g_err;  // the thread's last diagnostic (defined in the common unit of capi.hip)
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
#include "../../include/scl_hip/detail/field.hpp"

namespace {
using namespace sclhip;

constexpr size_t GRID_Y_MAX = 65535;

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

// two one-limb elements per lane: every base 16-byte aligned, every stride that separates rows or terms even
bool two_per_lane(size_t limbs, std::initializer_list<const void*> ptrs, std::initializer_list<size_t> strides) {
  if (limbs != 1) return false;
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  for (size_t s : strides)
    if (s & 1) return false;
  return true;
}

}  // namespace
#endif  // !SCL_UNIT_ENGINE

// ---- the AES part ----------------------------------------------------------------------------------------------------------
#ifdef SCL_UNIT_AES
#include "aes_key_host.hpp"  // make_aes_key

namespace {

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
