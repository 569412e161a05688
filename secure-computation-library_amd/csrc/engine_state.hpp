// csrc/engine_state.hpp -- what the translation units of libscl_hip.so share on the host side, declared ONCE: the state of
// the library (sclhip_state), the Mont128 latch rule, the dispatch on the field tag and the per-thread device buffers.  Host
// code only, everything but the state in an anonymous namespace; it brings unit_host.hpp (the engine's part) with it.
// capi.hip, hash_unit.hip and merkle_leaves.hip include it after their kernels and before their entry points.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "tu_config.hpp"
#include "../../include/scl_hip.h"
#include "../../include/scl_hip/detail/field.hpp"

// ---- state shared by the translation units of the library ------------------------------------------------
// The library is capi.hip compiled once per field family (tu_config.hpp, Makefile) beside the units built once; capi.hip's
// unit built with SCL_TU_COMMON says SCL_ENGINE_STATE_DEFINE and defines the state below, every other unit sees it as
// extern.  Everything mutable is per host thread except the Mont128 default (behind its mutex).
struct Knob {
  long v;
  long load() const { return v; }
  Knob& operator=(long x) {
    v = x;
    return *this;
  }
};
struct Scratch {
  int device = -1;
  void* dev = nullptr;
  size_t bytes = 0;
};
struct TempArena {
  int device = -1;
  void* dev = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;
  bool pending = false;
};
// the "a zero was inverted" flag of scl_hip_ew in pinned host memory the device writes straight into: the call then needs no
// memset launch and no copy back, only the stream synchronisation it owes its caller anyway.  host == nullptr: not allocated
// (yet, or the allocation failed once: then the flag lives in the device scratch as before)
struct HostFlag {
  unsigned* host = nullptr;
  unsigned* dev = nullptr;
  bool failed = false;
};
namespace sclhip_state {
#ifdef SCL_ENGINE_STATE_DEFINE
#define SCL_STATE(decl, ...) decl __VA_ARGS__
#else
#define SCL_STATE(decl, ...) extern decl
#endif
SCL_STATE(thread_local std::string g_err);
// Experiment knobs (scl_hip_set_tuning).  Per host thread, like the Mont128 modulus below: the library keeps no mutable
// state that two host threads share, so concurrent callers with different settings cannot race (scl_hip.h, Conventions).
SCL_STATE(thread_local Knob g_max_blocks, {0});
SCL_STATE(thread_local Knob g_force_scalar, {0});
SCL_STATE(thread_local Knob g_force_table, {0});
SCL_STATE(thread_local Knob g_mfma, {0});       // 0 auto, 1 always (where applicable), -1 never
// GF(2^128) sharing at the default nodes: 1 = eight nodes per Horner loop (k_share_gf_tiles), 0 = one node at a time
// (k_share_gf_nodes) ("gf_tiles")
SCL_STATE(thread_local Knob g_gf_tiles, {1});
SCL_STATE(thread_local Knob g_open_gather_always, {0});  // the open step on ONE rank: 1 = still through RCCL's all-gather
SCL_STATE(thread_local Knob g_prg_two_pass, {0});  // PRG-driven sharing: 0 auto, 1 always two passes, -1 always fused
// Headline streaming kernels (k_recover_fixed, k_share_small): resident waves per CU (kernels.hpp, "Launch geometry");
// "stream_waves" 0 = no cap, -1 = by element size: 10 for one-word elements, 12 for wider ones (profiles/r2_probe_cap_rec.txt,
// r2_probe_c3_waves.txt)
SCL_STATE(thread_local Knob g_stream_waves, {-1});
// the same cap for the Mersenne61 small-node share kernel ("share_waves"; 0 = the 256-thread kernel without a cap)
SCL_STATE(thread_local Knob g_share_waves, {9});
SCL_STATE(thread_local Knob g_share_waves128, {12});  // .. and for the 16-byte fields' small-node share kernel ("share_waves128")
SCL_STATE(thread_local Knob g_aes_blocks, {0});
// element-wise inverse / divide: 0 auto = Montgomery's simultaneous inversion with the chain length chosen by the batch, N > 0 =
// that chain length (8, 16, 32, 64 or 128; Mersenne61: any N = its register kernel), -1 = one Fermat chain per element (k_ew, the kernels
// of rounds 1-4); GF(2^128) multiply: -1 = the register-only product ("inv_batch")
SCL_STATE(thread_local Knob g_inv_batch, {0});
SCL_STATE(thread_local Knob g_inv_two_level, {0});
SCL_STATE(thread_local Knob g_gemm_slab_mib, {0});  // digit planes per factor and launch of the general matrix-core product, MiB (0 = 1024) ("gemm_slab_mib")
SCL_STATE(thread_local Knob g_matmul_lds_min, {0});  // columns from which k_matmul (left factor in LDS, a thread per column) is taken; thin kernel likewise (0 = default) ("matmul_lds_min")
SCL_STATE(thread_local Knob g_transpose_tile, {0});  // secrets per LDS tile of the 16-byte layout bridge (0 = 512 within 40 KiB) ("transpose_tile")
// Mont128 modulus: a process-wide default, latched per host thread at its first use (mont_ctx below)
SCL_STATE(thread_local sclhip::Mont128::Ctx g_mont, = {0, 0, 0, 0});  // p == 0: this thread has not latched a modulus yet
SCL_STATE(std::mutex g_mont_default_mu);
SCL_STATE(sclhip::Mont128::Ctx g_mont_default, = {0, 0, 0, 0});
// how often the default has been set, and where this thread stands: the generation it latched (or set its own modulus) at
SCL_STATE(unsigned long g_mont_default_gen, = 0);
SCL_STATE(thread_local unsigned long g_mont_gen, = 0);
SCL_STATE(thread_local bool g_mont_own, = false);
// per-thread device scratch (only used by calls that synchronise before returning)
SCL_STATE(thread_local Scratch g_scratch);
SCL_STATE(thread_local HostFlag g_hflag);
// arena 0: tables, queues and products of one call; arena 1: the coefficient rows of a two-pass PRG sharing (whose second
// pass may take arena 0 itself)
SCL_STATE(thread_local TempArena g_temps[2]);
#undef SCL_STATE
}  // namespace sclhip_state

// fail / HIP_TRY / SCL_TRY / S / aligned16 / alias_check on the slot above
#ifndef SCL_UNIT_ENGINE
#define SCL_UNIT_ENGINE
#endif
#include "unit_host.hpp"

namespace {
using namespace sclhip;
using namespace sclhip_state;

// ---- Mont128 modulus: a process-wide default, latched per host thread ---------------------------------------
// scl_hip_mont128_set_prime sets the CALLING thread's modulus and the process-wide default.  A thread that has set its own
// keeps it whatever other threads do; a thread that never set one LATCHES the default at its first use (the modulus set last
// by any thread before that, 2^128 - 159 if none was) and keeps that value: a worker in the middle of a share-then-recover
// sequence does not switch modulus because some other thread set a different prime.  What it must not do either is go on
// SILENTLY: once the default has changed after a thread latched it, that thread's next Mont128 call fails with
// SCL_ERR_BAD_ARG (its data may be residues of either modulus -- only the caller knows) until the thread says which it means:
// scl_hip_mont128_set_prime (its own) or scl_hip_mont128_relatch (the current default).
int mont_set(u128 p) {
  if (!(p & 1) || p < 3) return fail(SCL_ERR_BAD_ARG, "mont128: modulus must be odd and >= 3");
  g_mont = Mont128::make_ctx(p);
  g_mont_own = true;
  std::lock_guard<std::mutex> lk(g_mont_default_mu);
  // the generation moves only when the default's VALUE does: pool workers that each set the same prime at start-up (or the
  // built-in 2^128 - 159) change nothing for the threads that latched it
  if (g_mont_default.p != g_mont.p) {
    g_mont_default = g_mont;
    ++g_mont_default_gen;
  }
  g_mont_gen = g_mont_default_gen;
  return SCL_OK;
}

void mont_latch_locked() {  // (g_mont_default_mu held)
  if (!g_mont_default.p)
    g_mont_default = Mont128::make_ctx((((u128)0xFFFFFFFFFFFFFFFFull) << 64) | (u128)0xFFFFFFFFFFFFFF61ull);  // 2^128 - 159
  g_mont = g_mont_default;
  g_mont_gen = g_mont_default_gen;
  g_mont_own = false;
}

// SCL_OK, or the stale-latch error described above
int mont_check() {
  if (!g_mont.p || g_mont_own) return SCL_OK;
  std::lock_guard<std::mutex> lk(g_mont_default_mu);
  if (g_mont_gen == g_mont_default_gen) return SCL_OK;
  return fail(SCL_ERR_BAD_ARG,
              "mont128: this thread latched the process-wide default modulus at its first Mont128 call and the default has been "
              "changed since (scl_hip_mont128_set_prime on another thread); call scl_hip_mont128_set_prime or "
              "scl_hip_mont128_relatch on this thread to say which modulus it computes over");
}

Mont128::Ctx mont_ctx() {
  if (g_mont.p) return g_mont;
  std::lock_guard<std::mutex> lk(g_mont_default_mu);
  mont_latch_locked();
  return g_mont;
}

// (tu_config.hpp: the fields THIS translation unit instantiates kernels for)
int not_in_this_unit() { return fail(SCL_ERR_BAD_ARG, "field family not built into this translation unit"); }

template <class Fn>
int with_field(int field, Fn&& fn) {
  switch (field) {
    case SCL_M61:
      if constexpr (SCL_TU_HAS(0)) return fn(M61{}, M61::Ctx{});
      else return not_in_this_unit();
    case SCL_M127:
      if constexpr (SCL_TU_HAS(1)) return fn(M127{}, M127::Ctx{});
      else return not_in_this_unit();
    case SCL_MONT128:
      if constexpr (SCL_TU_HAS(2)) {
        SCL_TRY(mont_check());
        return fn(Mont128{}, mont_ctx());
      } else {
        return not_in_this_unit();
      }
    case SCL_GF2_128:
      if constexpr (SCL_TU_HAS(3)) return fn(Gf128{}, Gf128::Ctx{});
      else return not_in_this_unit();
    case SCL_SECP256K1_SCALAR:
      if constexpr (SCL_TU_HAS(4)) return fn(Secp256k1Scalar{}, Secp256k1Scalar::Ctx{});
      else return not_in_this_unit();
    case SCL_SECP256K1_FIELD:
      if constexpr (SCL_TU_HAS(5)) return fn(Secp256k1Field{}, Secp256k1Field::Ctx{});
      else return not_in_this_unit();
    default: return fail(SCL_ERR_BAD_ARG, "unknown field tag");
  }
}

// Rings Z2k<K> travel under the tag SCL_Z2K(K) = 0x100 + K.  Only the entry points that make sense in a ring
// dispatch through here (element-wise, reductions, randomness, additive sharing, matmul); the Shamir and
// Lagrange entry points stay on with_field and refuse ring tags, as division by node differences would.
inline bool is_ring(int field) { return field > 0x100 && field <= 0x100 + 128; }

template <class Fn>
int with_ring_or_field(int field, Fn&& fn) {
  if (is_ring(field)) {
    const int K = field - 0x100;
    if constexpr (SCL_TU_HAS(6)) {
      if (K <= 64) return fn(Z2k64{}, Z2k64::make_ctx(K));
      return fn(Z2k128{}, Z2k128::make_ctx(K));
    } else {
      return not_in_this_unit();
    }
  }
  return with_field(field, fn);
}

// ---- per-thread device scratch (only used by calls that synchronise before returning) -------------

int scratch(size_t bytes, void** out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (g_scratch.dev && (g_scratch.device != dev || g_scratch.bytes < bytes)) {
    (void)hipFree(g_scratch.dev);
    g_scratch = Scratch{};
  }
  if (!g_scratch.dev) {
    size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    HIP_TRY(hipMalloc(&g_scratch.dev, want));
    g_scratch.device = dev;
    g_scratch.bytes = want;
  }
  *out = g_scratch.dev;
  return SCL_OK;
}

// ---- per-thread device temporary for asynchronous calls ---------------------------------------------------
// A kernel-written temporary that outlives the call (the call returns before its kernels ran).  One buffer per
// host thread, kept and grown; an event recorded after the last use makes the next user -- possibly on another
// stream -- wait for it.  (hipMallocAsync / hipFreeAsync on the null stream proved unreliable under the ROCm 7.2
// runtime: a queue allocated that way lost writes between two kernels of one call.)

int temp_acquire(size_t bytes, hipStream_t st, void** out, int which = 0) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  TempArena& a = g_temps[which];
  if (a.dev && (a.device != dev || a.bytes < bytes)) {
    if (a.pending) HIP_TRY(hipEventSynchronize(a.done));
    (void)hipFree(a.dev);
    (void)hipEventDestroy(a.done);
    a = TempArena{};
  }
  if (!a.dev) {
    HIP_TRY(hipMalloc(&a.dev, bytes < (1u << 20) ? (1u << 20) : bytes));
    HIP_TRY(hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
    a.device = dev;
    a.bytes = bytes < (1u << 20) ? (1u << 20) : bytes;
  }
  if (a.pending) HIP_TRY(hipStreamWaitEvent(st, a.done, 0));
  *out = a.dev;
  return SCL_OK;
}

// An arena is kept for the thread's next call up to TEMP_RETAIN_BYTES; a larger one (the digit planes of a matrix product
// with both factors beyond ~4096 x 4096, or with K beyond 2^21: the planes grow with K, 512 bytes per 32-row tile and inner
// column) goes back when the call that grew it ends -- hipFree waits for that call's kernels, which run for milliseconds
// at such sizes; the retained arenas are what scl_hip_thread_cleanup frees.
constexpr size_t TEMP_RETAIN_BYTES = (size_t)1 << 30;

int temp_release(hipStream_t st, int which = 0) {
  TempArena& a = g_temps[which];
  if (a.dev && a.bytes > TEMP_RETAIN_BYTES) {
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(a.dev);
    (void)hipEventDestroy(a.done);
    a = TempArena{};
    return SCL_OK;
  }
  HIP_TRY(hipEventRecord(a.done, st));
  a.pending = true;
  return SCL_OK;
}

}  // namespace
