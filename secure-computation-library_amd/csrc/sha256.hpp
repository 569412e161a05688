// csrc/sha256.hpp -- SHA-256 (FIPS 180-4) for gfx950, one hash per lane, everything in registers.
//
// scl::util::Sha256 (include/scl/util/sha256.h:33-67, src/scl/util/sha256.cc) hashes on the host, a byte at a time into a 64-byte
// chunk.  Here a lane holds the eight state words, and the message schedule as a rolling window of sixteen words: word t of the
// schedule overwrites word t - 16, the 64 rounds are unrolled so that every index and every round constant is an immediate.
//   rotate        one funnel shift (v_alignbit_b32 of a word with itself)
//   Ch, Maj       one three-input bit operation each (v_bitop3_b32; table bit 4a + 2b + c, tools/bitop3_probe.hip)
//   Sigma, sigma  the three-way xor of the rotations, one v_bitop3_b32
// A tree node SHA256(left || right) is 64 bytes of data and one block of nothing but padding; the schedule of that second block
// is a constant, so it is folded into the round constants (KPAD below) and the second compression does no schedule work.
// Digests travel as the eight state words (big-endian words of the digest bytes); ld_digest / st_digest swap at the boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sclhip {

typedef uint32_t u32;
typedef uint64_t u64;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

namespace sha256 {

struct Table {
  u32 v[64];
};

constexpr Table K = {{
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2}};

constexpr u32 IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

constexpr u32 c_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }

// K[t] + W[t] of the block that follows 64 bytes of data: 0x80, zeros, the bit length 512
constexpr Table pad_block_constants() {
  u32 w[64] = {};
  w[0] = 0x80000000u;
  w[15] = 512;
  for (int t = 16; t < 64; ++t) {
    const u32 s0 = c_rotr(w[t - 15], 7) ^ c_rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
    const u32 s1 = c_rotr(w[t - 2], 17) ^ c_rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
    w[t] = w[t - 16] + s0 + w[t - 7] + s1;
  }
  Table r = {};
  for (int t = 0; t < 64; ++t) r.v[t] = K.v[t] + w[t];
  return r;
}
constexpr Table KPAD = pad_block_constants();

__device__ __forceinline__ u32 rotr(u32 x, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(x, x, n);
#else
  return (x >> n) | (x << (32 - n));
#endif
}
template <int TABLE>
__device__ __forceinline__ u32 bit3(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, TABLE);
#else
  u32 r = 0;  // (host pass of the compiler only: never called there)
  for (int i = 0; i < 32; ++i) r |= ((TABLE >> ((((a >> i) & 1) << 2) | (((b >> i) & 1) << 1) | ((c >> i) & 1))) & 1u) << i;
  return r;
#endif
}
__device__ __forceinline__ u32 x3(u32 a, u32 b, u32 c) { return bit3<0x96>(a, b, c); }
__device__ __forceinline__ u32 ch(u32 e, u32 f, u32 g) { return bit3<0xCA>(e, f, g); }   // e ? f : g
__device__ __forceinline__ u32 maj(u32 a, u32 b, u32 c) { return bit3<0xE8>(a, b, c); }  // two or more of three
__device__ __forceinline__ u32 big0(u32 a) { return x3(rotr(a, 2), rotr(a, 13), rotr(a, 22)); }
__device__ __forceinline__ u32 big1(u32 e) { return x3(rotr(e, 6), rotr(e, 11), rotr(e, 25)); }
__device__ __forceinline__ u32 small0(u32 x) { return x3(rotr(x, 7), rotr(x, 18), x >> 3); }
__device__ __forceinline__ u32 small1(u32 x) { return x3(rotr(x, 17), rotr(x, 19), x >> 10); }

#define SCL_SHA_ROUND(KW)                                     \
  {                                                           \
    const u32 t1 = h + big1(e) + ch(e, f, g) + (KW);          \
    const u32 t2 = big0(a) + maj(a, b, c);                    \
    h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2; \
  }

// one block: st += compress(st, w); w (the block's sixteen big-endian words) is consumed as the schedule window
__device__ __forceinline__ void compress(u32 (&st)[8], u32 (&w)[16]) {
  u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) w[t & 15] += small1(w[(t - 2) & 15]) + w[(t - 7) & 15] + small0(w[(t - 15) & 15]);
    SCL_SHA_ROUND(K.v[t] + w[t & 15]);
  }
  st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}

// the padding block behind 64 bytes of data: schedule folded into the constants
__device__ __forceinline__ void compress_pad64(u32 (&st)[8]) {
  u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) SCL_SHA_ROUND(KPAD.v[t]);
  st[0] += a, st[1] += b, st[2] += c, st[3] += d, st[4] += e, st[5] += f, st[6] += g, st[7] += h;
}
#undef SCL_SHA_ROUND

__device__ __forceinline__ void init(u32 (&st)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = IV[i];
}

// out = SHA256(left || right), digests as state words; out may be left or right
__device__ __forceinline__ void node(u32 (&out)[8], const u32 (&left)[8], const u32 (&right)[8]) {
  u32 w[16], st[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = left[i], w[8 + i] = right[i];
  init(st);
  compress(st, w);
  compress_pad64(st);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = st[i];
}

// SHA256 of a message of WORDS * 4 <= 32 bytes given as the 32-bit little-endian words of its memory image (what the wire
// kernels store): one block
template <int WORDS>
__device__ __forceinline__ void short_message(u32 (&st)[8], const u32 (&image)[WORDS]) {
  static_assert(WORDS <= 8, "one block");
  u32 w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = i < WORDS ? __builtin_bswap32(image[i]) : i == WORDS ? 0x80000000u : i == 15 ? WORDS * 32u : 0u;
  init(st);
  compress(st, w);
}

// a digest in memory (32 bytes, 16-byte aligned) <-> state words
__device__ __forceinline__ void ld_digest(u32 (&d)[8], const unsigned char* p) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(p), hi = *reinterpret_cast<const u32x4*>(p + 16);
  d[0] = __builtin_bswap32(lo.x), d[1] = __builtin_bswap32(lo.y), d[2] = __builtin_bswap32(lo.z), d[3] = __builtin_bswap32(lo.w);
  d[4] = __builtin_bswap32(hi.x), d[5] = __builtin_bswap32(hi.y), d[6] = __builtin_bswap32(hi.z), d[7] = __builtin_bswap32(hi.w);
}
__device__ __forceinline__ void st_digest(unsigned char* p, const u32 (&d)[8]) {
  u32x4 lo, hi;
  lo.x = __builtin_bswap32(d[0]), lo.y = __builtin_bswap32(d[1]), lo.z = __builtin_bswap32(d[2]), lo.w = __builtin_bswap32(d[3]);
  hi.x = __builtin_bswap32(d[4]), hi.y = __builtin_bswap32(d[5]), hi.z = __builtin_bswap32(d[6]), hi.w = __builtin_bswap32(d[7]);
  *reinterpret_cast<u32x4*>(p) = lo;
  *reinterpret_cast<u32x4*>(p + 16) = hi;
}

}  // namespace sha256

// The reference's tree (include/scl/util/merkle.h:74-120): the leaf level is padded to an even count by repeating its last
// digest (one leaf included), and so is every later level of odd size greater than one.  Repeating the last node is reading it
// twice, so a level keeps its REAL count here -- level 0 has L nodes, level l + 1 has ceil(count(l) / 2) -- and the right child's
// index is clamped to the last node.  depth = levels above the leaves = max(1, ceil(log2 L)).
inline size_t merkle_level_size(size_t L, size_t level) {
  size_t r = L;
  for (size_t l = 0; l < level && r; ++l) r = (l > 0 && r == 1) ? 0 : (r + 1) / 2;
  return r;
}
inline size_t merkle_depth(size_t L) {
  if (L == 0) return 0;
  size_t depth = 1;
  for (size_t r = (L + 1) / 2; r > 1; r = (r + 1) / 2) ++depth;
  return depth;
}
// nodes of all levels, leaves included
inline size_t merkle_tree_nodes(size_t L) {
  if (L == 0) return 0;
  size_t total = L, r = L;
  do {
    r = (r + 1) / 2;
    total += r;
  } while (r > 1);
  return total;
}

}  // namespace sclhip
