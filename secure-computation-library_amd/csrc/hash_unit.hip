// csrc/hash_unit.hip -- the SHA-256 / Merkle kernels that do not depend on a field, as a translation unit of their own: the
// units of capi.hip are compiled once per field family, and so is the one kernel here that sees elements (merkle_leaves.hip).
// Its entry points (scl_hip_sha256, scl_hip_merkle_depth .. _verify) are defined at the end; the leaf digests, the one step that
// depends on a field, are merkle_leaves.hip, compiled per family.
//
// Replaces scl::util::Sha256 (include/scl/util/sha256.h:33-67, iuf_hash.h:41-105) over batches and the loops of
// scl::util::MerkleTree (include/scl/util/merkle.h:74-181).  One lane computes one digest everywhere; a batch of T trees of L
// leaves is stored leaf-major, tree-minor -- node j of tree tau of a level at (j * T + tau) * 32 -- so that one index formula
// reads 64 contiguous bytes per lane for one long tree (T = 1) and neighbouring digests in neighbouring lanes for many short
// ones (the SoA share matrix: T = secrets, L = parties, no transpose).
#include <hip/hip_runtime.h>

#include "../../include/scl_hip.h"
#include "sha256.hpp"

namespace sclhip {
namespace {

constexpr int HBLOCK = 256;
#define SCL_HASH_STRIDE(q, n) \
  for (size_t q = (size_t)blockIdx.x * HBLOCK + threadIdx.x; q < (n); q += (size_t)gridDim.x * HBLOCK)

inline unsigned hash_grid(size_t items) {
  const size_t blocks = (items + HBLOCK - 1) / HBLOCK;
  return (unsigned)(blocks < 1 ? 1 : blocks > 0x7fffffffu ? 0x7fffffffu : blocks);
}

// `count` messages of msg_len bytes, message i at msgs + i * stride -> digest i at digests + i * 32.  Any length: the padding
// (0x80, zeros, the 64-bit bit length, FIPS 180-4 section 5.1.1) is produced on the fly, block by block.  ALIGNED: base and
// stride are multiples of four, whole words of the message are loaded as words.
template <bool ALIGNED>
__global__ __launch_bounds__(HBLOCK) void k_sha256_batch(unsigned char* digests, const unsigned char* msgs, size_t msg_len,
                                                         size_t stride, size_t count) {
  const size_t blocks = (msg_len + 9 + 63) / 64;
  SCL_HASH_STRIDE(i, count) {
    const unsigned char* m = msgs + i * stride;
    u32 st[8];
    sha256::init(st);
    for (size_t blk = 0; blk < blocks; ++blk) {
      u32 w[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const size_t at = blk * 64 + (size_t)j * 4;
        u32 v;
        if (ALIGNED && at + 4 <= msg_len) {
          v = __builtin_bswap32(*reinterpret_cast<const u32*>(m + at));
        } else {
          v = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const size_t p = at + b;
            const u32 byte = p < msg_len ? (u32)m[p] : p == msg_len ? 0x80u : 0u;
            v = (v << 8) | byte;
          }
        }
        w[j] = v;
      }
      if (blk + 1 == blocks) {
        const u64 bits = (u64)msg_len * 8;
        w[14] = (u32)(bits >> 32);
        w[15] = (u32)bits;
      }
      sha256::compress(st, w);
    }
    sha256::st_digest(digests + i * 32, st);
  }
}

// one level of T trees: node j of tree tau = SHA256(child 2j || child min(2j + 1, count - 1)) -- the clamp is the reference's
// "repeat the last digest" (merkle.h:85-89,112-116) without the copy
template <bool ONE_TREE>
__global__ __launch_bounds__(HBLOCK) void k_merkle_level(unsigned char* out, const unsigned char* in, size_t count, size_t T) {
  const size_t half = (count + 1) / 2, total = half * T;
  SCL_HASH_STRIDE(g, total) {
    const size_t j = ONE_TREE ? g : g / T, tau = ONE_TREE ? 0 : g - j * T;
    const size_t lj = 2 * j, rj = lj + 1 < count ? lj + 1 : count - 1;
    u32 l[8], r[8];
    sha256::ld_digest(l, in + (lj * T + tau) * 32);
    sha256::ld_digest(r, in + (rj * T + tau) * 32);
    sha256::node(l, l, r);
    sha256::st_digest(out + g * 32, l);
  }
}

// path[(l * k + q) * 32] = the sibling of query q's node at level l.  Indices from device memory are clamped (tree to T - 1,
// leaf to L - 1); NULL arrays select the regular pattern tree = q mod T, leaf = first_leaf + q / T.
__global__ __launch_bounds__(HBLOCK) void k_merkle_paths(unsigned char* path, const unsigned char* tree, size_t L, size_t T,
                                                         const u64* leaf_index, const u64* tree_index, size_t first_leaf, size_t k,
                                                         size_t depth) {
  const size_t total = k * depth;
  SCL_HASH_STRIDE(g, total) {
    const size_t level = g / k, q = g - level * k;
    size_t tau = tree_index ? (size_t)tree_index[q] : q % T;
    size_t leaf = leaf_index ? (size_t)leaf_index[q] : first_leaf + q / T;
    tau = tau < T ? tau : T - 1;
    leaf = leaf < L ? leaf : L - 1;
    size_t off = 0, count = L;
    for (size_t l = 0; l < level; ++l) {
      off += count * T;
      count = (count + 1) / 2;
    }
    const size_t j = leaf >> level, sib = (j ^ 1) < count ? (j ^ 1) : j;
    const u32x4* src = reinterpret_cast<const u32x4*>(tree + (off + sib * T + tau) * 32);
    u32x4* dst = reinterpret_cast<u32x4*>(path + g * 32);
    dst[0] = src[0];
    dst[1] = src[1];
  }
}

// MerkleTree::verify (merkle.h:165-181) per query: walk `depth` siblings up from the leaf digest, compare with the root.
// ok[q] = 1 iff the digests agree AND the query's indices were in range (leaf index below 2^depth, root index below
// num_roots); out-of-range indices are masked / clamped before use.  Every lane runs all `depth` levels: nothing here
// branches on the data.
__global__ __launch_bounds__(HBLOCK) void k_merkle_verify(unsigned char* ok, const unsigned char* leaf_digests, const u64* leaf_index,
                                                          size_t leaf, const unsigned char* path, size_t depth,
                                                          const unsigned char* roots, const u64* root_index, size_t num_roots,
                                                          size_t k) {
  SCL_HASH_STRIDE(q, k) {
    const u64 idx = leaf_index ? leaf_index[q] : (u64)leaf;
    u64 ri = root_index ? root_index[q] : (u64)(q % num_roots);
    u32 bad = (depth < 64 && (idx >> depth) != 0) | (ri >= num_roots);
    ri = ri < num_roots ? ri : num_roots - 1;
    u32 d[8], s[8], l[8], r[8];
    sha256::ld_digest(d, leaf_digests + q * 32);
    for (size_t level = 0; level < depth; ++level) {
      sha256::ld_digest(s, path + (level * k + q) * 32);
      const bool sib_left = level < 64 && ((idx >> level) & 1);
#pragma unroll
      for (int i = 0; i < 8; ++i) l[i] = sib_left ? s[i] : d[i], r[i] = sib_left ? d[i] : s[i];
      sha256::node(d, l, r);
    }
    sha256::ld_digest(s, roots + ri * 32);
    u32 diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= d[i] ^ s[i];
    ok[q] = (unsigned char)((diff == 0) & (bad == 0));
  }
}

}  // namespace

namespace {
hipError_t hash_launch_sha256(unsigned char* digests, const unsigned char* msgs, size_t msg_len, size_t msg_stride, size_t count,
                              hipStream_t st) {
  if (count == 0) return hipSuccess;
  const bool aligned = ((reinterpret_cast<uintptr_t>(msgs) | msg_stride) & 3) == 0;
  if (aligned) hipLaunchKernelGGL(k_sha256_batch<true>, dim3(hash_grid(count)), dim3(HBLOCK), 0, st, digests, msgs, msg_len, msg_stride, count);
  else hipLaunchKernelGGL(k_sha256_batch<false>, dim3(hash_grid(count)), dim3(HBLOCK), 0, st, digests, msgs, msg_len, msg_stride, count);
  return hipGetLastError();
}

hipError_t hash_launch_level(unsigned char* out, const unsigned char* in, size_t count, size_t T, hipStream_t st) {
  const size_t total = (count + 1) / 2 * T;
  if (total == 0) return hipSuccess;
  if (T == 1) hipLaunchKernelGGL(k_merkle_level<true>, dim3(hash_grid(total)), dim3(HBLOCK), 0, st, out, in, count, T);
  else hipLaunchKernelGGL(k_merkle_level<false>, dim3(hash_grid(total)), dim3(HBLOCK), 0, st, out, in, count, T);
  return hipGetLastError();
}

hipError_t hash_launch_paths(unsigned char* path, const unsigned char* tree, size_t L, size_t T, const u64* leaf_index,
                             const u64* tree_index, size_t first_leaf, size_t k, hipStream_t st) {
  const size_t depth = merkle_depth(L);
  if (k * depth == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merkle_paths, dim3(hash_grid(k * depth)), dim3(HBLOCK), 0, st, path, tree, L, T, leaf_index, tree_index,
                     first_leaf, k, depth);
  return hipGetLastError();
}

hipError_t hash_launch_verify(unsigned char* ok, const unsigned char* leaf_digests, const u64* leaf_index, size_t leaf,
                              const unsigned char* path, size_t depth, const unsigned char* roots, const u64* root_index,
                              size_t num_roots, size_t k, hipStream_t st) {
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(k_merkle_verify, dim3(hash_grid(k)), dim3(HBLOCK), 0, st, ok, leaf_digests, leaf_index, leaf, path, depth,
                     roots, root_index, num_roots, k);
  return hipGetLastError();
}
}  // namespace

}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
// The thread's last diagnostic and its temporary arenas (temp_acquire / temp_release on arena 0) are the engine's.
#include "engine_state.hpp"

namespace {
using namespace sclhip;

int merkle_shape_check(const char* what, size_t L, size_t T) {
  if (L == 0) return fail(SCL_ERR_BAD_ARG, std::string(what) + ": a tree has at least one leaf");
  if (T == 0) return fail(SCL_ERR_BAD_ARG, std::string(what) + ": no trees");
  if (scl_hip_merkle_tree_bytes(L, T) == 0) return fail(SCL_ERR_BAD_ARG, std::string(what) + ": L * T overflows");
  return SCL_OK;
}
}  // namespace

extern "C" {

int scl_hip_sha256(unsigned char* digests, const unsigned char* msgs, size_t msg_len, size_t msg_stride, size_t count,
                   void* stream) {
  if (count == 0) return SCL_OK;
  if (!digests || (msg_len && !msgs)) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(digests)) return fail(SCL_ERR_BAD_ARG, "digest buffer not 16-byte aligned");
  if (count > 1 && msg_stride < msg_len) return fail(SCL_ERR_SIZE_MISMATCH, "msg_stride < msg_len");
  SCL_TRY(alias_check("sha256", {sclhip::alias::vec("digests_dev", digests, count, 32, true), sclhip::alias::mat("msgs_dev", msgs, count, msg_stride, msg_len, 1, false)}));
  HIP_TRY(hash_launch_sha256(digests, msgs, msg_len, msg_stride, count, S(stream)));
  return SCL_OK;
}

size_t scl_hip_merkle_depth(size_t L) { return merkle_depth(L); }
size_t scl_hip_merkle_level_size(size_t L, size_t level) { return merkle_level_size(L, level); }
size_t scl_hip_merkle_tree_bytes(size_t L, size_t T) {
  const size_t nodes = merkle_tree_nodes(L);
  if (T && nodes > ((size_t)-1) / 32 / T) return 0;
  return nodes * T * 32;
}

int scl_hip_merkle_build(unsigned char* tree, const unsigned char* leaf_digests, size_t L, size_t T, void* stream) {
  SCL_TRY(merkle_shape_check("merkle_build", L, T));
  if (!tree || !leaf_digests) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(tree) || !aligned16(leaf_digests)) return fail(SCL_ERR_BAD_ARG, "digest buffer not 16-byte aligned");
  SCL_TRY(alias_check("merkle_build", {sclhip::alias::vec("tree_dev", tree, scl_hip_merkle_tree_bytes(L, T), 1, true, 1),
                                       sclhip::alias::vec("leaf_digests_dev", leaf_digests, L * T, 32, false, 1)}));
  if (leaf_digests != tree) HIP_TRY(hipMemcpyAsync(tree, leaf_digests, L * T * 32, hipMemcpyDeviceToDevice, S(stream)));
  unsigned char* in = tree;
  for (size_t count = L;; count = (count + 1) / 2) {
    unsigned char* out = in + count * T * 32;
    HIP_TRY(hash_launch_level(out, in, count, T, S(stream)));
    if ((count + 1) / 2 == 1) break;
    in = out;
  }
  return SCL_OK;
}

int scl_hip_merkle_root(unsigned char* roots, const unsigned char* leaf_digests, size_t L, size_t T, void* stream) {
  SCL_TRY(merkle_shape_check("merkle_root", L, T));
  if (!roots || !leaf_digests) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(roots) || !aligned16(leaf_digests)) return fail(SCL_ERR_BAD_ARG, "digest buffer not 16-byte aligned");
  SCL_TRY(alias_check("merkle_root", {sclhip::alias::vec("roots_dev", roots, T, 32, true), sclhip::alias::vec("leaf_digests_dev", leaf_digests, L * T, 32, false)}));
  // levels 1, 2, .. alternate between two regions of the thread's arena; the last one goes to `roots`
  const size_t n1 = (L + 1) / 2, n2 = (n1 + 1) / 2;
  if (n1 == 1) {
    HIP_TRY(hash_launch_level(roots, leaf_digests, L, T, S(stream)));
    return SCL_OK;
  }
  void* tmp = nullptr;
  SCL_TRY(temp_acquire((n1 + n2) * T * 32, S(stream), &tmp));
  unsigned char* buf[2] = {static_cast<unsigned char*>(tmp), static_cast<unsigned char*>(tmp) + n1 * T * 32};
  const unsigned char* in = leaf_digests;
  int which = 0;
  for (size_t count = L;; count = (count + 1) / 2) {
    const bool last = (count + 1) / 2 == 1;
    unsigned char* out = last ? roots : buf[which];
    HIP_TRY(hash_launch_level(out, in, count, T, S(stream)));
    if (last) break;
    in = out;
    which ^= 1;
  }
  return temp_release(S(stream));
}

int scl_hip_merkle_paths(unsigned char* path, const unsigned char* tree, size_t L, size_t T, const uint64_t* leaf_index,
                         const uint64_t* tree_index, size_t first_leaf, size_t k, void* stream) {
  SCL_TRY(merkle_shape_check("merkle_paths", L, T));
  if (k == 0) return SCL_OK;
  if (!path || !tree) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(path) || !aligned16(tree)) return fail(SCL_ERR_BAD_ARG, "digest buffer not 16-byte aligned");
  if (!leaf_index && (first_leaf >= L || (k - 1) / T >= L - first_leaf))
    return fail(SCL_ERR_INVALID_RANGE, "merkle_paths: leaf index >= L");
  SCL_TRY(alias_check("merkle_paths", {sclhip::alias::mat("path_dev", path, merkle_depth(L), k, k, 32, true),
                                       sclhip::alias::vec("tree_dev", tree, scl_hip_merkle_tree_bytes(L, T), 1, false),
                                       sclhip::alias::vec("leaf_index_dev", leaf_index, k, 8, false), sclhip::alias::vec("tree_index_dev", tree_index, k, 8, false)}));
  HIP_TRY(hash_launch_paths(path, tree, L, T, leaf_index, tree_index, first_leaf, k, S(stream)));
  return SCL_OK;
}

int scl_hip_merkle_verify(unsigned char* ok, const unsigned char* leaf_digests, const uint64_t* leaf_index, size_t leaf,
                          const unsigned char* path, size_t depth, const unsigned char* roots, const uint64_t* root_index,
                          size_t num_roots, size_t k, void* stream) {
  if (k == 0) return SCL_OK;
  if (!ok || !leaf_digests || !roots || (depth && !path)) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(leaf_digests) || !aligned16(roots) || !aligned16(path))
    return fail(SCL_ERR_BAD_ARG, "digest buffer not 16-byte aligned");
  if (num_roots == 0) return fail(SCL_ERR_BAD_ARG, "merkle_verify: no roots");
  if (depth > 64) return fail(SCL_ERR_BAD_ARG, "merkle_verify: depth > 64");
  if (!leaf_index && depth < 64 && (leaf >> depth) != 0) return fail(SCL_ERR_INVALID_RANGE, "merkle_verify: leaf index >= 2^depth");
  SCL_TRY(alias_check("merkle_verify", {sclhip::alias::vec("ok_dev", ok, k, 1, true), sclhip::alias::vec("leaf_digests_dev", leaf_digests, k, 32, false),
                                        sclhip::alias::vec("leaf_index_dev", leaf_index, k, 8, false), sclhip::alias::mat("path_dev", path, depth, k, k, 32, false),
                                        sclhip::alias::vec("roots_dev", roots, num_roots, 32, false), sclhip::alias::vec("root_index_dev", root_index, k, 8, false)}));
  HIP_TRY(hash_launch_verify(ok, leaf_digests, leaf_index, leaf, path, depth, roots, root_index, num_roots, k, S(stream)));
  return SCL_OK;
}

}  // extern "C"
