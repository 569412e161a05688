// csrc/merkle_leaves.hip -- leaf digests of a Merkle tree over field elements, the one field-dependent step of the commitment
// path; compiled once per field family like capi.hip (tu_config.hpp, Makefile) and routed by field tag (capi_route.cc).
//
// MerkleTree::hashLeafs (include/scl/util/merkle.h:74-92): digest = HASH{}.update(leaf).finalize() with
// Serializer<FF>::write = ff::toBytes (ff.h:355-391) -- SHA-256 of exactly the bytes k_wire_pack stores for the element
// (kernels.hpp; tests/test_gpu_merkle.py holds the two together for every field): the value little-endian for the Mersenne
// fields and GF(2^128), out of Montgomery form and big-endian for Mont128 and the secp256k1 fields.  The conversions are the
// fields' own (detail/field.hpp: from_mont, to_be_image); an element is at most 32 bytes, one compression (sha256.hpp).
#include <hip/hip_runtime.h>

#include "tu_config.hpp"
#if SCL_TU_FIELDS != 0xff
#include "capi_names.inc"  // this unit's name for scl_hip_merkle_leaves
#endif
#include "../../include/scl_hip.h"
#include "../../include/scl_hip/detail/field.hpp"
#include "kernels.hpp"
#include "sha256.hpp"

using namespace sclhip;

namespace sclhip {
// the 2 * LIMBS 32-bit words of FF::write's image of element `se`, as they lie in memory
template <class F>
__device__ __forceinline__ void leaf_image(const typename F::Ctx& ctx, const u64* src, size_t se, u32 (&o)[2 * F::LIMBS]) {
  if constexpr (F::LIMBS == 1) {
    const u64 v = src[se];
    o[0] = (u32)v;
    o[1] = (u32)(v >> 32);
  } else if constexpr (F::LIMBS == 2) {
    u128 v = F::ld(src + 2 * se);
    if constexpr (F::TAG == 2) v = bswap128(F::from_mont(ctx, v));  // Montgomery family: value, big-endian
    o[0] = (u32)v;
    o[1] = (u32)(v >> 32);
    o[2] = (u32)(v >> 64);
    o[3] = (u32)(v >> 96);
  } else {
    const typename F::E img = F::to_be_image(ctx, F::ld(src + 4 * se));  // montyToBytes
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = (u32)img.w[j];
      o[2 * j + 1] = (u32)(img.w[j] >> 32);
    }
  }
}

// a rows x cols window with a row stride; digest of element (row, col) at (row * cols + col) * 32
template <class F>
__global__ __launch_bounds__(BLOCK) void k_merkle_leaves(typename F::Ctx ctx, unsigned char* digests, const u64* src, size_t stride,
                                                         size_t cols, size_t n) {
  SCL_GRID_STRIDE(e, n) {
    u32 w[2 * F::LIMBS], st[8];
    leaf_image<F>(ctx, src, stride == cols ? e : (e / cols) * stride + e % cols, w);
    sha256::short_message<2 * F::LIMBS>(st, w);
    sha256::st_digest(digests + e * 32, st);
  }
}
}  // namespace sclhip

// the field dispatch, the Mont128 latch rule and fail / alias_check: the engine's
#include "engine_state.hpp"

namespace {
template <class F>
int launch(const typename F::Ctx& ctx, unsigned char* digests, const uint64_t* a, size_t stride, size_t cols, size_t n, void* stream) {
  if (reinterpret_cast<uintptr_t>(a) & (F::LIMBS == 1 ? 7 : 15)) return fail(SCL_ERR_BAD_ARG, "element buffer misaligned");
  const size_t blocks = (n + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL((k_merkle_leaves<F>), dim3((unsigned)(blocks > 0x7fffffffu ? 0x7fffffffu : blocks)), dim3(BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), ctx, digests, a, stride, cols, n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e == hipErrorNoDevice ? SCL_ERR_NO_DEVICE : SCL_ERR_HIP, std::string("k_merkle_leaves: ") + hipGetErrorString(e));
  return SCL_OK;
}
}  // namespace

extern "C" int scl_hip_merkle_leaves(int field, unsigned char* digests, const uint64_t* a, size_t stride, size_t rows, size_t cols,
                                     void* stream) {
  const size_t n = rows * cols;
  if (n == 0) return SCL_OK;
  if (!digests || !a) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (reinterpret_cast<uintptr_t>(digests) & 15) return fail(SCL_ERR_BAD_ARG, "digest buffer not 16-byte aligned");
  if (n / cols != rows) return fail(SCL_ERR_BAD_ARG, "rows * cols overflows");
  if (stride < cols) return fail(SCL_ERR_SIZE_MISMATCH, "stride < cols");
  if (const int L = scl_hip_limbs(field); L > 0)
    if (const int s = alias_check("merkle_leaves", {sclhip::alias::vec("digests_dev", digests, n, 32, true),
                                                    sclhip::alias::mat("a_dev", a, rows, stride, cols, (size_t)L * 8, false)});
        s != SCL_OK)
      return s;
  // (with_field refuses the rings SCL_Z2K(K) too: the reference has no Serializer<Z2k>; Mont128 computes over the calling thread's
  // modulus, latched at first use, and not silently once the default it latched has been replaced: mont_check)
  return with_field(field, [&](auto f, auto ctx) -> int { return launch<decltype(f)>(ctx, digests, a, stride, cols, n, stream); });
}
