// csrc/ec_common.hpp -- the launch conventions of the three curve units (ec_unit.hip, ecdsa_unit.hip, pedersen_unit.hip): one
// lane owns one point, blocks are one wave, kernels grid-stride.  Included inside each unit's `namespace sclhip { namespace {`.
#pragma once

// 64 lanes a block: one wave, and the whole register file of a SIMD lane is open to the compiler (no spilling at the price of
// occupancy, which a kernel that waits for nothing but its own multiplier does not need much of)
constexpr int EBLOCK = 64;
#define SCL_EC_STRIDE(q, n) \
  for (size_t q = (size_t)blockIdx.x * EBLOCK + threadIdx.x; q < (n); q += (size_t)gridDim.x * EBLOCK)

inline unsigned ec_grid(size_t items) {
  const size_t blocks = (items + EBLOCK - 1) / EBLOCK;
  return (unsigned)(blocks < 1 ? 1 : blocks > 0x7fffffffu ? 0x7fffffffu : blocks);
}
constexpr size_t GRID_Y_MAX = 65535;  // rows one launch takes along y: the sites chunk by it

// as raise_flag of kernels.hpp: the only bit anyone sets in the word is this one, so a plain store of 1 is the OR
__device__ __forceinline__ void raise_flag(unsigned* flag) {
  if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0)
    __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
