// csrc/pedersen_unit.hip -- Pedersen VSS over secp256k1: two-base commitments, their verification and the point side of
// ss::apply, a translation unit of its own (compiled once, like ec_unit.hip and ecdsa_unit.hip).
//
// Replaces pedersenSecretShare's commitments (include/scl/ss/pedersen.h:140-146), pedersenVerify (pedersen.h:178-207) and the
// commitment half of ss::apply (pedersen.h:236-274) over batches of secrets.  The conventions are ec_unit.hip's: one lane owns
// one point, 64-lane blocks, grid-stride loops, rolled loops, the point functions of include/scl_hip/detail/secp256k1.hpp.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip.h"
#include "../../include/scl_hip/detail/secp256k1.hpp"

namespace sclhip {
namespace {
using namespace secp;

#include "ec_common.hpp"  // EBLOCK, SCL_EC_STRIDE, ec_grid, GRID_Y_MAX

// dst[row][i] = a[row][i] * G + b[row][i] * H from the two window tables: 128 mixed additions into one accumulator, no
// doubling.  A zero digit is pt_add_mul_table's select, so no lane branches on its scalars.  Every operand has a row stride of
// its own (in elements): the share matrix is committed to as it lies.
__global__ __launch_bounds__(EBLOCK) void k_ec_mul_two_base(u64* dst, size_t dst_stride, const u64* gtable, const u64* htable,
                                                            const u64* a, size_t a_stride, const u64* b, size_t b_stride, size_t n) {
  dst += (size_t)blockIdx.y * dst_stride * POINT_LIMBS;
  a += (size_t)blockIdx.y * a_stride * 4;
  b += (size_t)blockIdx.y * b_stride * 4;
  SCL_EC_STRIDE(i, n) {
    Point acc = pt_add_mul_table(pt_infinity(), gtable, scalar_plain(FR::ld(a + i * 4)));
    acc = pt_add_mul_table(acc, htable, scalar_plain(FR::ld(b + i * 4)));
    pt_store(dst + i * POINT_LIMBS, acc);
  }
}

// dst[i][c] (+)= sum_k M[i][k] * P[k][c], k < p <= MM_ROWS, i = blockIdx.y: k_ec_lincomb's Straus chain with a row of M for
// scalars -- taken out of Montgomery form once per block into LDS, the deciding word read into a scalar register --, started
// at the highest bit set anywhere in the row.  That bit comes from the OR of the row's words, gathered in LDS and read by
// every lane alike, so the trip count is uniform.  A row without a set bit writes infinity (or, accumulating, leaves dst as it
// is) and never enters the chain.
constexpr int MM_ROWS = 256;
__global__ __launch_bounds__(EBLOCK) void k_ec_matmul(u64* dst, size_t dst_stride, const u64* M, size_t m_stride, unsigned p,
                                                      const u64* points, size_t row_stride, size_t cols, int accumulate) {
  __shared__ u32 bits[MM_ROWS * 8];
  __shared__ u32 any[8];
  dst += (size_t)blockIdx.y * dst_stride * POINT_LIMBS;
  M += (size_t)blockIdx.y * m_stride * 4;
  if (threadIdx.x < 8) any[threadIdx.x] = 0;
  __syncthreads();
  for (unsigned k = threadIdx.x; k < p; k += EBLOCK) {
    const Fe v = scalar_plain(FR::ld(M + (size_t)k * 4));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u32 lo = (u32)v.w[j], hi = (u32)(v.w[j] >> 32);
      bits[k * 8 + 2 * j] = lo;
      bits[k * 8 + 2 * j + 1] = hi;
      if (lo) atomicOr(&any[2 * j], lo);
      if (hi) atomicOr(&any[2 * j + 1], hi);
    }
  }
  __syncthreads();
  int top = -1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u32 w = any[j];
    if (w) top = 32 * j + 31 - __clz(w);
  }
  top = __builtin_amdgcn_readfirstlane(top);
  if (top < 0) {
    if (!accumulate) SCL_EC_STRIDE(c, cols) pt_store(dst + c * POINT_LIMBS, pt_infinity());
    return;
  }
  SCL_EC_STRIDE(c, cols) {
    Point acc = pt_infinity();
#pragma unroll 1
    for (int bit = top; bit >= 0; --bit) {
      acc = pt_dbl(acc);
#pragma unroll 1
      for (unsigned k = 0; k < p; ++k) {
        const u32 word = __builtin_amdgcn_readfirstlane(bits[k * 8 + (bit >> 5)]);
        if ((word >> (bit & 31)) & 1u) acc = pt_add(acc, pt_load(points + ((size_t)k * row_stride + c) * POINT_LIMBS));
      }
    }
    if (accumulate) acc = pt_add(acc, pt_load(dst + c * POINT_LIMBS));
    pt_store(dst + c * POINT_LIMBS, acc);
  }
}

}  // namespace
}  // namespace sclhip

// ---- the entry points ------------------------------------------------------------------------------------------------------
#define SCL_UNIT_ENGINE
#include "unit_host.hpp"

namespace {
using namespace sclhip;
using namespace sclhip::secp;

constexpr size_t PT_BYTES = POINT_LIMBS * sizeof(uint64_t);

// rows of a * G + b * H; more rows than one grid holds go to further launches
int two_base_rows(u64* dst, size_t dst_stride, const void* gtable, const void* htable, const u64* a, size_t a_stride, const u64* b,
                  size_t b_stride, size_t rows, size_t n, hipStream_t st) {
  if (n == 0) return SCL_OK;
  for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
    const size_t r = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
    hipLaunchKernelGGL(k_ec_mul_two_base, dim3(ec_grid(n), (unsigned)r), dim3(EBLOCK), 0, st, dst + r0 * dst_stride * POINT_LIMBS,
                       dst_stride, static_cast<const u64*>(gtable), static_cast<const u64*>(htable), a + r0 * a_stride * 4, a_stride,
                       b + r0 * b_stride * 4, b_stride, n);
    HIP_TRY(hipGetLastError());
  }
  return SCL_OK;
}

// M [rows][p] times P [p][cols]: p beyond one launch's LDS goes to further launches that add to dst, rows beyond one grid to
// further launches of their own
int matmul_rows(u64* dst, size_t dst_stride, const u64* M, size_t rows, size_t p, const u64* points, size_t row_stride, size_t cols,
                hipStream_t st) {
  for (size_t k0 = 0; k0 < p; k0 += MM_ROWS) {
    const size_t pk = p - k0 < (size_t)MM_ROWS ? p - k0 : (size_t)MM_ROWS;
    for (size_t r0 = 0; r0 < rows; r0 += GRID_Y_MAX) {
      const size_t r = rows - r0 < GRID_Y_MAX ? rows - r0 : GRID_Y_MAX;
      hipLaunchKernelGGL(k_ec_matmul, dim3(ec_grid(cols), (unsigned)r), dim3(EBLOCK), 0, st, dst + r0 * dst_stride * POINT_LIMBS,
                         dst_stride, M + (r0 * p + k0) * 4, p, (unsigned)pk, points + k0 * row_stride * POINT_LIMBS, row_stride, cols,
                         k0 ? 1 : 0);
      HIP_TRY(hipGetLastError());
    }
  }
  return SCL_OK;
}
}  // namespace

extern "C" {

int scl_hip_ec_mul_two_base(uint64_t* dst, const void* gtable, const void* htable, const uint64_t* a, const uint64_t* b, size_t n,
                            void* stream) {
  if (n == 0) return SCL_OK;
  if (!dst || !gtable || !htable || !a || !b) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(dst) || !aligned16(gtable) || !aligned16(htable) || !aligned16(a) || !aligned16(b))
    return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_mul_two_base", {alias::vec("dst_dev", dst, n, PT_BYTES, true), alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                          alias::vec("htable_dev", htable, scl_hip_ec_base_table_bytes(), 1, false),
                                          alias::vec("a_dev", a, n, 32, false), alias::vec("b_dev", b, n, 32, false)}));
  return two_base_rows(dst, n, gtable, htable, a, n, b, n, 1, n, S(stream));
}

int scl_hip_ec_matmul(uint64_t* dst, size_t dst_stride, const uint64_t* M, size_t rows, size_t p, const uint64_t* points,
                      size_t row_stride, size_t cols, void* stream) {
  if (rows == 0 || cols == 0) return SCL_OK;
  if (p == 0) return fail(SCL_ERR_BAD_ARG, "ec_matmul: no rows of points");
  if (!dst || !M || !points) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(dst) || !aligned16(M) || !aligned16(points)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (rows > 1 && dst_stride < cols) return fail(SCL_ERR_SIZE_MISMATCH, "dst_stride < cols");
  if (p > 1 && row_stride < cols) return fail(SCL_ERR_SIZE_MISMATCH, "row_stride < cols");
  SCL_TRY(alias_check("ec_matmul", {alias::mat("dst_dev", dst, rows, dst_stride, cols, PT_BYTES, true), alias::mat("M_dev", M, rows, p, p, 32, false),
                                    alias::mat("points_dev", points, p, row_stride, cols, PT_BYTES, false)}));
  return matmul_rows(dst, dst_stride, M, rows, p, points, row_stride, cols, S(stream));
}

int scl_hip_pedersen_commit(uint64_t* commit, size_t commit_stride, const void* gtable, const void* htable, const uint64_t* secrets,
                            size_t secret_stride, const uint64_t* shares, size_t share_stride, size_t t, size_t n, size_t N,
                            void* stream) {
  if (N == 0) return SCL_OK;
  if (!commit || !gtable || !htable || !secrets || (t && !shares)) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(commit) || !aligned16(gtable) || !aligned16(htable) || !aligned16(secrets) || !aligned16(shares))
    return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (n < t) return fail(SCL_ERR_SIZE_MISMATCH, "pedersen_commit: n < t");
  if (t && commit_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "commit_stride < N");
  if (secret_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "secret_stride < N");
  if (t && share_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "share_stride < N");
  // (of the packed share matrix, rows 0 .. t - 1 and n .. n + t - 1 are read)
  SCL_TRY(alias_check("pedersen_commit", {alias::mat("commit_dev", commit, t + 1, commit_stride, N, PT_BYTES, true),
                                          alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                          alias::vec("htable_dev", htable, scl_hip_ec_base_table_bytes(), 1, false),
                                          alias::mat("secrets_dev", secrets, 2, secret_stride, N, 32, false),
                                          alias::mat("shares_dev", shares, t ? n + t : 0, share_stride, N, 32, false)}));
  SCL_TRY(two_base_rows(commit, commit_stride, gtable, htable, secrets, 0, secrets + secret_stride * 4, 0, 1, N, S(stream)));
  // component 0 of party k - 1 is row k - 1 of the packed matrix, component 1 is n rows further on
  return two_base_rows(commit + commit_stride * POINT_LIMBS, commit_stride, gtable, htable, shares, share_stride,
                       shares + n * share_stride * 4, share_stride, t, N, S(stream));
}

int scl_hip_pedersen_verify(unsigned char* ok, const uint64_t* share, const uint64_t* rand, const uint64_t* commit, size_t commit_stride,
                            size_t t, const uint64_t* lambda, const void* gtable, const void* htable, uint64_t* scratch, size_t N,
                            void* stream) {
  if (N == 0) return SCL_OK;
  if (!ok || !share || !rand || !commit || !lambda || !gtable || !htable || !scratch) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(share) || !aligned16(rand) || !aligned16(commit) || !aligned16(lambda) || !aligned16(gtable) || !aligned16(htable) ||
      !aligned16(scratch))
    return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (t && commit_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "commit_stride < N");
  SCL_TRY(alias_check("pedersen_verify", {alias::vec("ok_dev", ok, N, 1, true), alias::vec("share_dev", share, N, 32, false),
                                          alias::vec("rand_dev", rand, N, 32, false), alias::mat("commit_dev", commit, t + 1, commit_stride, N, PT_BYTES, false),
                                          alias::vec("lambda_dev", lambda, t + 1, 32, false),
                                          alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                          alias::vec("htable_dev", htable, scl_hip_ec_base_table_bytes(), 1, false),
                                          alias::vec("scratch_points_dev", scratch, 2 * N, PT_BYTES, true)}));
  uint64_t* lhs = scratch;
  uint64_t* rhs = scratch + N * POINT_LIMBS;
  // the sum over the commitments is the one-row case of the matrix product: lambda is its row
  SCL_TRY(matmul_rows(lhs, N, lambda, 1, t + 1, commit, commit_stride, N, S(stream)));
  SCL_TRY(two_base_rows(rhs, N, gtable, htable, share, N, rand, N, 1, N, S(stream)));
  return scl_hip_ec_equal(ok, lhs, rhs, N, stream);
}

}  // extern "C"
