// csrc/ec_unit.hip -- batched secp256k1 group arithmetic and Feldman VSS, a translation unit of its own (compiled once: the
// curve fixes both of its fields, nothing here depends on the field family of a capi.hip unit).
//
// Replaces math::EC<Secp256k1> over vectors (include/scl/math/ec.h, src/scl/math/curves/secp256k1_curve.cc) and
// feldmanSecretShare / feldmanVerify (include/scl/ss/feldman.h:107-163) over batches of secrets.  The point functions are
// include/scl_hip/detail/secp256k1.hpp (shared with the host mirror).  One lane owns one point everywhere.
//
// Layout: a point is 12 uint64_t (X, Y, Z, four Montgomery limbs each), arrays are [count][12].  These kernels are bound by
// vector issue by a wide margin -- a mixed addition is ~4,500 vector instructions against 96 + 64 bytes of traffic --, so the
// array-of-structures layout costs nothing measurable and is not tuned.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip.h"
#include "../../include/scl_hip/detail/secp256k1.hpp"

namespace sclhip {
namespace {
using namespace secp;

#include "ec_common.hpp"  // EBLOCK, SCL_EC_STRIDE, ec_grid

// Vector<EC> element-wise: a + b, a - b, -a, 2a
__global__ __launch_bounds__(EBLOCK) void k_ec_ew(int op, u64* dst, const u64* a, const u64* b, size_t n) {
  SCL_EC_STRIDE(i, n) {
    const Point p = pt_load(a + i * POINT_LIMBS);
    Point r;
    if (op == SCL_OP_ADD) r = pt_add(p, pt_load(b + i * POINT_LIMBS));
    else if (op == SCL_OP_SUB) r = pt_sub(p, pt_load(b + i * POINT_LIMBS));
    else if (op == SCL_OP_NEG) r = pt_neg(p);
    else r = pt_dbl(p);
    pt_store(dst + i * POINT_LIMBS, r);
  }
}

__global__ __launch_bounds__(EBLOCK) void k_ec_equal(unsigned char* eq, const u64* a, const u64* b, size_t n) {
  SCL_EC_STRIDE(i, n) eq[i] = pt_equal(pt_load(a + i * POINT_LIMBS), pt_load(b + i * POINT_LIMBS)) ? 1 : 0;
}

// The window table of a base point B: entry (w, d - 1), d = 1..15, is the affine d * 16^w * B.  One lane an entry, each on its
// own: 4w doublings, d - 1 additions, one Fermat inversion.  960 lanes of at most ~3,000 products; built once per base.
__global__ __launch_bounds__(EBLOCK) void k_ec_base_table(u64* table, Point base) {
  const unsigned e = blockIdx.x * EBLOCK + threadIdx.x;
  if (e >= WINDOWS * WINDOW_ENTRIES) return;
  const unsigned w = e / WINDOW_ENTRIES, d = e % WINDOW_ENTRIES + 1;
  Point p = base;
#pragma unroll 1
  for (unsigned i = 0; i < 4 * w; ++i) p = pt_dbl(p);
  Point r = p;
#pragma unroll 1
  for (unsigned i = 1; i < d; ++i) r = pt_add(r, p);
  const Affine a = pt_to_affine(r);
  FQ::st(table + (size_t)e * AFFINE_LIMBS, a.x);
  FQ::st(table + (size_t)e * AFFINE_LIMBS + 4, a.y);
}

// dst[row][i] = scalars[row][i] * B from B's window table: 64 mixed additions, no doubling.  A zero digit has no affine
// operand; the lane adds entry 1 of the window like the others and keeps its old sum (a select, not a branch).
__global__ __launch_bounds__(EBLOCK) void k_ec_mul_base(u64* dst, size_t dst_stride, const u64* table, const u64* scalars,
                                                        size_t src_stride, size_t n) {
  dst += (size_t)blockIdx.y * dst_stride * POINT_LIMBS;
  scalars += (size_t)blockIdx.y * src_stride * 4;
  SCL_EC_STRIDE(i, n) {
    const Fe k = scalar_plain(FR::ld(scalars + i * 4));
    Point acc = pt_infinity();
#pragma unroll 1
    for (int w = 0; w < WINDOWS; ++w) {
      const unsigned d = scalar_digit(k, w);
      const u64* ent = table + ((size_t)w * WINDOW_ENTRIES + (d ? d - 1 : 0)) * AFFINE_LIMBS;
      const Affine q{FQ::ld(ent), FQ::ld(ent + 4)};
      acc = pt_select(d != 0, pt_add_affine(acc, q), acc);
    }
    pt_store(dst + i * POINT_LIMBS, acc);
  }
}

// dst[i] (+)= sum_k scalars[k] * P[k][i], k < m <= LC_ROWS, the same m scalars for every lane.  One shared chain of 256
// doublings with the rows added in between (Straus).  The scalars are taken out of Montgomery form once per block into LDS;
// the bit that decides an addition is read into a scalar register, so the branch on it is uniform over the wave.
constexpr int LC_ROWS = 256;
__global__ __launch_bounds__(EBLOCK) void k_ec_lincomb(u64* dst, const u64* points, size_t row_stride, unsigned m,
                                                       const u64* scalars, size_t n, int accumulate) {
  __shared__ u32 bits[LC_ROWS * 8];
  for (unsigned k = threadIdx.x; k < m; k += EBLOCK) {
    const Fe v = scalar_plain(FR::ld(scalars + (size_t)k * 4));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bits[k * 8 + 2 * j] = (u32)v.w[j];
      bits[k * 8 + 2 * j + 1] = (u32)(v.w[j] >> 32);
    }
  }
  __syncthreads();
  SCL_EC_STRIDE(i, n) {
    Point acc = pt_infinity();
#pragma unroll 1
    for (int bit = 255; bit >= 0; --bit) {
      acc = pt_dbl(acc);
#pragma unroll 1
      for (unsigned k = 0; k < m; ++k) {
        const u32 word = __builtin_amdgcn_readfirstlane(bits[k * 8 + (bit >> 5)]);
        if ((word >> (bit & 31)) & 1u) acc = pt_add(acc, pt_load(points + ((size_t)k * row_stride + i) * POINT_LIMBS));
      }
    }
    if (accumulate) acc = pt_add(acc, pt_load(dst + i * POINT_LIMBS));
    pt_store(dst + i * POINT_LIMBS, acc);
  }
}

__global__ __launch_bounds__(EBLOCK) void k_ec_wire_pack(unsigned char* dst, const u64* points, size_t n) {
  SCL_EC_STRIDE(i, n) pt_write(dst + i * WIRE_BYTES, pt_load(points + i * POINT_LIMBS));
}

__global__ __launch_bounds__(EBLOCK) void k_ec_wire_unpack(u64* points, unsigned char* status, const unsigned char* src, size_t n) {
  SCL_EC_STRIDE(i, n) {
    Point p;
    status[i] = (unsigned char)pt_read(p, src + i * WIRE_BYTES);
    pt_store(points + i * POINT_LIMBS, p);
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

int mul_base_rows(u64* dst, size_t dst_stride, const void* table, const u64* scalars, size_t src_stride, size_t rows, size_t n,
                  hipStream_t st) {
  if (rows == 0 || n == 0) return SCL_OK;
  if (rows > 65535) return fail(SCL_ERR_BAD_ARG, "more than 65535 rows of scalars");
  hipLaunchKernelGGL(k_ec_mul_base, dim3(ec_grid(n), (unsigned)rows), dim3(EBLOCK), 0, st, dst, dst_stride,
                     static_cast<const u64*>(table), scalars, src_stride, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int lincomb_rows(u64* dst, const u64* points, size_t row_stride, size_t m, const u64* scalars, size_t n, hipStream_t st) {
  // more rows than one launch recodes: further launches add their part to dst
  for (size_t k0 = 0; k0 < m; k0 += LC_ROWS) {
    const size_t rows = m - k0 < (size_t)LC_ROWS ? m - k0 : (size_t)LC_ROWS;
    hipLaunchKernelGGL(k_ec_lincomb, dim3(ec_grid(n)), dim3(EBLOCK), 0, st, dst, points + k0 * row_stride * POINT_LIMBS, row_stride,
                       (unsigned)rows, scalars + k0 * 4, n, k0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
  }
  return SCL_OK;
}
}  // namespace

extern "C" {

int scl_hip_ec_generator(uint64_t point_host[12]) {
  if (!point_host) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  pt_store(point_host, pt_generator());
  return SCL_OK;
}

int scl_hip_ec_ew(int op, uint64_t* dst, const uint64_t* a, const uint64_t* b, size_t n, void* stream) {
  const bool binary = op == SCL_OP_ADD || op == SCL_OP_SUB;
  if (!binary && op != SCL_OP_NEG && op != SCL_EC_OP_DBL) return fail(SCL_ERR_BAD_ARG, "ec_ew: op is not ADD, SUB, NEG or DBL");
  if (n == 0) return SCL_OK;
  if (!dst || !a || (binary && !b)) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(dst) || !aligned16(a) || !aligned16(b)) return fail(SCL_ERR_BAD_ARG, "point buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_ew", {alias::vec("dst_dev", dst, n, PT_BYTES, true, 1), alias::vec("a_dev", a, n, PT_BYTES, false, 1),
                                alias::vec("b_dev", binary ? b : nullptr, n, PT_BYTES, false, 1)}));
  hipLaunchKernelGGL(k_ec_ew, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), op, dst, a, b, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ec_equal(unsigned char* eq, const uint64_t* a, const uint64_t* b, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!eq || !a || !b) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(a) || !aligned16(b)) return fail(SCL_ERR_BAD_ARG, "point buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_equal", {alias::vec("eq_dev", eq, n, 1, true), alias::vec("a_dev", a, n, PT_BYTES, false), alias::vec("b_dev", b, n, PT_BYTES, false)}));
  hipLaunchKernelGGL(k_ec_equal, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), eq, a, b, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

size_t scl_hip_ec_base_table_bytes(void) { return (size_t)WINDOWS * WINDOW_ENTRIES * AFFINE_LIMBS * sizeof(uint64_t); }

int scl_hip_ec_base_table(void* table, const uint64_t base_host[12], void* stream) {
  if (!table || !base_host) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(table)) return fail(SCL_ERR_BAD_ARG, "base table not 16-byte aligned");
  const Point base = pt_load(base_host);
  if (pt_is_infinity(base)) return fail(SCL_ERR_BAD_ARG, "ec_base_table: the base is the point at infinity");
  hipLaunchKernelGGL(k_ec_base_table, dim3(WINDOWS * WINDOW_ENTRIES / EBLOCK), dim3(EBLOCK), 0, S(stream),
                     static_cast<u64*>(table), base);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ec_mul_base(uint64_t* dst, const void* table, const uint64_t* scalars, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!dst || !table || !scalars) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(dst) || !aligned16(table) || !aligned16(scalars)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_mul_base", {alias::vec("dst_dev", dst, n, PT_BYTES, true), alias::vec("table_dev", table, scl_hip_ec_base_table_bytes(), 1, false),
                                      alias::vec("scalars_dev", scalars, n, 32, false)}));
  return mul_base_rows(dst, n, table, scalars, n, 1, n, S(stream));
}

int scl_hip_ec_lincomb(uint64_t* dst, const uint64_t* points, size_t row_stride, size_t m, const uint64_t* scalars, size_t n,
                       void* stream) {
  if (n == 0) return SCL_OK;
  if (m == 0) return fail(SCL_ERR_BAD_ARG, "ec_lincomb: no rows");
  if (!dst || !points || !scalars) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(dst) || !aligned16(points) || !aligned16(scalars)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (m > 1 && row_stride < n) return fail(SCL_ERR_SIZE_MISMATCH, "row_stride < n");
  // (m > 256 takes a second launch that adds to dst: a dst on a later row of points is read after it was written)
  SCL_TRY(alias_check("ec_lincomb", {alias::vec("dst_dev", dst, n, PT_BYTES, true), alias::mat("points_dev", points, m, row_stride, n, PT_BYTES, false),
                                     alias::vec("scalars_dev", scalars, m, 32, false)}));
  return lincomb_rows(dst, points, row_stride, m, scalars, n, S(stream));
}

int scl_hip_ec_wire_pack(unsigned char* dst, const uint64_t* points, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!dst || !points) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(points)) return fail(SCL_ERR_BAD_ARG, "point buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_wire_pack", {alias::vec("dst_dev", dst, n, WIRE_BYTES, true), alias::vec("points_dev", points, n, PT_BYTES, false)}));
  hipLaunchKernelGGL(k_ec_wire_pack, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), dst, points, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ec_wire_unpack(uint64_t* points, unsigned char* status, const unsigned char* src, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!points || !status || !src) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(points)) return fail(SCL_ERR_BAD_ARG, "point buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_wire_unpack", {alias::vec("points_dev", points, n, PT_BYTES, true), alias::vec("status_dev", status, n, 1, true),
                                         alias::vec("src_dev", src, n, WIRE_BYTES, false)}));
  hipLaunchKernelGGL(k_ec_wire_unpack, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), points, status, src, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_feldman_commit(uint64_t* commit, size_t commit_stride, const void* gtable, const uint64_t* secrets,
                           const uint64_t* shares, size_t share_stride, size_t t, size_t N, void* stream) {
  if (N == 0) return SCL_OK;
  if (!commit || !gtable || !secrets || (t && !shares)) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(commit) || !aligned16(gtable) || !aligned16(secrets) || !aligned16(shares))
    return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (t && commit_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "commit_stride < N");
  if (t > 1 && share_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "share_stride < N");
  SCL_TRY(alias_check("feldman_commit", {alias::mat("commit_dev", commit, t + 1, commit_stride, N, PT_BYTES, true),
                                         alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                         alias::vec("secrets_dev", secrets, N, 32, false), alias::mat("shares_dev", shares, t, share_stride, N, 32, false)}));
  SCL_TRY(mul_base_rows(commit, commit_stride, gtable, secrets, N, 1, N, S(stream)));
  return mul_base_rows(commit + commit_stride * POINT_LIMBS, commit_stride, gtable, shares, share_stride, t, N, S(stream));
}

int scl_hip_feldman_verify(unsigned char* ok, const uint64_t* share, const uint64_t* commit, size_t commit_stride, size_t t,
                           const uint64_t* lambda, const void* gtable, uint64_t* scratch, size_t N, void* stream) {
  if (N == 0) return SCL_OK;
  if (!ok || !share || !commit || !lambda || !gtable || !scratch) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(share) || !aligned16(commit) || !aligned16(lambda) || !aligned16(gtable) || !aligned16(scratch))
    return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (t && commit_stride < N) return fail(SCL_ERR_SIZE_MISMATCH, "commit_stride < N");
  SCL_TRY(alias_check("feldman_verify", {alias::vec("ok_dev", ok, N, 1, true), alias::vec("share_dev", share, N, 32, false),
                                         alias::mat("commit_dev", commit, t + 1, commit_stride, N, PT_BYTES, false),
                                         alias::vec("lambda_dev", lambda, t + 1, 32, false),
                                         alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                         alias::vec("scratch_points_dev", scratch, 2 * N, PT_BYTES, true)}));
  uint64_t* lhs = scratch;
  uint64_t* rhs = scratch + N * POINT_LIMBS;
  SCL_TRY(lincomb_rows(lhs, commit, commit_stride, t + 1, lambda, N, S(stream)));
  SCL_TRY(mul_base_rows(rhs, N, gtable, share, N, 1, N, S(stream)));
  hipLaunchKernelGGL(k_ec_equal, dim3(ec_grid(N)), dim3(EBLOCK), 0, S(stream), ok, lhs, rhs, N);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

}  // extern "C"
