// csrc/ecdsa_unit.hip -- batched ECDSA over secp256k1 and the per-lane scalar multiplication it needs, a translation unit of
// its own beside ec_unit.hip (compiled once, for the same reason).
//
// Replaces util::ECDSA over batches (include/scl/util/sign.h:87-178: Sign, verify, conversionFunc, digestToElement for 32-byte
// digests) and EC::operator*(FF<Scalar>) over a vector of points (secp256k1_curve.cc:309-326).  The point and scalar functions
// are include/scl_hip/detail/secp256k1.hpp (shared with the host mirror, include/scl_hip/util/sign.h).  One lane owns one
// signature or point; blocks are one wave, loops around point functions stay rolled, as in ec_unit.hip.
//
// The per-lane window table of k_ec_mul / k_ecdsa_verify lives in caller-supplied scratch, [entry][slot][12] with slot = the
// thread's index in the grid: the 64 lanes of a wave write entry d side by side while they build it, and read 96 contiguous
// bytes each wherever their digits point.  The grid is capped so that the scratch is bounded (MUL_SLOTS_MAX slots of 1 536
// bytes); a lane reuses its slot for every item it strides over.  docs/kernels/ecdsa.md says why projective and why this order.
#include <hip/hip_runtime.h>

#include "../../include/scl_hip.h"
#include "../../include/scl_hip/detail/secp256k1.hpp"

namespace sclhip {
namespace {
using namespace secp;

#include "ec_common.hpp"  // EBLOCK, SCL_EC_STRIDE, ec_grid, raise_flag

constexpr size_t MUL_SLOTS_MAX = (size_t)1 << 17;  // 2 048 blocks: eight waves on each of 256 CUs
// slots of the window-table scratch a call over n items uses: a whole number of blocks
inline size_t mul_slots(size_t n) {
  const size_t s = (n + EBLOCK - 1) / EBLOCK * EBLOCK;
  return s < MUL_SLOTS_MAX ? s : MUL_SLOTS_MAX;
}

// dst[i] = scalars[i] * points[i].  The lane's table: scratch + slot * 12, entries gridDim.x * 64 * 12 limbs apart.
__global__ __launch_bounds__(EBLOCK) void k_ec_mul(u64* dst, const u64* points, const u64* scalars, u64* scratch, size_t n) {
  const size_t slots = (size_t)gridDim.x * EBLOCK;
  u64* table = scratch + ((size_t)blockIdx.x * EBLOCK + threadIdx.x) * POINT_LIMBS;
  SCL_EC_STRIDE(i, n) {
    const Fe k = scalar_plain(FR::ld(scalars + i * 4));
    const Point r = pt_mul_window(pt_load(points + i * POINT_LIMBS), k, table, slots * POINT_LIMBS);
    pt_store(dst + i * POINT_LIMBS, r);
  }
}

__global__ __launch_bounds__(EBLOCK) void k_ecdsa_conversion(u64* dst, const u64* points, size_t n) {
  SCL_EC_STRIDE(i, n) FR::st(dst + i * 4, ecdsa_conversion(pt_load(points + i * POINT_LIMBS)));
}

// (r, s) = (C(k G), k^-1 (h + sk r)).  k = 0: k G is infinity, so r = 0, and rinv(0) = 0, so s = 0 -- the lane writes (0, 0)
// by the same arithmetic as its neighbours and raises the flag.
__global__ __launch_bounds__(EBLOCK) void k_ecdsa_sign(u64* sig, const u64* gtable, const u64* sk, size_t sk_stride, const u64* nonces,
                                                       const unsigned char* digests, unsigned* status, size_t n) {
  SCL_EC_STRIDE(i, n) {
    const Fe k = FR::ld(nonces + i * 4);
    const Point R = pt_add_mul_table(pt_infinity(), gtable, scalar_plain(k));
    const Fe r = ecdsa_conversion(R);
    const Fe h = scalar_from_be32(digests + i * 32);
    const Fe s = rmul(rinv(k), FR::add(FR::Ctx{}, h, rmul(FR::ld(sk + i * sk_stride * 4), r)));
    FR::st(sig + i * 8, r);
    FR::st(sig + i * 8 + 4, s);
    if (FR::is_zero(k) && status) raise_flag(status);
  }
}

// the verdict of a lane whose R = u1 G + u2 Q is known: 2 for s == 0 (where the reference's inverse throws), else accepted or not
__device__ __forceinline__ unsigned char verdict(const Point& R, const Fe& r, const Fe& s) {
  const bool ok = pt_x_is(R, scalar_plain(r));
  return (unsigned char)(FR::is_zero(s) ? 2 : ok ? 1 : 0);
}

// verify (sign.h:135-146): u2 Q by the window ladder, then u1 G from the generator's table into the same accumulator.  The
// inversion of s is the lane's own (rinv), so a zero in one lane is nobody else's business: that lane computes with s^-1 = 0,
// gets infinity, and reports 2.
__global__ __launch_bounds__(EBLOCK) void k_ecdsa_verify(unsigned char* out, const u64* sig, const unsigned char* digests, const u64* pk,
                                                         size_t pk_stride, const u64* gtable, u64* scratch, size_t n) {
  const size_t slots = (size_t)gridDim.x * EBLOCK;
  u64* table = scratch + ((size_t)blockIdx.x * EBLOCK + threadIdx.x) * POINT_LIMBS;
  SCL_EC_STRIDE(i, n) {
    const Fe r = FR::ld(sig + i * 8), s = FR::ld(sig + i * 8 + 4);
    const Fe si = rinv(s);
    const Fe u1 = scalar_plain(rmul(scalar_from_be32(digests + i * 32), si));
    const Fe u2 = scalar_plain(rmul(r, si));
    Point R = pt_mul_window(pt_load(pk + i * pk_stride * POINT_LIMBS), u2, table, slots * POINT_LIMBS);
    R = pt_add_mul_table(R, gtable, u1);
    out[i] = verdict(R, r, s);
  }
}

// one signer: u2 Q from Q's own window table, 128 mixed additions and no ladder
__global__ __launch_bounds__(EBLOCK) void k_ecdsa_verify_base(unsigned char* out, const u64* sig, const unsigned char* digests,
                                                              const u64* qtable, const u64* gtable, size_t n) {
  SCL_EC_STRIDE(i, n) {
    const Fe r = FR::ld(sig + i * 8), s = FR::ld(sig + i * 8 + 4);
    const Fe si = rinv(s);
    const Fe u1 = scalar_plain(rmul(scalar_from_be32(digests + i * 32), si));
    const Fe u2 = scalar_plain(rmul(r, si));
    Point R = pt_add_mul_table(pt_infinity(), gtable, u1);
    R = pt_add_mul_table(R, qtable, u2);
    out[i] = verdict(R, r, s);
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

inline unsigned mul_grid(size_t n) { return (unsigned)(mul_slots(n) / EBLOCK); }
constexpr size_t PT_BYTES = POINT_LIMBS * sizeof(uint64_t);
}  // namespace

extern "C" {

size_t scl_hip_ec_mul_scratch_bytes(size_t n) { return mul_slots(n) * MUL_TABLE_ENTRIES * POINT_LIMBS * sizeof(uint64_t); }

int scl_hip_ec_mul(uint64_t* dst, const uint64_t* points, const uint64_t* scalars, void* scratch, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!dst || !points || !scalars || !scratch) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(dst) || !aligned16(points) || !aligned16(scalars) || !aligned16(scratch))
    return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  SCL_TRY(alias_check("ec_mul", {alias::vec("dst_dev", dst, n, PT_BYTES, true, 1), alias::vec("points_dev", points, n, PT_BYTES, false, 1),
                                 alias::vec("scalars_dev", scalars, n, 32, false), alias::vec("scratch_dev", scratch, scl_hip_ec_mul_scratch_bytes(n), 1, true)}));
  hipLaunchKernelGGL(k_ec_mul, dim3(mul_grid(n)), dim3(EBLOCK), 0, S(stream), dst, points, scalars, static_cast<u64*>(scratch), n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ecdsa_conversion(uint64_t* scalars, const uint64_t* points, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!scalars || !points) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(scalars) || !aligned16(points)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  SCL_TRY(alias_check("ecdsa_conversion", {alias::vec("scalars_dev", scalars, n, 32, true), alias::vec("points_dev", points, n, PT_BYTES, false)}));
  hipLaunchKernelGGL(k_ecdsa_conversion, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), scalars, points, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ecdsa_sign(uint64_t* sig, const void* gtable, const uint64_t* sk, size_t sk_stride, const uint64_t* nonces,
                       const unsigned char* digests, unsigned* status, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!sig || !gtable || !sk || !nonces || !digests) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(sig) || !aligned16(gtable) || !aligned16(sk) || !aligned16(nonces)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(status) & 3) return fail(SCL_ERR_BAD_ARG, "status_dev is not 4-byte aligned");
  if (sk_stride > 1) return fail(SCL_ERR_BAD_ARG, "ecdsa_sign: sk_stride is 0 (one key) or 1 (a key per signature)");
  SCL_TRY(alias_check("ecdsa_sign", {alias::vec("sig_dev", sig, n, 64, true), alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                     alias::vec("sk_dev", sk, sk_stride ? n : 1, 32, false), alias::vec("nonces_dev", nonces, n, 32, false),
                                     alias::vec("digests_dev", digests, n, 32, false), alias::vec("status_dev", status, 1, 4, true)}));
  hipLaunchKernelGGL(k_ecdsa_sign, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), sig, static_cast<const u64*>(gtable), sk, sk_stride,
                     nonces, digests, status, n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ecdsa_verify(unsigned char* verdict, const uint64_t* sig, const unsigned char* digests, const uint64_t* pk, size_t pk_stride,
                         const void* gtable, void* scratch, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!verdict || !sig || !digests || !pk || !gtable || !scratch) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(sig) || !aligned16(pk) || !aligned16(gtable) || !aligned16(scratch)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  if (pk_stride > 1) return fail(SCL_ERR_BAD_ARG, "ecdsa_verify: pk_stride is 0 (one key) or 1 (a key per signature)");
  SCL_TRY(alias_check("ecdsa_verify", {alias::vec("verdict_dev", verdict, n, 1, true), alias::vec("sig_dev", sig, n, 64, false),
                                       alias::vec("digests_dev", digests, n, 32, false), alias::vec("pk_dev", pk, pk_stride ? n : 1, PT_BYTES, false),
                                       alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false),
                                       alias::vec("scratch_dev", scratch, scl_hip_ec_mul_scratch_bytes(n), 1, true)}));
  hipLaunchKernelGGL(k_ecdsa_verify, dim3(mul_grid(n)), dim3(EBLOCK), 0, S(stream), verdict, sig, digests, pk, pk_stride,
                     static_cast<const u64*>(gtable), static_cast<u64*>(scratch), n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

int scl_hip_ecdsa_verify_base(unsigned char* verdict, const uint64_t* sig, const unsigned char* digests, const void* qtable,
                              const void* gtable, size_t n, void* stream) {
  if (n == 0) return SCL_OK;
  if (!verdict || !sig || !digests || !qtable || !gtable) return fail(SCL_ERR_BAD_ARG, "NULL operand");
  if (!aligned16(sig) || !aligned16(qtable) || !aligned16(gtable)) return fail(SCL_ERR_BAD_ARG, "buffer not 16-byte aligned");
  SCL_TRY(alias_check("ecdsa_verify_base", {alias::vec("verdict_dev", verdict, n, 1, true), alias::vec("sig_dev", sig, n, 64, false),
                                            alias::vec("digests_dev", digests, n, 32, false),
                                            alias::vec("qtable_dev", qtable, scl_hip_ec_base_table_bytes(), 1, false),
                                            alias::vec("gtable_dev", gtable, scl_hip_ec_base_table_bytes(), 1, false)}));
  hipLaunchKernelGGL(k_ecdsa_verify_base, dim3(ec_grid(n)), dim3(EBLOCK), 0, S(stream), verdict, sig, digests,
                     static_cast<const u64*>(qtable), static_cast<const u64*>(gtable), n);
  HIP_TRY(hipGetLastError());
  return SCL_OK;
}

}  // extern "C"
