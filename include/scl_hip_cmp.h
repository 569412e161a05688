/* include/scl_hip_cmp.h -- exact comparison and truncation of Shamir sharings: the bitwise less-than.  The C ABI of
 * libscl_hip_cmp.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_fx.so, whose mask it starts from and whose shared random bits (libscl_hip_rb.so) it consumes.  Honest majority,
 * n > 2t.  p is the field's prime, |p| its bit length.  x stands for a signed integer in [-2^(k-1), 2^(k-1)); the caller supplies
 * B = k + kappa shared random bits [b_0] .. [b_(B-1)] per value.  With 1 <= w < k <= B <= |p| - 2:
 *
 *   1. [c] = [x] + 2^(k-1) + [r] and [r'] = sum_{i<w} 2^i [b_i]            scl_fx_trunc_mask with shift = w
 *   2. open c; c' = c mod 2^w AS AN INTEGER (as scl_fx_trunc_finish takes it).  Then x mod 2^w = c' - r' + 2^w [c' < r'].
 *   3. [c' < r'] from the public bits of c' and the shared bits [b_0 .. b_(w-1)], by a tree:
 *          leaf i     lt_i = (1 - c_i) b_i,  eq_i = c_i ? b_i : 1 - b_i     (linear: c_i is public)
 *          combine    lt = lt_hi + eq_hi lt_lo,  eq = eq_hi eq_lo
 *      scl_cmp_levels(w) levels halve the node count; the last needs lt only; a node without a partner combines with the
 *      identity (lt = 0, eq = 1).  Each level is one Damgard-Nielsen multiplication: scl_cmp_first_mask / scl_cmp_level_mask
 *      write [d]_2t = ... + [R]_2t, scl_hm_mul_finish (libscl_hip_hm.so) opens the whole level in one call and subtracts [R]_t.
 *      The first level works from the bit planes and c, fused with the opening of c.  Rounds: one for c, one per level.
 *      Double sharings: scl_cmp_planes(w) planes of N (119 for w = 59).
 *   4. a = c' - r' + 2^w lt, local:  x mod 2^w = a;  floor(x / 2^w) = (x - a) 2^-w, exactly;  with w = k - 1,
 *      [x < 0] = -(x - a) 2^-w.  [x < y] is the last form on x - y with one more bit of k.             scl_cmp_finish
 *
 * THE BIT PLANES are those of scl_hip_fx.h: plane i, row r at bits_dev + i * bits_plane_stride + r * bits_row_stride (elements);
 * the planes 0 .. w - 1 are read.
 *
 * THE NODE ARRAY.  Node j owns two planes: lt_j at plane 2j, eq_j at plane 2j + 1.  Plane q, row r lies at base + q * plane_stride +
 * r * row_stride (elements), N elements long.  With plane_stride = N, one scl_hm_mul_finish over 2 * nodes * N columns finishes a
 * level.  d_dev and r2_dev of one call are node arrays of the same node count: ceil(w / 2) nodes for the first level,
 * ceil(cnt / 2) for a later one.  Under SCL_CMP_LT_ONLY both are the one plane 0.
 *
 * THE STATUS of scl_cmp_first_mask, one byte per column, is that of scl_fx_trunc_finish: 1 where the opened c is at or above
 * 2^(B+1); such a column is computed as if c were 0, and scl_cmp_finish writes 0 in every row of it.  Best effort, as there.
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h and scl_hip_fx.h: SoA rows, strides in elements,
 * 8-byte alignment for one-limb elements and 16-byte alignment for wider ones, values canonical in and out, `stream` a
 * hipStream_t passed as void*.  Accepted tags: the five prime fields.  SCL_GF2_128 is refused ("GF(2^128) has no integers below
 * a prime: there are no bits of an opened value to compare") and so is a ring tag ("a ring Z2k is not a field: it has no 2^-w and
 * no Shamir sharing"), each with a message that names the reason.  SCL_MONT128 computes over the calling thread's modulus and
 * honours the latch rule documented at scl_hip_mont128_set_prime.
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown or refused tag, w == 0,
 * w >= B, B > |p| - 2, m outside 1..64, cnt < 2, an unknown flag or `what`, SCL_CMP_LT_ONLY where more than one node comes out
 * and a forbidden overlap are SCL_ERR_BAD_ARG; a stride smaller than N is SCL_ERR_SIZE_MISMATCH; no device SCL_ERR_NO_DEVICE.
 * N == 0 or rows == 0 returns SCL_OK at once.  A call allocates nothing, copies nothing and never synchronises: each can be
 * captured into a hipGraph from its first call on -- the constants travel as kernel arguments.
 */
#ifndef SCL_HIP_CMP_H
#define SCL_HIP_CMP_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_CMP_ABI_VERSION 1
int         scl_cmp_abi_version(void);          /* 1 */
const char* scl_cmp_last_error(void);           /* per thread, like scl_hip_last_error */

size_t scl_cmp_levels(size_t w);   /* max(1, ceil(log2 w)); 0 for w == 0 */
size_t scl_cmp_planes(size_t w);   /* double-sharing planes over all levels: per level 2*ceil(cnt/2), 1 for the last; 0 for w == 0 */

/* flags */
#define SCL_CMP_LT_ONLY 1u          /* last level: write plane 0 (lt) of the single output node only; the eq product is skipped */

/* `what` of scl_cmp_finish */
#define SCL_CMP_MOD   0             /* x mod 2^w */
#define SCL_CMP_TRUNC 1             /* floor(x / 2^w) */
#define SCL_CMP_LTZ   2             /* [x < 0], w = k - 1 */

/* Level 1, fused with the opening.  Per column c = sum_j lambda[j] csh[j][s] once (lambda_host: m canonical elements on the host,
 * 1 <= m <= 64; m == 1 with lambda = {1} for an already opened c); status[s] = 1 where c >= 2^(B+1), and such a column is
 * computed as if c were 0.  cmod[s] = c mod 2^w as a field element (N elements).  For each pair of bits (2j+1, 2j),
 * j < ceil(w/2), and each row, the combined node from the leaves + r2 -> d, a node array of ceil(w/2) nodes; bit w - 1 of an odd
 * w has no partner.  One lane per column (Mersenne61: two where bases and strides allow) walks its rows and pairs; the traffic is
 * (m + (w + 4 ceil(w/2)) rows + 1) N elements and N bytes.  SCL_CMP_LT_ONLY needs w <= 2.  No two operands may overlap. */
int scl_cmp_first_mask(int field, uint64_t* d_dev, size_t d_plane_stride, size_t d_row_stride,
                       uint64_t* cmod_dev, unsigned char* status_dev,
                       const uint64_t* csh_dev, size_t c_stride, const uint64_t* lambda_host, size_t m,
                       const uint64_t* bits_dev, size_t bits_plane_stride, size_t bits_row_stride,
                       const uint64_t* r2_dev, size_t r2_plane_stride, size_t r2_row_stride,
                       size_t w, size_t B, size_t rows, size_t N, unsigned flags, void* stream);

/* A later level: cnt >= 2 nodes in, ceil(cnt/2) out.  d = combine(node[2j+1], node[2j]) + r2; a lone last node + r2.  The traffic
 * is 8 rows N elements per pair.  SCL_CMP_LT_ONLY needs cnt == 2.  d_dev must not overlap nodes_dev or r2_dev. */
int scl_cmp_level_mask(int field, uint64_t* d_dev, size_t d_plane_stride, size_t d_row_stride,
                       const uint64_t* nodes_dev, size_t n_plane_stride, size_t n_row_stride,
                       const uint64_t* r2_dev, size_t r2_plane_stride, size_t r2_row_stride,
                       size_t cnt, size_t rows, size_t N, unsigned flags, void* stream);

/* a = cmod - rlow + 2^w lt; out = a (SCL_CMP_MOD), (x - a) 2^-w (SCL_CMP_TRUNC), -(x - a) 2^-w (SCL_CMP_LTZ).  A column whose
 * status is not 0 is 0 in every row.  out may be exactly x, rlow or lt with equal strides.  x may be NULL for SCL_CMP_MOD.  The
 * traffic is (4 rows + 1) N elements and N bytes.  w must be in 1..|p| - 3. */
int scl_cmp_finish(int field, uint64_t* out_dev, size_t out_stride, const uint64_t* lt_dev, size_t lt_stride,
                   const uint64_t* cmod_dev, const unsigned char* status_dev, const uint64_t* rlow_dev, size_t rlow_stride,
                   const uint64_t* x_dev, size_t x_stride, size_t w, int what, size_t rows, size_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_CMP_H */
