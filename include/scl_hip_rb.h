/* include/scl_hip_rb.h -- random shared bits over the engine of scl_hip.h: the C ABI of libscl_hip_rb.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_hm.so.  Comparison, truncation, bit decomposition and fixed-point arithmetic over Shamir sharings consume shared
 * random bits; the honest-majority construction of one is ([r]_d = a degree-d sharing)
 *
 *   1. take a random [r]_t                                         scl_hm_double_share_prg, scl_hm_apply
 *   2. square it: [r^2]_2t + [R]_2t                                scl_hm_mul_mask (x = y = r), scl_hm_mul_finish
 *   3. open u = r^2                                                scl_hip_shamir_recover
 *   4. v = 1 / sqrt(u)                                             scl_rb_sqrt
 *   5. [b]_t = (v [r]_t + 1) / 2                                   scl_rb_bits_finish: steps 4 and 5 in one launch
 *
 * r / sqrt(r^2) is 1 or -1 with equal probability and nobody learns which: b is 0 or 1.  r = 0 (probability 1/p) has no bit;
 * the column's status byte says so and the caller discards it.
 *
 * THE ALGORITHM is one for every prime field (include/scl_hip/detail/rb.hpp): with p - 1 = 2^s q, q odd,
 *     w = a^((q-1)/2),  x = a w,  b = x w = a^q,
 * then, with g = z^q for a fixed non-residue z, the constant-time Tonelli-Shanks rounds i = s-1 .. 1: t = b^(2^(i-1)); where
 * t != 1, x *= g and b *= g^2 (a select, not a branch on data); g = g^2.  a is a residue exactly when x^2 == a in the end.  The
 * inverse root costs no second chain: 1/a = w^2 b0^(2^s - 1), 1/x = x / a (for s = 1 it is w).  One exponentiation of about the
 * field's bit length per element -- about 70 dependent products over Mersenne61, 272 over the secp256k1 prime, about 385 over its order:
 *     Mersenne61       s = 1    2^59 - 1, an addition chain          Mersenne127        s = 1    2^125 - 1, an addition chain
 *     secp256k1 prime  s = 1    (p-3)/4, an addition chain           secp256k1 order    s = 6    fixed 2-bit windows
 *     Mont128          s from the calling thread's modulus (5 for 2^128 - 159, 1 for 2^127 - 1), fixed 2-bit windows
 * For Mont128 the host derives s, q, the non-residue (the smallest integer that fails Euler's criterion) and g when the
 * thread's modulus changes and keeps them with it: no device work, no synchronisation.
 *
 * THE CANONICAL ROOT is the one whose integer value is even -- the value FF::write serialises, for the Montgomery fields the
 * value after from_mont, not the stored residue.  SCL_RB_ODD_ROOT selects the other root, its negative.
 *
 * THE STATUS, one byte per element or column:
 *     0   ok
 *     1   the input was zero; the root 0 is written (and 0 for its inverse; a column of bits is all 0)
 *     2   the input is a non-residue; 0 is written
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h and scl_hip_hm.h: SoA rows, strides in elements,
 * 8-byte alignment for one-limb elements and 16-byte alignment for wider ones, values canonical in and out, `stream` a
 * hipStream_t passed as void*.  Accepted tags: the five prime fields.  SCL_GF2_128 is refused ("squaring is a bijection of
 * GF(2^128): every element has one root and r / sqrt(r^2) is always 1") and so is a ring tag ("a ring Z2k is not a field"), each
 * with a message that names the reason.  SCL_MONT128 computes over the calling thread's modulus and honours the latch rule
 * documented at scl_hip_mont128_set_prime, as libscl_hip_hm.so does.
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown or refused tag, an
 * unknown flag bit and a forbidden overlap are SCL_ERR_BAD_ARG; a stride smaller than N is SCL_ERR_SIZE_MISMATCH; no device
 * SCL_ERR_NO_DEVICE.  N == 0 or rows == 0 returns SCL_OK at once.  status_dev is required.  A call allocates nothing, copies
 * nothing and never synchronises: each can be captured into a hipGraph from its first call on.
 */
#ifndef SCL_HIP_RB_H
#define SCL_HIP_RB_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_RB_ABI_VERSION 1
int         scl_rb_abi_version(void);          /* 1 */
const char* scl_rb_last_error(void);           /* per thread, like scl_hip_last_error */

/* flags of scl_rb_sqrt */
#define SCL_RB_ODD_ROOT 1u   /* the root with an odd integer value instead of the even one */
#define SCL_RB_INVERSE  2u   /* write 1/root instead of root */

/* out[s] = sqrt(a[s]) (or its inverse) and status[s] for s < N, one lane per element.  out_dev may be exactly a_dev (in place:
 * a lane reads its element before it writes it); any other overlap of out_dev, status_dev and a_dev is refused with both
 * operands named.  Refused too: a flags bit other than the two above. */
int scl_rb_sqrt(int field, uint64_t* out_dev, unsigned char* status_dev, const uint64_t* a_dev, size_t N, unsigned flags, void* stream);

/* Steps 4 and 5 for `rows` parties' shares at once: per column s < N, h = 2^-1 / root(u[s]) once (the even root), then
 *     b[i][s] = h * r[i][s] + 2^-1     for i < rows,
 * and status[s].  A column whose status is not 0 is 0 in every row: the output is always defined.  One lane per column
 * (Mersenne61: two where bases and strides allow); the traffic is (2 rows + 1) N elements and N bytes.  b_dev may be exactly
 * r_dev with b_stride == r_stride (in place); any other overlap is refused with both operands named -- b on u, b on r at an
 * offset or another stride, status on anything.  b_stride < N or r_stride < N is SCL_ERR_SIZE_MISMATCH. */
int scl_rb_bits_finish(int field, uint64_t* b_dev, size_t b_stride, unsigned char* status_dev,
                       const uint64_t* u_dev, const uint64_t* r_dev, size_t r_stride, size_t rows, size_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_RB_H */
