/* include/scl_hip_fx.h -- fixed-point arithmetic over Shamir sharings, its first step: probabilistic truncation.  The C ABI of
 * libscl_hip_fx.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_rb.so, whose shared random bits it consumes.  A fixed-point product [x][y] carries 2f fractional bits; f of them are
 * dropped by the probabilistic truncation of Catrina and de Hoogh -- one mask, one opening, one local finish, the shape of
 * scl_hm_mul_mask / _finish.  p is the field's prime, |p| its bit length.  x stands for a signed integer in
 * [-2^(k-1), 2^(k-1)); the caller supplies B = k + kappa shared random bits [b_0] .. [b_(B-1)] per value (kappa, the statistical
 * parameter, may be 0).  With 1 <= shift < k <= B <= |p| - 2:
 *
 *     r  = sum_{i<B} 2^i b_i                  r' = sum_{i<shift} 2^i b_i
 *   1. [c] = [x] + 2^(k-1) + [r], and [r']                          scl_fx_trunc_mask (degree t: everything is linear)
 *   2. open c from t + 1 or more shares,                            scl_fx_trunc_finish: steps 2 and 3 in one launch
 *   3. c' = c mod 2^shift AS AN INTEGER, from the canonical value -- what FF::write serialises, for the Montgomery fields the value
 *      after from_mont, not the stored residue --, and [y] = ([x] + [r'] - c') * 2^-shift in the field.
 *
 * B <= |p| - 2 makes c < 2^(B+1) < p, so nothing wraps, and
 *     y = floor((x + 2^(k-1)) / 2^shift) + carry - 2^(k-1-shift),   carry = [ (x + 2^(k-1)) mod 2^shift + r' >= 2^shift ]:
 * y is floor(x / 2^shift) or that plus one.
 *
 * THE BIT PLANES.  `bits_dev` holds B planes of rows x N elements: plane i, row r lies at bits_dev + i * plane_stride +
 * r * row_stride (elements), N elements long.  One scl_rb_bits_finish over B * N columns feeds it without a copy: plane_stride
 * = N, row_stride = B * N.
 *
 * THE STATUS of scl_fx_trunc_finish, one byte per column:
 *     0   ok
 *     1   the opened c is at or above 2^(B+1): an input out of range, planes that were no bits, or wrong shares.  The column
 *         is 0 in every row: the output is always defined.
 * The check is best effort: a wrong c that stays below 2^(B+1) is not caught, and neither is an x outside [-2^(k-1), 2^(k-1))
 * that a large enough kappa hides.
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h and scl_hip_rb.h: SoA rows, strides in elements,
 * 8-byte alignment for one-limb elements and 16-byte alignment for wider ones, values canonical in and out, `stream` a
 * hipStream_t passed as void*.  Accepted tags: the five prime fields.  SCL_GF2_128 is refused ("GF(2^128) has no integers below
 * a prime: there is nothing to reduce modulo 2^shift") and so is a ring tag ("a ring Z2k is not a field: it has no 2^-shift and no
 * Shamir sharing"), each with a message that names the reason.  SCL_MONT128 computes over the calling thread's modulus and honours
 * the latch rule documented at scl_hip_mont128_set_prime, as libscl_hip_rb.so does.
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown or refused tag, a bit
 * count, k or shift out of range, m outside 1..64 and a forbidden overlap are SCL_ERR_BAD_ARG; a stride smaller than N is
 * SCL_ERR_SIZE_MISMATCH; no device SCL_ERR_NO_DEVICE.  N == 0 or rows == 0 returns SCL_OK at once.  status_dev is required.  A call
 * allocates nothing, copies nothing and never synchronises: each can be captured into a hipGraph from its first call on -- the
 * constants (2^(k-1), 2^-shift, the masks, for SCL_MONT128 whatever the latched modulus determines) travel as kernel arguments.
 */
#ifndef SCL_HIP_FX_H
#define SCL_HIP_FX_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_FX_ABI_VERSION 1
int         scl_fx_abi_version(void);          /* 1 */
const char* scl_fx_last_error(void);           /* per thread, like scl_hip_last_error */

/* |p| - 2, the largest B: 59 for SCL_M61, 125 for SCL_M127, 254 for both secp256k1 fields; for SCL_MONT128 from the calling
 * thread's modulus (126 for 2^128 - 159, 125 for 2^127 - 1).  0 for a refused or unknown tag (and for a stale Mont128 latch). */
size_t scl_fx_max_bits(int field);

/* out[r][s] = sum_{i<B} 2^i bits[i][r][s] for r < rows, s < N: the bounded random value that masks are made of.  One lane per
 * column (Mersenne61: two where bases and strides allow), Horner from the top plane down, no field product; the traffic is
 * (B + 1) rows N elements.  1 <= B <= scl_fx_max_bits(field), else SCL_ERR_BAD_ARG.  out_dev must not overlap bits_dev.
 * out_stride < N, plane_stride < N (B > 1) or row_stride < N (rows > 1) is SCL_ERR_SIZE_MISMATCH. */
int scl_fx_compose(int field, uint64_t* out_dev, size_t out_stride, const uint64_t* bits_dev, size_t plane_stride, size_t row_stride,
                   size_t B, size_t rows, size_t N, void* stream);

/* Step 1 for `rows` parties' shares at once, one launch: c[r][s] = x[r][s] + 2^(k-1) + r and rlow[r][s] = r', r and r' composed
 * from the planes as above.  The traffic is (B + 3) rows N elements.  c_dev may be exactly x_dev with c_stride == x_stride (in
 * place: a lane reads its element before it writes it); every other overlap of c_dev, rlow_dev, x_dev and bits_dev is refused
 * with both operands named.  Refused with the reason: shift == 0, shift >= k, k > B, B > scl_fx_max_bits(field). */
int scl_fx_trunc_mask(int field, uint64_t* c_dev, size_t c_stride, uint64_t* rlow_dev, size_t rlow_stride, const uint64_t* x_dev,
                      size_t x_stride, const uint64_t* bits_dev, size_t plane_stride, size_t row_stride, size_t k, size_t shift, size_t B,
                      size_t rows, size_t N, void* stream);

/* Steps 2 and 3: per column s < N the opening c = sum_{j<m} lambda[j] csh[j][s] once (lambda_host: m canonical elements on the
 * host, they travel with the launch; 1 <= m <= 64, and m == 1 with lambda = {1} is the form for an already opened c), c' and
 * status[s], then for every row r < rows
 *     y[r][s] = (x[r][s] + rlow[r][s] - c') * 2^-shift.
 * A column whose status is not 0 is 0 in every row.  One lane per column (Mersenne61: two where bases and strides allow); the
 * traffic is (m + 3 rows) N elements and N bytes.  y_dev may be exactly x_dev, or exactly rlow_dev, with equal strides (in
 * place); any other overlap is refused with both operands named.  Refused with the reason: shift == 0, shift >= B,
 * B > scl_fx_max_bits(field), m outside 1..64. */
int scl_fx_trunc_finish(int field, uint64_t* y_dev, size_t y_stride, unsigned char* status_dev, const uint64_t* csh_dev, size_t c_stride,
                        const uint64_t* lambda_host, size_t m, const uint64_t* x_dev, size_t x_stride, const uint64_t* rlow_dev,
                        size_t rlow_stride, size_t shift, size_t B, size_t rows, size_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_FX_H */
