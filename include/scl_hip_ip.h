/* include/scl_hip_ip.h -- inner and matrix products of Shamir sharings at one opening each: the C ABI of libscl_hip_ip.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_mpc.so, libscl_hip_prep.so and libscl_hip_hm.so.  scl_hip_hm.h multiplies element by element; the point of the
 * Damgard-Nielsen shape it implements is that a whole SUM of products costs the same single opening as one product
 * ([r]_d = a degree-d sharing):
 *
 *   local step      [d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t                          scl_ip_dot_mask, scl_ip_matmul_mask
 *   open, subtract  open d from the n shares, [z]_t = d - [R]_t                      scl_hm_mul_finish (any number of rows)
 *
 * and [z]_t is a sharing of the inner product.  Both entry points serve MANY INDEPENDENT instances, the engine's batch model:
 * SoA rows of N columns, one instance per column.  One large product of two share matrices is scl_hip_matmul plus one
 * addition and is not served here.
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h, as in scl_hip_hm.h: SoA rows, strides in
 * elements, 8-byte alignment for one-limb elements and 16-byte alignment for wider ones, values canonical in and out,
 * `stream` a hipStream_t passed as void*.  Accepted tags: the six fields.  Shamir needs a field: a ring tag is refused with
 * "unknown field tag".  SCL_MONT128 computes over the calling thread's modulus and honours the latch rule documented at
 * scl_hip_mont128_set_prime, as libscl_hip_hm.so does.
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown tag, a forbidden
 * overlap, and what each entry point lists below, are SCL_ERR_BAD_ARG; a stride smaller than N is SCL_ERR_SIZE_MISMATCH; no
 * device SCL_ERR_NO_DEVICE.  N == 0, rows == 0 and batch == 0 return SCL_OK at once.
 *
 * WHAT A CALL DOES BESIDES LAUNCHING.  Nothing: a call allocates nothing, copies nothing and never synchronises, so each can
 * be captured into a hipGraph from its first call on.
 *
 * THE ACCUMULATION.  A lane keeps the sum in the field's lazy accumulator and folds once per F::ACC_TERMS terms
 * (Mersenne61: 64; the other fields: 2^24 and above), the addend counting as a term (include/scl_hip/detail/ip.hpp).  Every
 * residue has one canonical representative, so the result is bit-identical to the same value built one reduced operation at a
 * time.
 */
#ifndef SCL_HIP_IP_H
#define SCL_HIP_IP_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_IP_ABI_VERSION 1
int         scl_ip_abi_version(void);          /* 1 */
const char* scl_ip_last_error(void);           /* per thread, like scl_hip_last_error */

/* The local step of an inner product: d[r][s] = sum_{k<terms} x[k][r][s] * y[k][r][s] + r2[r][s] for r < rows, s < N.
 * Element x[k][r][s] lies at x_dev + k * x_term_stride + r * op_stride + s, y likewise with y_term_stride; r2[r][s] at
 * r2_dev + r * op_stride + s; d[r][s] at d_dev + r * d_stride + s.  r2_dev == NULL: no addend, a plain sum of products (the
 * form the verification protocols want).  One launch per 65535 rows; (2 terms + 2) rows N elements of traffic, 2 terms + 1
 * without r2.  A lane owns a column of a row (Mersenne61: two where bases and strides allow 16-byte accesses).  terms == 1
 * with r2 is exactly scl_hm_mul_mask.
 * The term strides are free: inputs are only read, so terms may overlap one another (a term stride of 0 is sum of terms
 * copies) and x may be y (sums of squares).
 * Refused: terms == 0; d_stride < N or op_stride < N (SCL_ERR_SIZE_MISMATCH); an extent that overflows.
 * Aliasing: d_dev may be r2_dev (with d_stride == op_stride: the same pointer and stride, and no other overlap of the two);
 * d_dev must not overlap x_dev; d_dev must not overlap y_dev (each judged on the bounding span of all terms and rows); x_dev,
 * y_dev and r2_dev are inputs and may overlap one another. */
int scl_ip_dot_mask(int field, uint64_t* d_dev, size_t d_stride,
                    const uint64_t* x_dev, size_t x_term_stride,
                    const uint64_t* y_dev, size_t y_term_stride,
                    const uint64_t* r2_dev, size_t op_stride,
                    size_t terms, size_t rows, size_t N, void* stream);

/* The local step of a batch of small matrix products: for q < batch, i < a, l < b, s < N
 *     D[q][i][l][s] = sum_{k<K} X[q][i][k][s] * Y[q][k][l][s] + R2[q][i][l][s].
 * Entry (i,k) of batch q of X is a row of N columns at x_dev + q * x_batch_stride + (i * K + k) * x_stride: X is row-major
 * a x K, Y row-major K x b, D and R2 row-major a x b, all addressed the same way.  `batch` is the parties simulated on one
 * device, as in scl_hm_apply; with batch == 1 the batch strides are ignored.  r2_dev == NULL: no addend.
 * A lane owns a column of one batch and a TI x TL tile of outputs in accumulators and walks k once per tile (TI + TL operand
 * loads per k); tiles and batches go on the grid's other axes, one launch per 65535 batches and per 65535 tiles.  Traffic
 * per column and batch:
 *     ceil(b/TL) a K + ceil(a/TI) K b + 2 a b   elements (a b less without r2),
 * TI x TL per field from scl_ip_matmul_tile: 4 x 4 for Mersenne61, 2 x 4 for the 16-byte fields, 2 x 2 for the 32-byte fields
 * (docs/kernels/ip.md has the register figures).  a == b == 1 is the inner product and runs the kernel of scl_ip_dot_mask.
 * Refused: a, K or b equal to 0 or above 65535; a row stride < N (SCL_ERR_SIZE_MISMATCH); with batch > 1, a d_batch_stride
 * too small to keep the batches of D apart; a batch count whose extents overflow.
 * Aliasing: d_dev may be r2_dev (with d_stride == r2_stride and, where batch > 1, d_batch_stride == r2_batch_stride: the same
 * pointer and strides, and no other overlap of the two); d_dev must not overlap x_dev; d_dev must not overlap y_dev (each
 * judged on the bounding span of all batches); x_dev, y_dev and r2_dev are inputs and may overlap one another. */
int scl_ip_matmul_mask(int field,
                       uint64_t* d_dev,  size_t d_stride,  size_t d_batch_stride,
                       const uint64_t* x_dev,  size_t x_stride,  size_t x_batch_stride,
                       const uint64_t* y_dev,  size_t y_stride,  size_t y_batch_stride,
                       const uint64_t* r2_dev, size_t r2_stride, size_t r2_batch_stride,
                       size_t a, size_t K, size_t b, size_t batch, size_t N, void* stream);

/* The output tile a lane of scl_ip_matmul_mask owns for this field: *ti rows by *tl columns; both 0 for a tag the call refuses. */
void scl_ip_matmul_tile(int field, int* ti, int* tl);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_IP_H */
