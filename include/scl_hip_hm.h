/* include/scl_hip_hm.h -- honest-majority multiplication over the engine of scl_hip.h: the C ABI of libscl_hip_hm.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_mpc.so and libscl_hip_prep.so.  Those two multiply with triples of a trusted dealer; a Shamir deployment with
 * n > 2t parties needs none.  This library holds the pieces of the Damgard-Nielsen multiplication ([r]_d = a degree-d sharing):
 *
 *   preprocessing   party i picks r_i and deals it twice, [r_i]_t and [r_i]_2t      scl_hm_double_share_prg
 *                   everyone applies the (n-t) x n hyper-invertible matrix M
 *                   (Matrix::hyperInvertible, matrix.h:462-475) to the n sharings
 *                   it received, at both degrees: n-t double sharings nobody knows   scl_hm_apply
 *   per product     [d]_2t = [x]_t [y]_t + [R]_2t                                   scl_hm_mul_mask
 *                   open d from the n shares, [z]_t = d - [R]_t                     scl_hm_mul_finish
 *
 * THE DISCIPLINE of scl_hm_double_share_prg.  E = the field's byteSize (8, 16 or 32), BPE = ceil(E/16) = the blocks one
 * FF::random consumes (ff.h:72-76: util::PRG::next draws whole blocks and buffers nothing, prg.cc:124-146),
 * Bs(d) = ceil((d+1) E / 16) = the blocks of one Vector::random(d+1) draw (vector.h:507-519).  The double sharings a call deals
 * are what a reference program deals that runs, on ONE util::PRG,
 *     r = FF::random(prg);  lo = shamirSecretShare(r, t, n, prg);  hi = shamirSecretShare(r, 2t, n, prg);
 * once per double sharing.  Double sharing s occupies the blocks [counter0 + s*B, counter0 + (s+1)*B),
 * B = BPE + Bs(t) + Bs(2t), drawn in this order:
 *     1. r                                                                          ff.h:72-76
 *     2. ONE Vector::random(t+1) draw of Bs(t) blocks for the degree-t polynomial; its first element is discarded and
 *        replaced by r                                                              shamir.h:56-57
 *     3. ONE Vector::random(2t+1) draw of Bs(2t) blocks for the degree-2t polynomial, treated likewise
 *   Mersenne61 (10,3): B = 1 + 2 + 4 = 7.  secp256k1 order (10,3): B = 2 + 8 + 14 = 24.
 * Row i of lo_dev and of hi_dev holds party i's shares, the polynomials at the node i+1 (over GF(2^128): the bit pattern of
 * i+1, as everywhere in the engine).  A caller that holds `prg` at counter0 and deals N double sharings advances it by
 * N * scl_hm_double_blocks(..) blocks; double sharings [f, f+k) of a long run are the call with counter0 + f*B.
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h: SoA rows, strides in elements, 8-byte alignment
 * for one-limb elements and 16-byte alignment for wider ones, values canonical in and out, `stream` a hipStream_t passed as
 * void*.  Accepted tags: the six fields.  Shamir needs a field: a ring tag is refused with "unknown field tag", as
 * scl_prep_triples_shamir_prg refuses it.  SCL_MONT128 computes over the calling thread's modulus and honours the latch rule
 * documented at scl_hip_mont128_set_prime, as libscl_hip_mpc.so does.
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown tag, a forbidden
 * overlap, and what each entry point lists below, are SCL_ERR_BAD_ARG; a stride smaller than N is SCL_ERR_SIZE_MISMATCH; no
 * device SCL_ERR_NO_DEVICE.  N == 0 returns SCL_OK at once.
 *
 * WHAT A CALL DOES BESIDES LAUNCHING.  scl_hm_apply, scl_hm_mul_mask, scl_hm_mul_finish and the fused path of
 * scl_hm_double_share_prg allocate nothing, copy nothing and never synchronise: each can be captured into a hipGraph from its
 * first call on.  The two-pass path ends in two calls of scl_hip_shamir_share and inherits what scl_hip_prep.h states of that
 * call: no synchronisation, but the FIRST call of a shape the engine shares through a device table builds the table (one
 * hipMalloc, one synchronous hipMemcpy).  So a two-pass call is captured after one call of the same shape outside the capture.
 */
#ifndef SCL_HIP_HM_H
#define SCL_HIP_HM_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_HM_ABI_VERSION 1
int         scl_hm_abi_version(void);          /* 1 */
const char* scl_hm_last_error(void);           /* per thread, like scl_hip_last_error */

/* flags of scl_hm_double_share_prg / scl_hm_double_scratch_bytes: bit 0 forces the two-pass path */
#define SCL_HM_TWO_PASS 1u

/* B of the discipline above: the AES blocks one double sharing consumes; 0 for arguments the deal call refuses. */
size_t scl_hm_double_blocks(int field, size_t n, size_t t);

/* Bytes of device scratch scl_hm_double_share_prg needs for this case: 0 where the fused kernel deals it (Mersenne61,
 * Mersenne127 and GF(2^128) at t <= 3, flags bit 0 clear), else (1 + 3t) * N elements (the two-pass path: the Montgomery
 * fields, t >= 4, or flags bit 0).  0 for arguments the call refuses. */
size_t scl_hm_double_scratch_bytes(int field, size_t N, size_t n, size_t t, unsigned flags);

/* N double sharings of one dealer: lo_dev the n x N matrix of degree-t shares, hi_dev that of degree-2t shares of the same
 * secrets, one stride.  Refused: n <= 2t (degree 2t could not be opened), n > 65535, 2t > 48 (2t > 16 for the 32-byte fields:
 * beyond it the engine's share call synchronises the stream), a block range that wraps the 64-bit counter, matrices or
 * scratch that overlap, a flags bit other than bit 0, a two-pass case without scratch (the message names the bytes needed).
 * Fused (one launch, nothing read, scratch_dev ignored and may be NULL) where scl_hm_double_scratch_bytes is 0; else two
 * passes: one launch writes r[N] and the 3t coefficient rows [3t][N] (t of the first polynomial, then 2t of the second) into
 * scratch_dev (16-byte aligned), then two calls of scl_hip_shamir_share evaluate them on the same stream.  The two paths deal
 * the same sharings. */
int scl_hm_double_share_prg(int field, uint64_t* lo_dev, uint64_t* hi_dev, size_t stride, size_t N, size_t t, size_t n,
                            const unsigned char* seed_host, size_t seed_len, uint64_t counter0,
                            uint64_t* scratch_dev, unsigned flags, void* stream);

/* A small matrix applied across sharings (the extraction): for b < batch and k < m
 *     out[b][k][s] = sum_{i<n} M[k][i] * in[b][i][s],   s < N,
 * row k of batch b of `out` at out_dev + b * out_batch_stride + k * out_stride elements, `in` likewise.  M_dev is m x n,
 * row-major with leading dimension ldm >= n, canonical and already on the device (the caller uploads it once).  One launch per
 * 65535 batches; a lane owns a column (Mersenne61: two where bases and strides allow).  Where n <= 16 and the m n elements of M
 * fit 16 KiB -- the extraction's own shapes -- the lane keeps its n inputs in registers and the traffic is (n + m) N elements
 * per batch; otherwise it walks the n input rows once per group of R output rows (R per field: docs/kernels/hm.md) and the
 * traffic is (ceil(m/R) n + m) N.
 * With dealers' matrices laid out [dealer][party][N], party j's input is base + j * stride with in_stride = n * stride; batch
 * and its two strides let one launch serve all n simulated parties.  With batch == 1 the batch strides are ignored.
 * Refused: m == 0, n == 0, n > 65535, ldm < n, out overlapping in or M.  batch == 0 returns SCL_OK like N == 0. */
int scl_hm_apply(int field, uint64_t* out_dev, size_t out_stride, size_t out_batch_stride,
                 const uint64_t* in_dev, size_t in_stride, size_t in_batch_stride,
                 const uint64_t* M_dev, size_t ldm, size_t m, size_t n, size_t batch, size_t N, void* stream);

/* The first local step of a product: d[r][s] = x[r][s] * y[r][s] + r2[r][s] for r < rows -- one product and one reduction.
 * x, y and r2 share op_stride.  d_dev may be exactly r2_dev with d_stride == op_stride; any other overlap is refused.
 * rows == 0 returns SCL_OK like N == 0. */
int scl_hm_mul_mask(int field, uint64_t* d_dev, size_t d_stride, const uint64_t* x_dev, const uint64_t* y_dev,
                    const uint64_t* r2_dev, size_t op_stride, size_t rows, size_t N, void* stream);

/* The second: open and subtract in one launch, z[r][s] = sum_{j<m} lambda[j] * dsh[j][s] - r[r][s] for r < rows.  lambda_host
 * (m canonical elements on the host) travels with the launch, as in scl_hip_shamir_recover; 1 <= m <= 64 -- beyond that
 * the call is refused: use scl_hip_shamir_recover and scl_hip_ew.  m == 1 with lambda = {1} is the form for a d that was
 * already opened.  The opened value is computed once per column and reused for all rows: (m + 2 rows) N elements of traffic.
 * z_dev may be exactly r_dev with z_stride == r_stride; z may not overlap dsh otherwise.  rows == 0 returns SCL_OK. */
int scl_hm_mul_finish(int field, uint64_t* z_dev, size_t z_stride, const uint64_t* dsh_dev, size_t d_stride,
                      const uint64_t* lambda_host, size_t m, const uint64_t* r_dev, size_t r_stride,
                      size_t rows, size_t N, void* stream);

/* THE HYPER-INVERTIBLE MATRIX needs no entry point: row i of Matrix::hyperInvertible(m, n) (matrix.h:462-475) is
 * scl_hip_lagrange_basis with nodes NULL (= 1..n) and x = -i.  GF(2^128) is this project's own field; in characteristic 2
 * -i = i collides with the nodes, so the bindings (scl_amd.hm.hyper_invertible, hip::hyperInvertible) take the evaluation
 * points as an optional argument and default, over GF(2^128), to the bit patterns n + 1 + i.  That default is this
 * project's choice, not the reference's. */

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_HM_H */
