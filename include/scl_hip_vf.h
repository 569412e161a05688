/* include/scl_hip_vf.h -- batch verification: random linear combinations of sharings along N.  The C ABI of libscl_hip_vf.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_mpc.so, libscl_hip_prep.so, libscl_hip_hm.so and libscl_hip_ip.so.  Those libraries are passively secure.  A
 * party that wants to DETECT cheating checks that N dealt sharings have the right degree, that N double sharings share one
 * value at both degrees, that N products are right -- and the affordable way is to draw a public coin, fold the N instances
 * into one with a random linear combination, and check that one:
 *
 *   plain form     out[r][j] = sum_s rho_j[s] x[r][s]                       (y_dev == NULL)
 *   product form   out[r][j] = sum_s rho_j[s] x[r][s] y[r][s]
 *
 * for j < reps, r < rows, s over the N columns.  Every other batched entry point of the project reduces across rows per
 * column; these reduce ALONG N per row.  out[r][j] lies at out_dev + r * out_stride + j, so n rows of parties by `reps`
 * columns is directly the share matrix scl_hip_shamir_recover_detect takes with N = reps.  x[r][s] lies at
 * x_dev + r * op_stride + s, y likewise.  1 <= reps <= 4: one combination over Mersenne61 has soundness error about 2^-61, two
 * or three repetitions are what a user of that field needs, and one launch re-uses the loads of x for all of them.
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h, as in scl_hip_ip.h: SoA rows, strides in
 * elements, 8-byte alignment for one-limb elements and 16-byte alignment for wider ones, values canonical in and out,
 * `stream` a hipStream_t passed as void*.  Accepted tags: the six fields; a ring tag is refused with "unknown field tag".
 * SCL_MONT128 computes over the calling thread's modulus and honours the latch rule documented at
 * scl_hip_mont128_set_prime, as libscl_hip_ip.so does.
 *
 * Errors are decided on the host before anything is launched, with the argument named in scl_vf_last_error: a NULL or
 * misaligned pointer, an unknown tag, reps outside 1..4, a scratch smaller than scl_vf_scratch_bytes, an extent that
 * overflows, a block range that wraps the 64-bit counter and a forbidden overlap are SCL_ERR_BAD_ARG; a stride below its
 * extent (out_stride < reps, op_stride < N, rho_stride < N) is SCL_ERR_SIZE_MISMATCH; no device SCL_ERR_NO_DEVICE.
 * rows == 0 returns SCL_OK at once.  N == 0 with rows > 0 WRITES ZEROS: the empty sum is defined.
 *
 * WHAT A CALL DOES BESIDES LAUNCHING.  Nothing: a call allocates nothing, copies nothing and never synchronises (the AES key
 * is expanded on the host into a kernel argument), so each can be captured into a hipGraph from its first call on.  Every
 * launch goes to `stream`: the combination kernel (per 65535 groups of rows), then one small kernel that sums the
 * per-workgroup partial sums; scl_vf_combine_prg in its two-pass form fills the coefficient rows first.  There are no atomics,
 * no counters in memory and no last-block pattern.
 *
 * THE ACCUMULATION.  A lane keeps R x reps sums in the field's lazy accumulator, R rows of x against the same coefficient
 * held in registers (scl_vf_launch_shape has R).  Before a term goes in, an accumulator that has reached F::ACC_TERMS terms
 * (Mersenne61: 64; the other fields: 2^24 and above) folds into itself (include/scl_hip/detail/vf.hpp, on the count of
 * ip.hpp).  In the product form x y is reduced to an element first and then multiplied by rho: one term.  The second kernel
 * adds the partial sums under the same count.  Field addition is exact and every residue has one canonical representative,
 * so THE RESULT DOES NOT DEPEND ON THE ORDER of the additions: it is bit-identical to Vector::innerProd of the reference, one
 * reduced operation at a time.
 *
 * THE COIN of scl_vf_combine_prg.  rho_j is the j-th consecutive Vector<FF>::random(N, prg) of a util::PRG created from the
 * seed (zero-padded or truncated to 16 bytes) with its block counter at counter0: rho_j draws blocks
 * [counter0 + j B, counter0 + (j + 1) B), B = scl_vf_coin_blocks(field, N).  The block-to-element mapping is exactly that of
 * scl_hip_vector_random: Mersenne61 two elements a block (the second half of the last block is discarded at odd N), the
 * 16-byte fields one block an element, the 32-byte fields two blocks an element.
 */
#ifndef SCL_HIP_VF_H
#define SCL_HIP_VF_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_VF_ABI_VERSION 1
int         scl_vf_abi_version(void);          /* 1 */
const char* scl_vf_last_error(void);           /* per thread, like scl_hip_last_error */

/* flags of scl_vf_scratch_bytes: the scratch of scl_vf_combine_prg (without it: of scl_vf_combine) */
#define SCL_VF_PRG 1u

/* ceil(N * byteSize / 16): the AES blocks one Vector::random(N, prg) consumes.  0 for a tag the calls refuse. */
size_t scl_vf_coin_blocks(int field, size_t N);

/* Bytes of scratch a call with these arguments needs: the per-workgroup partial sums (rows * reps elements per workgroup
 * along N) and, with SCL_VF_PRG for a field whose scl_vf_combine_prg takes the two-pass path, reps coefficient rows of N
 * elements.  Monotone in rows, reps and N.  0: a tag or reps the calls refuse, unknown flags, or a size that overflows. */
size_t scl_vf_scratch_bytes(int field, size_t rows, size_t reps, size_t N, unsigned flags);

/* The launch geometry for this field and reps, for tests and probes.  `prg` non-zero: of scl_vf_combine_prg.
 *   *rows_per_group   R: rows of x a lane accumulates against one coefficient
 *   *cols_per_trip    columns one workgroup covers per trip of its lanes
 *   *max_groups       the most workgroups along N (beyond cols_per_trip * max_groups columns a lane takes further trips)
 *   *fused            scl_vf_combine_prg draws the coin in registers (1) or fills coefficient rows in scratch first (0);
 *                     0 where prg == 0
 * All 0 for a tag or reps the calls refuse.  Any pointer may be NULL. */
void scl_vf_launch_shape(int field, size_t reps, int prg, int* rows_per_group, size_t* cols_per_trip, size_t* max_groups, int* fused);

/* out[r][j] = sum_s rho_j[s] x[r][s] (y[r][s]), rho_j drawn from the AES-CTR PRG as described above.  y_dev == NULL: the
 * plain form.  Mersenne61 draws rho in registers and moves rows * N elements (2 rows N in the product form); the other
 * fields take the two-pass path: scl_hip_vector_random's kernel fills reps rows of scratch, then the streaming
 * form of scl_vf_combine reads them once per group of R rows.
 * Refused: reps == 0 or reps > 4; out_stride < reps or op_stride < N (SCL_ERR_SIZE_MISMATCH); scratch_bytes below
 * scl_vf_scratch_bytes(field, rows, reps, N, SCL_VF_PRG); counter0 + reps * B wrapping 2^64 or ending within 128 blocks of
 * it (counter0 + reps * B > 2^64 - 129: the kernels round their work up and draw a few blocks past the last, as
 * scl_hm_double_share_prg's do); an extent that overflows.
 * Aliasing: out_dev must not overlap x_dev, y_dev or scratch_dev; scratch_dev must not overlap x_dev or y_dev; x_dev and
 * y_dev are inputs and may overlap one another (x_dev == y_dev gives sum rho x^2). */
int scl_vf_combine_prg(int field, uint64_t* out_dev, size_t out_stride,
                       const uint64_t* x_dev, const uint64_t* y_dev, size_t op_stride,
                       size_t rows, size_t N, size_t reps,
                       const unsigned char* seed_host, size_t seed_len, uint64_t counter0,
                       uint64_t* scratch_dev, size_t scratch_bytes, void* stream);

/* The same value with rho_j read from rho_dev + j * rho_stride: coefficients that come from elsewhere (powers of a
 * challenge, a coin agreed on another way).  rows (2 rows in the product form) * N elements of x and y, and the reps
 * coefficient rows once per group of R rows.
 * Refused: reps == 0 or reps > 4; out_stride < reps, op_stride < N or rho_stride < N (SCL_ERR_SIZE_MISMATCH); scratch_bytes
 * below scl_vf_scratch_bytes(field, rows, reps, N, 0); an extent that overflows.
 * Aliasing: out_dev must not overlap x_dev, y_dev, rho_dev or scratch_dev; scratch_dev must not overlap x_dev, y_dev or
 * rho_dev; x_dev, y_dev and rho_dev are inputs and may overlap one another. */
int scl_vf_combine(int field, uint64_t* out_dev, size_t out_stride,
                   const uint64_t* x_dev, const uint64_t* y_dev, size_t op_stride,
                   const uint64_t* rho_dev, size_t rho_stride,
                   size_t rows, size_t N, size_t reps,
                   uint64_t* scratch_dev, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_VF_H */
