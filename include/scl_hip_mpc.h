/* include/scl_hip_mpc.h -- protocol arithmetic over the engine of scl_hip.h: the C ABI of libscl_hip_mpc.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h).  It
 * holds the online phase of Beaver multiplication, the reference's only in-tree protocol (test/scl/protocol/beaver.h:31-70):
 *   mask    [e] = [x] - [a],  [d] = [y] - [b]              beaver.h:40-41 (e first, then d, one packet)
 *   ... the parties open e and d (scl_hip_shamir_recover / scl_hip_additive_recover / scl_hip_open_*) ...
 *   finish  [z] = e [b] + d [a] + [c]  (+ e d, added by the parties that add constants)      beaver.h:57-61
 * Each call is ONE kernel launch on the caller's stream: nothing allocates, copies or synchronises, so both can be captured
 * into a hipGraph.
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h: SoA rows, strides in elements, 8-byte alignment
 * for one-limb elements and 16-byte alignment for wider ones, `stream` a hipStream_t passed as void*, values canonical on
 * entry and on exit (rings: taken modulo 2^K, returned masked).  All six fields and SCL_Z2K(K), 1 <= K <= 128, are accepted.
 * SCL_MONT128 computes over the calling thread's modulus (scl_hip_mont128_get_prime) and honours the latch rule documented
 * at scl_hip_mont128_set_prime: a thread whose latched default has gone stale gets SCL_ERR_BAD_ARG here as from the engine
 * (the check is the engine's own, reached through scl_hip_lagrange_basis on one node: a host-only call).
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown tag, ed_rows > rows
 * or a forbidden overlap is SCL_ERR_BAD_ARG, a stride smaller than N SCL_ERR_SIZE_MISMATCH, no device SCL_ERR_NO_DEVICE.
 * N == 0 or rows == 0 returns SCL_OK at once.
 */
#ifndef SCL_HIP_MPC_H
#define SCL_HIP_MPC_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_MPC_ABI_VERSION 1
int         scl_mpc_abi_version(void);          /* 1 */
const char* scl_mpc_last_error(void);           /* per thread, like scl_hip_last_error */

/* e = x - a and d = y - b for `rows` parties' vectors of N elements in one launch.  Operand row r starts at
 * base + r*op_stride elements.  Output: a (2*rows) x N SoA matrix of stride de_stride -- rows 0..rows-1 are e, rows
 * rows..2*rows-1 are d.  With rows = 1 and de_stride = N that is the reference's packet, e then d, contiguous; with
 * rows = n the two halves are share matrices scl_hip_shamir_recover / scl_hip_additive_recover take as they lie.
 * de_dev may not overlap an operand.  (More than 65535 rows are split over launches.) */
int scl_mpc_beaver_mask(int field, uint64_t* de_dev, size_t de_stride, const uint64_t* x_dev, const uint64_t* y_dev,
                        const uint64_t* a_dev, const uint64_t* b_dev, size_t op_stride, size_t rows, size_t N, void* stream);

/* z[r][s] = e[s]*b[r][s] + d[s]*a[r][s] + c[r][s], plus e[s]*d[s] for rows r < ed_rows (Shamir: ed_rows = rows -- a
 * constant is its own sharing; additive: 1 where row 0 is party 0, else 0).  e_dev, d_dev: N opened values shared by all
 * rows.  z_dev may be exactly a_dev, b_dev or c_dev with z_stride == op_stride (each lane reads before it writes); any
 * other overlap with an operand, e or d is SCL_ERR_BAD_ARG. */
int scl_mpc_beaver_finish(int field, uint64_t* z_dev, size_t z_stride, const uint64_t* e_dev, const uint64_t* d_dev,
                          const uint64_t* a_dev, const uint64_t* b_dev, const uint64_t* c_dev, size_t op_stride,
                          size_t rows, size_t ed_rows, size_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_MPC_H */
