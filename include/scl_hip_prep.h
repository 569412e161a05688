/* include/scl_hip_prep.h -- preprocessing over the engine of scl_hip.h: the C ABI of libscl_hip_prep.so.
 *
 * An extension library beside libscl_hip.so (it links against it and uses nothing but the prototypes of scl_hip.h), like
 * libscl_hip_mpc.so.  It holds the trusted dealer of multiplication triples ([a], [b], [c = a b]), the half of the
 * reference's only in-tree protocol that feeds BeaverMul: randomTriple2 (test/scl/protocol/triple.h:37-48).  The triples a
 * call deals are the triples the reference deals, one randomTriple call after another on ONE util::PRG with the same seed,
 * word for word: the AES-CTR stream is counter-addressed, so triple s owns a fixed range of blocks and every lane of the
 * kernels finds its own.
 *
 * THE DISCIPLINE.  E = the field's byteSize (8, 16 or 32; rings: (K-1)/8 + 1), BPE = ceil(E/16) = the blocks one
 * FF::random consumes (ff.h:72-76: util::PRG::next draws whole blocks and buffers nothing, prg.cc:124-146).
 *
 *   additive, n >= 2 parties  (triple.h:37-48 with its `2` replaced by n):  triple s occupies the blocks
 *   [counter0 + s*B, counter0 + (s+1)*B), B = (2 + 3 (n-1)) BPE, drawn in this order:
 *     1. a                                                       triple.h:39
 *     2. b                                                       triple.h:40
 *     3. the n-1 random shares of a  (share n-1 = a - their sum)  triple.h:43, additive.h:41-53
 *     4. the n-1 random shares of b                              triple.h:44
 *     5. the n-1 random shares of c = a b                        triple.h:41, 45
 *   n = 2 is the reference's function literally.
 *
 *   Shamir (n, t), nodes 1..n  (the same shape with shamirSecretShare(v, t, n, prg), shamir.h:51-68, in place of
 *   additiveShare):  B = 2 BPE + 3 Bs with Bs = ceil((t+1) E / 16), drawn in this order:
 *     1. a   (BPE blocks)
 *     2. b   (BPE blocks)
 *     3. ONE Vector::random(t+1) draw of Bs blocks (shamir.h:56, vector.h:507-519: (t+1) E consecutive bytes) for the
 *        polynomial of a; its first element is discarded (shamir.h:57) and replaced by a
 *     4. one such draw for b
 *     5. one such draw for c = a b
 *   Party i's share is the polynomial at the node i+1 (over GF(2^128): the bit pattern of i+1, as everywhere in the engine).
 *
 * a_dev, b_dev and c_dev are n x N share matrices (row i = party i's shares of the N triples) of ONE stride: what
 * scl_mpc_beaver_mask / scl_mpc_beaver_finish and the engine's recover calls take as they lie.  A caller that holds `prg`
 * at counter0 and deals N triples advances it by N * scl_prep_triple_blocks(..) blocks; triples [f, f+k) of a long run are
 * the call with counter0 + f*B (shards need no communication).
 *
 * Field tags, scl_status values and every convention are those of scl_hip.h: SoA rows, strides in elements, 8-byte alignment
 * for one-limb elements and 16-byte alignment for wider ones, values canonical, `stream` a hipStream_t passed as void*.
 * Accepted tags: additive -- what scl_hip_additive_share_prg accepts (all six fields and SCL_Z2K(K), 1 <= K <= 128);
 * Shamir -- what scl_hip_shamir_share_prg accepts (the six fields).  SCL_MONT128 computes over the calling thread's modulus
 * and honours the latch rule documented at scl_hip_mont128_set_prime, as libscl_hip_mpc.so does.
 *
 * Errors are decided on the host before anything is launched: a NULL or misaligned pointer, an unknown tag, n < 2
 * (additive), n == 0 or n > 65535 (Shamir), a threshold t > 48 (t > 16 for the 32-byte fields) -- see below --, overlapping
 * matrices, a flags bit other than bit 0, a block range that wraps the 64-bit counter or a two-pass case without scratch is
 * SCL_ERR_BAD_ARG; stride < N is SCL_ERR_SIZE_MISMATCH; no device SCL_ERR_NO_DEVICE.  N == 0 returns SCL_OK at once.
 *
 * WHAT A CALL DOES BESIDES LAUNCHING.  scl_prep_triples_additive_prg and the fused path of scl_prep_triples_shamir_prg allocate
 * nothing, copy nothing and never synchronise: each can be captured into a hipGraph from its first call on.  The two-pass
 * path ends in three calls of the engine's scl_hip_shamir_share and inherits what that call does:
 *   - it never synchronises: the thresholds at which the engine evaluates chunk by chunk (it stages each chunk's table from
 *     host memory and waits for the stream) are the ones refused above;
 *   - the engine keeps a device table per (device, field parameters, n, t) for the shapes it shares through one: shapes of
 *     the Montgomery fields (SCL_MONT128, both secp256k1 fields) at t >= 1, and the Mersenne61 shapes it sends to the matrix
 *     cores (n <= 128 and n (t+1) >= 512).  The FIRST call of such a shape on a device builds the table: one hipMalloc and
 *     one synchronous hipMemcpy of the table (32 KiB at most for the Montgomery fields).  The tables are cached (the sixteen
 *     shapes used last, per process and kind); every later call of a cached shape allocates and copies nothing.
 * So a two-pass call is captured into a hipGraph after one call of the same shape has run outside the capture.
 */
#ifndef SCL_HIP_PREP_H
#define SCL_HIP_PREP_H

#include "scl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this boundary.  A binding checks it BEFORE it looks up symbols. */
#define SCL_PREP_ABI_VERSION 1
int         scl_prep_abi_version(void);          /* 1 */
const char* scl_prep_last_error(void);           /* per thread, like scl_hip_last_error */

/* scheme argument of scl_prep_triple_blocks */
#define SCL_PREP_ADDITIVE 0
#define SCL_PREP_SHAMIR   1
/* flags of scl_prep_triples_shamir_prg / scl_prep_triples_scratch_bytes: bit 0 forces the two-pass path */
#define SCL_PREP_TWO_PASS 1u

/* B of the discipline above: the AES blocks one triple consumes.  scheme 0 = additive (t ignored), 1 = Shamir; 0 for
 * arguments the deal calls refuse. */
size_t scl_prep_triple_blocks(int field, int scheme, size_t n, size_t t);

/* Bytes of device scratch scl_prep_triples_shamir_prg needs for this case: 0 where the fused kernel deals it (Mersenne61,
 * Mersenne127 and GF(2^128) at t <= 7, flags bit 0 clear), else (3 + 3t) * N elements (the two-pass path: the Montgomery
 * fields, t >= 8, or flags bit 0).  0 for arguments the call refuses. */
size_t scl_prep_triples_scratch_bytes(int field, size_t N, size_t n, size_t t, unsigned flags);

/* N additive triples among n >= 2 parties in ONE launch (two for Mersenne61 with two triples per lane and an odd N).
 * Nothing is read from device memory. */
int scl_prep_triples_additive_prg(int field, uint64_t* a_dev, uint64_t* b_dev, uint64_t* c_dev, size_t stride,
                                  size_t N, size_t n, const unsigned char* seed_host, size_t seed_len,
                                  uint64_t counter0, void* stream);

/* N Shamir (n, t) triples at the nodes 1..n, t <= 48 (t <= 16 for the 32-byte fields).  Fused (one launch, nothing read,
 * scratch_dev ignored and may be NULL) where scl_prep_triples_scratch_bytes is 0; else two passes: one launch writes a[N], b[N], c[N] and the 3t coefficient rows
 * [3t][N] into scratch_dev (16-byte aligned, not overlapping the matrices), then three calls of scl_hip_shamir_share
 * evaluate them on the same stream.  The two paths deal the same triples. */
int scl_prep_triples_shamir_prg(int field, uint64_t* a_dev, uint64_t* b_dev, uint64_t* c_dev, size_t stride,
                                size_t N, size_t t, size_t n, const unsigned char* seed_host, size_t seed_len,
                                uint64_t counter0, uint64_t* scratch_dev, unsigned flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCL_HIP_PREP_H */
