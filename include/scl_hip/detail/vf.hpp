// include/scl_hip/detail/vf.hpp -- the per-element arithmetic of batch verification, once, for host and device: random linear
// combinations of sharings along N,
//
//   plain     out_j = sum_s rho_j[s] x[s]
//   product   out_j = sum_s rho_j[s] (x[s] y[s])
//
// for REPS coefficient vectors rho_j that meet the same x (and y).  The accumulator is any type with zero / mac / add / fold and
// a TERMS bound, as in ip.hpp: IpAcc<F> (host and device) or the matrix kernels' MatAcc<F> (csrc/kernels.hpp, device only).
//
// THE COUNT is ip_take_term's (ip.hpp), not restated here.  The REPS accumulators of a column take their terms together and
// share one count: before a term goes in, accumulators that have reached F::ACC_TERMS terms (Mersenne61: 64) fold into
// themselves.  In the product form x y is reduced to an element FIRST and then multiplied by rho: rho (x y) is one product of
// two canonical elements, one term, so the bound is the one the accumulator promises (an unreduced triple product of Mersenne61
// elements has 183 bits and fits nothing).  The second stage adds canonical partial sums under the same count.  Field addition
// is exact and every residue has one canonical representative, so the value does not depend on the order in which lanes,
// workgroups and stages add: it is bit-identical to the same sum built one reduced operation at a time
// (tests/cxx/vf_host_check.cc).
#pragma once

#include "ip.hpp"

namespace sclhip {

// acc[j] += rho[j] * (x or x y) for j < REPS: one term for all REPS accumulators
template <class F, int REPS, bool PROD, class A>
SCL_HD void vf_take(const typename F::Ctx& ctx, A* acc, int& terms, const typename F::E* rho, const typename F::E& x, const typename F::E& y) {
  ip_take_term<F, REPS>(ctx, acc, terms);
  const typename F::E m = PROD ? F::mul(ctx, x, y) : x;
#pragma unroll
  for (int j = 0; j < REPS; ++j) acc[j].mac(ctx, rho[j], m);
}

// acc += part, a canonical partial sum: one term (the second stage)
template <class F, class A>
SCL_HD void vf_take_partial(const typename F::Ctx& ctx, A& acc, int& terms, const typename F::E& part) {
  ip_take_term<F, 1>(ctx, &acc, terms);
  acc.add(ctx, part);
}

// sum_{s<n} rho[s] x[s] (y[s]); y == nullptr: the plain form.  One column range on the field's own accumulator -- what the host
// check and the C++ mirror's host form run.
template <class F>
SCL_HD typename F::E vf_combine_one(const typename F::Ctx& ctx, const typename F::E* rho, const typename F::E* x, const typename F::E* y, size_t n) {
  IpAcc<F> acc;
  acc.zero();
  int terms = 0;
  for (size_t s = 0; s < n; ++s) {
    if (y) vf_take<F, 1, true>(ctx, &acc, terms, rho + s, x[s], y[s]);
    else vf_take<F, 1, false>(ctx, &acc, terms, rho + s, x[s], x[s]);
  }
  return acc.fold(ctx);
}

// the second stage on the host: the sum of n canonical partials under the count
template <class F>
SCL_HD typename F::E vf_sum_partials(const typename F::Ctx& ctx, const typename F::E* part, size_t n) {
  IpAcc<F> acc;
  acc.zero();
  int terms = 0;
  for (size_t k = 0; k < n; ++k) vf_take_partial<F>(ctx, acc, terms, part[k]);
  return acc.fold(ctx);
}

// ---- the launch geometry, shared by the entry points, scl_vf_scratch_bytes and scl_vf_launch_shape ---------------------------
// A pack is two columns for Mersenne61 and one for the other fields.  The streaming form runs 256-lane workgroups, at most
// VF_GRID_STREAM of them along N; the fused AES form runs 1024-lane workgroups, one per CU (they share the 128 KiB of AES
// tables).  What a lane holds per trip -- reps x U coefficient packs, U packs of x (and y), R x reps accumulators -- is what
// compiles without scratch or spills (docs/kernels/vf.md has the register figures).
constexpr size_t VF_THREADS_STREAM = 256, VF_THREADS_AES = 1024;
constexpr size_t VF_GRID_STREAM = 1024, VF_GRID_AES = 256;
constexpr size_t VF_REPS_MAX = 4;

constexpr size_t vf_cols_per_pack(size_t limbs) { return limbs == 1 ? 2 : 1; }
// repetitions one launch serves: the 32-byte fields hold two repetitions' accumulators and coefficients, so three and four are
// two launches
constexpr size_t vf_reps_per_launch(size_t limbs) { return limbs == 4 ? 2 : 4; }
// U, the packs of columns a lane takes per trip.  Streaming: 16-byte loads, four in flight per operand for the one- and two-limb
// fields (two from three repetitions on for the two-limb ones), two packs of two loads for the 32-byte fields (as ip_unit's
// dot_unroll).  Fused: two AES blocks a trip, one from two repetitions on.
constexpr int vf_unroll(size_t limbs, bool aes, size_t reps) {
  return aes ? (reps <= 1 ? 2 : 1) : (limbs == 1 ? 4 : limbs == 2 ? (reps >= 3 ? 2 : 4) : 2);
}
// columns one workgroup covers per trip
constexpr size_t vf_cols_per_trip(size_t limbs, bool aes, size_t reps) {
  return (aes ? VF_THREADS_AES : VF_THREADS_STREAM) * (size_t)vf_unroll(limbs, aes, reps) * vf_cols_per_pack(limbs);
}
// workgroups along N = partial sums per (row, repetition); at least one, so that N == 0 writes zeros through the same path
constexpr size_t vf_groups(size_t limbs, bool aes, size_t reps, size_t N) {
  const size_t per = vf_cols_per_trip(limbs, aes, reps), cap = aes ? VF_GRID_AES : VF_GRID_STREAM;
  const size_t g = N / per + (N % per != 0);
  return g < 1 ? 1 : g > cap ? cap : g;
}
// R: rows of x a lane keeps accumulators for, by element width and repetitions -- R * reps accumulators a lane: eight for
// Mersenne61, four for the 16-byte fields, two for the 32-byte fields; three repetitions run on the budget of four.  A call of
// more repetitions than a launch serves has the R of its first launch.
constexpr int vf_rows_per_group(size_t limbs, bool aes, size_t reps) {
  if (aes && reps <= 2) return 5;  // 1024-lane workgroups have 128 registers a lane; ten parties are two groups
  const int budget = limbs == 1 ? 8 : limbs == 2 ? 4 : 2;
  const size_t lr = reps < vf_reps_per_launch(limbs) ? reps : vf_reps_per_launch(limbs);
  const int r = budget / (int)(lr >= 3 ? 4 : lr == 2 ? 2 : 1);
  return r < 1 ? 1 : r;
}
// the fields whose scl_vf_combine_prg draws the coin in registers, by tag (scl_hip.h): Mersenne61; the others fill coefficient
// rows first (docs/kernels/vf.md says why)
constexpr bool vf_fused(int tag) { return tag == 0; }

}  // namespace sclhip
