// csrc/launch_rules.hpp -- the arithmetic of the engine's launches that needs no device: grid sizes, the residency pad, the
// matrix-core shape and the step from a run-time integer to a template argument.  Plain C++17 without a HIP include, so a
// host program checks it (tests/cxx/launch_rules_check.cc).
#pragma once

#include <cstddef>
#include <type_traits>
#include <utility>

namespace sclhip {

// blocks of `block` items over `work` items, at most `cap` (cap <= 0: 2^31 - 1), at least one
inline unsigned grid_cap(size_t work, int block, long cap) {
  size_t blocks = (work + block - 1) / block;
  if (cap <= 0) cap = 0x7fffffff;
  if (blocks > (size_t)cap) blocks = (size_t)cap;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}

// dynamic LDS bytes that cap the residency of a kernel with `static_lds` bytes of its own at `waves` waves of
// `block` threads per CU.  A CU has 160 KiB of LDS and hands it out in granules; the granule of gfx950 is not documented
// (512 B on earlier parts, 1280 B = 1/128 of the array is the other candidate), so the request is chosen to hold for BOTH:
// `groups` allocations fit, `groups + 1` do not, whichever granule rounds it up.  No such size exists for every count
// (24 and more groups per CU): then no cap is applied.
inline size_t residency_pad(long waves, int block, size_t static_lds) {
  if (waves <= 0) return 0;
  const size_t groups = (size_t)(waves * 64 / block);
  if (groups < 1) return 0;
  constexpr size_t LDS = 160 * 1024;
  auto holds = [&](size_t total, size_t granule) {
    const size_t alloc = (total + granule - 1) / granule * granule;
    return groups * alloc <= LDS && (groups + 1) * alloc > LDS;
  };
  for (size_t total = LDS / groups / 128 * 128; total > static_lds && total >= 1024; total -= 128)
    if (holds(total, 512) && holds(total, 1280)) return total <= 64 * 1024 ? total - static_lds : 0;
  return 0;
}

// The matrix-core sharing kernels' shape for `rows` rows (parties) and an inner dimension of k (t + 1): k-steps and row tiles.
// (one row tile with two k-steps would need 160 KiB for the staged right factor: such shapes take two row tiles)
struct MfmaShape {
  int KS, MT;
};
inline MfmaShape mfma_shape(size_t rows, size_t k) {
  const int KS = k <= 32 ? 1 : 2;
  return {KS, (rows <= 32 && KS == 1) ? 1 : rows <= 64 ? 2 : 4};
}

// fn(std::integral_constant<int, V>{}) for the V among V... that equals v; whether there was one
template <int... V, class Fn>
inline bool dispatch_of(long v, Fn&& fn) {
  return ((v == V ? (fn(std::integral_constant<int, V>{}), true) : false) || ...);
}

namespace detail {
template <int Lo, int... I, class Fn>
inline bool dispatch_seq(long v, std::integer_sequence<int, I...>, Fn&& fn) {
  return dispatch_of<(Lo + I)...>(v, fn);
}
}  // namespace detail

// the same for the V in [Lo, Hi]
template <int Lo, int Hi, class Fn>
inline bool dispatch_int(long v, Fn&& fn) {
  return detail::dispatch_seq<Lo>(v, std::make_integer_sequence<int, Hi - Lo + 1>{}, fn);
}

}  // namespace sclhip
