// include/scl_hip/hip/triples.h -- the trusted dealer of multiplication triples over device-resident share matrices: N triples
// in one call, the triples N calls of ss::randomTripleAdditive / ss::randomTripleShamir (ss/triples.h; the reference's
// randomTriple2, test/scl/protocol/triple.h:37-48) deal on one util::PRG with this seed from block counter0 on.  The result is
// the hip::Triple<hip::ShareMatrix<T>> hip::beaverMask and hip::beaverFinish take.  Thin calls into the C ABI of
// libscl_hip_prep.so (include/scl_hip_prep.h), which a program links beside libscl_hip.so.
#ifndef SCL_HIP_HIP_TRIPLES_H
#define SCL_HIP_HIP_TRIPLES_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../scl_hip_prep.h"
#include "../util/prg.h"
#include "beaver.h"
#include "device.h"

namespace scl::hip {

namespace triples_detail {
/// a status of libscl_hip_prep.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_prep_last_error); }
}  // namespace triples_detail

/// AES blocks one triple consumes: additive (t ignored) or Shamir (n, t); what a PRG advances by per triple
template <typename T>
std::uint64_t tripleBlocks(bool shamir, std::size_t n, std::size_t t = 0) {
  const std::size_t B = scl_prep_triple_blocks(T::Field::TAG, shamir ? SCL_PREP_SHAMIR : SCL_PREP_ADDITIVE, n, t);
  if (B == 0) throw std::invalid_argument("not a case the triple dealer accepts");
  return B;
}

/// N additive triples among n >= 2 parties
template <typename T>
Triple<ShareMatrix<T>> dealTriplesAdditive(std::size_t N, std::size_t n, const std::array<unsigned char, 16>& seed,
                                           std::uint64_t counter0 = 0, void* stream = nullptr) {
  Triple<ShareMatrix<T>> out{ShareMatrix<T>(n, N), ShareMatrix<T>(n, N), ShareMatrix<T>(n, N)};
  triples_detail::check(scl_prep_triples_additive_prg(T::Field::TAG, out.a.data(), out.b.data(), out.c.data(), out.a.stride(), N, n,
                                                      seed.data(), seed.size(), counter0, stream));
  return out;
}

/// N Shamir (n, t) triples at the nodes 1..n, t <= 48 (t <= 16 for the 32-byte fields: scl_hip_prep.h says why).  Where the case takes the two-pass path the scratch is allocated here and
/// released after the stream has run the call.
template <typename T>
Triple<ShareMatrix<T>> dealTriplesShamir(std::size_t N, std::size_t t, std::size_t n, const std::array<unsigned char, 16>& seed,
                                         std::uint64_t counter0 = 0, void* stream = nullptr) {
  Triple<ShareMatrix<T>> out{ShareMatrix<T>(n, N), ShareMatrix<T>(n, N), ShareMatrix<T>(n, N)};
  DeviceBuffer scratch(scl_prep_triples_scratch_bytes(T::Field::TAG, N, n, t, 0));
  triples_detail::check(scl_prep_triples_shamir_prg(T::Field::TAG, out.a.data(), out.b.data(), out.c.data(), out.a.stride(), N, t, n,
                                                    seed.data(), seed.size(), counter0, static_cast<std::uint64_t*>(scratch.get()), 0,
                                                    stream));
  if (scratch.bytes()) check(scl_hip_stream_sync(stream));
  return out;
}

/// the same on a util::PRG, which is advanced by the blocks the triples consumed
template <typename T>
Triple<ShareMatrix<T>> dealTriplesAdditive(std::size_t N, std::size_t n, util::PRG& prg, void* stream = nullptr) {
  auto out = dealTriplesAdditive<T>(N, n, prg.Seed(), prg.counter(), stream);
  prg.advance(N * tripleBlocks<T>(false, n));
  return out;
}
template <typename T>
Triple<ShareMatrix<T>> dealTriplesShamir(std::size_t N, std::size_t t, std::size_t n, util::PRG& prg, void* stream = nullptr) {
  auto out = dealTriplesShamir<T>(N, t, n, prg.Seed(), prg.counter(), stream);
  prg.advance(N * tripleBlocks<T>(true, n, t));
  return out;
}

}  // namespace scl::hip

#endif
