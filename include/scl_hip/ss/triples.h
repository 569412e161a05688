// include/scl_hip/ss/triples.h -- the trusted dealer of multiplication triples, one triple per call, on the host: the
// per-secret surface of the reference's test/scl/protocol/triple.h.  randomTripleAdditive<T>(2, prg) is randomTriple2<T>(prg)
// (triple.h:37-48) literally; with n parties its `2` is n, and randomTripleShamir puts shamirSecretShare(v, t, n, prg)
// (shamir.h:51-68) where additiveShare stands.  The draws come in the reference's order -- a, b, then the sharings of a, of b
// and of c = a b -- so a run of these calls on one util::PRG deals what hip::dealTriplesAdditive / hip::dealTriplesShamir
// (hip/triples.h) deal from the same seed and counter, word for word.
#ifndef SCL_HIP_SS_TRIPLES_H
#define SCL_HIP_SS_TRIPLES_H

#include <cstddef>
#include <stdexcept>
#include <vector>

#include "../hip/beaver.h"
#include "../util/prg.h"
#include "additive.h"
#include "shamir.h"

namespace scl::ss {

namespace triples_detail {
template <typename T, typename SHARE>
std::vector<hip::Triple<T>> deal(std::size_t n, util::PRG& prg, SHARE&& share) {
  const T a = T::random(prg);  // triple.h:39-41
  const T b = T::random(prg);
  const T c = a * b;
  const auto as = share(a);  // triple.h:43-45
  const auto bs = share(b);
  const auto cs = share(c);
  std::vector<hip::Triple<T>> out;
  out.reserve(n);
  for (std::size_t i = 0; i < n; ++i) out.push_back(hip::Triple<T>{as[i], bs[i], cs[i]});
  return out;
}
}  // namespace triples_detail

/// party i's triple at [i]: additive shares of a, b and c = a b among n >= 2 parties
template <typename T>
std::vector<hip::Triple<T>> randomTripleAdditive(std::size_t n, util::PRG& prg) {
  if (n < 2) throw std::invalid_argument("a triple is dealt to at least 2 parties");
  return triples_detail::deal<T>(n, prg, [&](const T& v) { return additiveShare(v, n, prg); });
}

/// party i's triple at [i]: Shamir (n, t) shares at the nodes 1..n
template <typename T>
std::vector<hip::Triple<T>> randomTripleShamir(std::size_t t, std::size_t n, util::PRG& prg) {
  if (n == 0) throw std::invalid_argument("cannot create shares for 0 people");
  return triples_detail::deal<T>(n, prg, [&](const T& v) { return shamirSecretShare(v, t, n, prg); });
}

}  // namespace scl::ss

#endif
