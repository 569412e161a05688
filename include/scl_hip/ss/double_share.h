// include/scl_hip/ss/double_share.h -- one double sharing per call, on the host: a fresh r shared twice, at degree t and at
// degree 2t, the preprocessing unit of honest-majority (Damgard-Nielsen) multiplication.  The draws come in the order a
// reference program produces that writes r = FF::random(prg), shamirSecretShare(r, t, n, prg), shamirSecretShare(r, 2t, n, prg)
// (ff.h:72-76, shamir.h:51-68) -- so a run of these calls on one util::PRG deals what hip::dealDoubleSharings (hip/hm.h) deals
// from the same seed and counter, word for word.
#ifndef SCL_HIP_SS_DOUBLE_SHARE_H
#define SCL_HIP_SS_DOUBLE_SHARE_H

#include <cstddef>
#include <stdexcept>
#include <vector>

#include "../util/prg.h"
#include "shamir.h"

namespace scl::ss {

/// party i's shares at [i]: lo of degree t, hi of degree 2t, of one secret
template <typename T>
struct DoubleSharing {
  std::vector<T> lo;
  std::vector<T> hi;
};

/// a double sharing of a fresh random secret among n > 2t parties at the nodes 1..n
template <typename T>
DoubleSharing<T> doubleShare(std::size_t t, std::size_t n, util::PRG& prg) {
  if (n <= 2 * t) throw std::invalid_argument("a degree-2t sharing among n <= 2t parties cannot be opened");
  const T r = T::random(prg);
  const auto lo = shamirSecretShare(r, t, n, prg);
  const auto hi = shamirSecretShare(r, 2 * t, n, prg);
  DoubleSharing<T> out;
  for (std::size_t i = 0; i < n; ++i) {
    out.lo.push_back(lo[i]);
    out.hi.push_back(hi[i]);
  }
  return out;
}

}  // namespace scl::ss

#endif
