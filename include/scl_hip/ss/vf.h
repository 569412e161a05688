// include/scl_hip/ss/vf.h -- batch verification, one instance per call, on the host: the random linear combination of short
// vectors with the coin drawn as a reference program draws it -- reps consecutive Vector<T>::random(N, prg) off one util::PRG
// (vector.h:507-519) -- and math::innerProd (vector.h:45-52).  A run on a PRG that stands at block counter0 computes what
// hip::combinePrg (hip/vf.h) computes from the same seed and counter, word for word.
#ifndef SCL_HIP_SS_VF_H
#define SCL_HIP_SS_VF_H

#include <cstddef>
#include <stdexcept>
#include <vector>

#include "../math/vector.h"
#include "../util/prg.h"

namespace scl::ss {

/// reps coefficient vectors of N elements, drawn one after the other
template <typename T>
std::vector<math::Vector<T>> combineCoins(std::size_t N, std::size_t reps, util::PRG& prg) {
  if (reps == 0 || reps > 4) throw std::invalid_argument("reps must be at least 1 and at most 4");
  std::vector<math::Vector<T>> rho;
  for (std::size_t j = 0; j < reps; ++j) rho.push_back(math::Vector<T>::random(N, prg));
  return rho;
}

/// out[j] = sum_s rho[j][s] x[s]: one row against every coefficient vector; the empty sum is zero
template <typename T>
std::vector<T> combine(const math::Vector<T>& x, const std::vector<math::Vector<T>>& rho) {
  std::vector<T> out;
  for (const auto& r : rho) {
    if (r.size() != x.size()) throw std::invalid_argument("Vec sizes mismatch");
    out.push_back(math::innerProd<T>(r.begin(), r.end(), x.begin()));
  }
  return out;
}

/// out[j] = sum_s rho[j][s] x[s] y[s]: x y is reduced first, then multiplied by rho
template <typename T>
std::vector<T> combine(const math::Vector<T>& x, const math::Vector<T>& y, const std::vector<math::Vector<T>>& rho) {
  return combine(x.multiplyEntryWise(y), rho);
}

}  // namespace scl::ss

#endif
