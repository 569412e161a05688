// include/scl_hip/ss/feldman.h -- Feldman verifiable secret sharing per secret on the host (include/scl/ss/feldman.h:36-163).
// The batch forms are the C ABI's scl_hip_feldman_commit / scl_hip_feldman_verify.
#ifndef SCL_HIP_SS_FELDMAN_H
#define SCL_HIP_SS_FELDMAN_H

#include <cstddef>
#include <utility>
#include <vector>

#include "../math/lagrange.h"
#include "../math/vector.h"
#include "../util/prg.h"
#include "shamir.h"

namespace scl::ss {

template <typename GROUP>
struct FeldmanShare {  // feldman.h:36-57
  using Group = GROUP;
  using Field = typename GROUP::ScalarField;
  Field share;
  math::Vector<Group> commitments;
};

template <typename GROUP>
struct FeldmanSharing {  // feldman.h:67-97
  using Group = GROUP;
  using Field = typename GROUP::ScalarField;
  math::Vector<Field> shares;
  math::Vector<GROUP> commitments;
  FeldmanShare<GROUP> getShare(std::size_t party_id) const { return {shares[party_id], commitments}; }
};

/// feldman.h:107-124: a Shamir sharing of the secret and G times each of f(0) = secret, f(1), .., f(t)
template <typename GROUP>
FeldmanSharing<GROUP> feldmanSecretShare(const typename FeldmanSharing<GROUP>::Field& secret, std::size_t t, std::size_t n,
                                         util::PRG& prg) {
  FeldmanSharing<GROUP> out;
  out.shares = shamirSecretShare(secret, t, n, prg);
  std::vector<GROUP> points(t + 1, GROUP::generator());
  points[0] *= secret;
  for (std::size_t k = 1; k <= t; ++k) points[k] *= out.shares[k - 1];
  out.commitments = math::Vector<GROUP>(std::move(points));
  return out;
}

/// feldman.h:136-144
template <typename GROUP>
bool feldmanVerify(const FeldmanShare<GROUP>& share, std::size_t share_index) {
  using F = typename GROUP::ScalarField;
  const auto ns = math::Vector<F>::range(share.commitments.size());
  const auto lb = math::computeLagrangeBasis(ns, static_cast<int>(share_index));
  GROUP v{};
  auto c = share.commitments.begin();
  for (auto l = lb.begin(); l != lb.end(); ++l, ++c) v += *l * *c;
  return v == GROUP::generator() * share.share;
}

/// feldman.h:157-163
template <typename GROUP>
bool feldmanVerify(const typename FeldmanShare<GROUP>::Field& share,
                   const math::Vector<typename FeldmanShare<GROUP>::Group>& commitments, std::size_t share_index) {
  return feldmanVerify<GROUP>({share, commitments}, share_index);
}

}  // namespace scl::ss

#endif
