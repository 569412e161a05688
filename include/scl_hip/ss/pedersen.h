// include/scl_hip/ss/pedersen.h -- Pedersen verifiable secret sharing per secret on the host (include/scl/ss/pedersen.h:44-287).
// The batch forms are hip::Pedersen (hip/pedersen.h) over the C ABI's scl_hip_pedersen_commit / scl_hip_pedersen_verify /
// scl_hip_ec_matmul.
#ifndef SCL_HIP_SS_PEDERSEN_H
#define SCL_HIP_SS_PEDERSEN_H

#include <cstddef>
#include <utility>
#include <vector>

#include "../math/array.h"
#include "../math/lagrange.h"
#include "../math/matrix.h"
#include "../math/vector.h"
#include "../util/prg.h"
#include "shamir.h"

namespace scl::ss {

template <typename GROUP>
struct PedersenShare {  // pedersen.h:44-79
  using Group = GROUP;
  using Field = typename GROUP::ScalarField;
  math::Array<Field, 2> share;  ///< {share, randomness}
  math::Vector<Group> commitments;
  Field getRand() const { return share[1]; }
  Field getShare() const { return share[0]; }
};

template <typename GROUP>
struct PedersenSharing {  // pedersen.h:84-114
  using Group = GROUP;
  using Field = typename GROUP::ScalarField;
  math::Vector<math::Array<Field, 2>> shares;
  math::Vector<Group> commitments;
  PedersenShare<GROUP> getShare(std::size_t party_id) const { return {shares[party_id], commitments}; }
};

/// pedersen.h:126-149: a Shamir sharing of {secret, randomness} and a G + b h for each of f(0), f(1), .., f(t)
template <typename T>
PedersenSharing<T> pedersenSecretShare(const typename PedersenSharing<T>::Field& secret, std::size_t t, std::size_t n, util::PRG& prg,
                                       const typename PedersenSharing<T>::Group& h,
                                       const typename PedersenSharing<T>::Field& randomness) {
  using F = typename PedersenSharing<T>::Field;
  using G = typename PedersenSharing<T>::Group;
  const math::Array<F, 2> s = {{secret, randomness}};
  PedersenSharing<T> out;
  out.shares = shamirSecretShare(s, t, n, prg);
  std::vector<G> comm;
  comm.reserve(t + 1);
  const auto gen = G::generator();
  comm.emplace_back(secret * gen + randomness * h);
  for (std::size_t i = 0; i < t; ++i) comm.emplace_back(out.shares[i][0] * gen + out.shares[i][1] * h);
  out.commitments = math::Vector<G>(std::move(comm));
  return out;
}

/// pedersen.h:160-170: the randomness is drawn from the PRG before the sharing
template <typename GROUP>
PedersenSharing<GROUP> pedersenSecretShare(const typename PedersenSharing<GROUP>::Field& secret, std::size_t t, std::size_t n,
                                           util::PRG& prg, const typename PedersenSharing<GROUP>::Group& h) {
  using F = typename PedersenSharing<GROUP>::Field;
  const auto rand = F::random(prg);
  return pedersenSecretShare<GROUP>(secret, t, n, prg, h, rand);
}

/// pedersen.h:178-191
template <typename GROUP>
GROUP computeCommitmentForIndex(const math::Vector<GROUP>& commitments, std::size_t share_index) {
  if (share_index < commitments.size()) return commitments[share_index];
  using Field = typename PedersenShare<GROUP>::Field;
  const auto ns = math::Vector<Field>::range(commitments.size());
  const auto lb = math::computeLagrangeBasis(ns, static_cast<int>(share_index));
  GROUP v{};
  auto c = commitments.begin();
  for (auto l = lb.begin(); l != lb.end(); ++l, ++c) v += *l * *c;
  return v;
}

/// pedersen.h:200-207
template <typename GROUP>
bool pedersenVerify(const PedersenShare<GROUP> share, std::size_t share_index, const typename PedersenShare<GROUP>::Group& h) {
  using Group = typename PedersenShare<GROUP>::Group;
  return computeCommitmentForIndex(share.commitments, share_index) == share.getShare() * Group::generator() + share.getRand() * h;
}

/// pedersen.h:217-224
template <typename T>
bool pedersenVerify(const math::Array<typename PedersenSharing<T>::Field, 2>& share,
                    const math::Vector<typename PedersenSharing<T>::Group>& commitments, std::size_t share_index,
                    const typename PedersenShare<T>::Group& h) {
  return pedersenVerify<T>({share, commitments}, share_index, h);
}

/// pedersen.h:236-274: a matrix applied to a list of shares from the left (DN07's randomisation): out[i] = sum_k M(i, k) in[k],
/// shares and commitments alike
template <typename T, typename IT>
std::vector<PedersenShare<T>> apply(const IT begin, const IT end, const math::Matrix<typename PedersenShare<T>::Field>& matrix) {
  std::vector<PedersenShare<T>> out;
  if (begin == end) return out;
  using Group = typename PedersenShare<T>::Group;
  const std::size_t width = begin->commitments.size();
  out.resize(matrix.rows());
  for (std::size_t row = 0; row < matrix.rows(); ++row) {
    PedersenShare<T>& sum = out[row];  // share {0, 0}, commitments all infinity
    sum.commitments = math::Vector<Group>(width);
    IT term = begin;
    for (std::size_t col = 0; col < matrix.cols(); ++col, ++term) {  // as the reference: matrix.cols() terms are read
      const auto coefficient = matrix(row, col);
      sum.share += term->share * coefficient;
      for (std::size_t c = 0; c < width; ++c) sum.commitments[c] += coefficient * term->commitments[c];
    }
  }
  return out;
}

/// pedersen.h:282-287
template <typename T>
std::vector<PedersenShare<T>> apply(const std::vector<PedersenShare<T>>& shares,
                                    const math::Matrix<typename PedersenShare<T>::Field>& matrix) {
  return apply<T>(shares.begin(), shares.end(), matrix);
}

}  // namespace scl::ss

#endif
