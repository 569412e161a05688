// include/scl_hip/hip/beaver.h -- Beaver multiplication over device-resident shares: the batch form of the reference's BeaverMul
// (test/scl/protocol/beaver.h:31-70).  hip::beaverMask is the arithmetic before the open step ([e] = [x] - [a], [d] = [y] - [b],
// beaver.h:40-41), hip::beaverFinish the arithmetic after it ([z] = e [b] + d [a] + [c], plus e d for the parties that add
// constants, beaver.h:57-61); the open step itself is what was there already (ss::shamirRecoverP / ss::additiveRecover in one
// process, hip/open.h across ranks).  Over hip::ShareMatrix all parties' rows go through one launch; over hip::DeviceVector one
// party works on its own shares, and its mask is the reference's packet: e, then d.  Thin calls into the C ABI of
// libscl_hip_mpc.so (include/scl_hip_mpc.h), which a program links beside libscl_hip.so.
#ifndef SCL_HIP_HIP_BEAVER_H
#define SCL_HIP_HIP_BEAVER_H

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../scl_hip_mpc.h"
#include "../math/lagrange.h"
#include "../math/vector.h"
#include "device.h"

namespace scl::hip {

/// A multiplication triple, c = a b: three values of one type, as in the reference's tests (test/scl/protocol/triple.h).  T
/// is whatever holds the shares: an element for one secret, a hip::DeviceVector for one party's shares of N triples, a
/// hip::ShareMatrix for every party's.
template <typename T>
struct Triple {
  T a;
  T b;
  T c;
};

namespace beaver_detail {
/// a status of libscl_hip_mpc.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_mpc_last_error); }
}  // namespace beaver_detail

/// What the parties send each other: rows 0..parties-1 are their shares of e, rows parties..2 parties-1 their shares of d.
template <typename T>
struct MaskedShares {
  ShareMatrix<T> de;
  std::size_t parties() const { return de.parties() / 2; }
  std::size_t secrets() const { return de.secrets(); }
  const std::uint64_t* eRows() const { return de.data(); }
  const std::uint64_t* dRows() const { return de.row(parties()); }
};

/// The opened values: e, then d, 2 N elements -- the layout of the reference's packet.
template <typename T>
struct OpenedMask {
  DeviceVector<T> ed;
  std::size_t secrets() const { return ed.size() / 2; }
  const std::uint64_t* e() const { return ed.data(); }
  const std::uint64_t* d() const { return ed.data() + secrets() * DeviceVector<T>::LIMBS; }
};

/// every party's [e] and [d] in one launch
template <typename T>
MaskedShares<T> beaverMask(const ShareMatrix<T>& x, const ShareMatrix<T>& y, const Triple<ShareMatrix<T>>& triple, void* stream = nullptr) {
  const std::size_t n = x.parties(), N = x.secrets();
  for (const ShareMatrix<T>* m : {&y, &triple.a, &triple.b})
    if (m->parties() != n || m->secrets() != N) detail::raise(SCL_ERR_SIZE_MISMATCH);
  MaskedShares<T> out{ShareMatrix<T>(2 * n, N)};
  beaver_detail::check(scl_mpc_beaver_mask(T::Field::TAG, out.de.data(), out.de.stride(), x.data(), y.data(), triple.a.data(),
                                           triple.b.data(), x.stride(), n, N, stream));
  return out;
}

/// one party's packet: its shares of e, then of d
template <typename T>
OpenedMask<T> beaverMask(const DeviceVector<T>& x, const DeviceVector<T>& y, const Triple<DeviceVector<T>>& triple, void* stream = nullptr) {
  const std::size_t N = x.size();
  if (y.size() != N || triple.a.size() != N || triple.b.size() != N) detail::raise(SCL_ERR_SIZE_MISMATCH);
  OpenedMask<T> out{DeviceVector<T>(2 * N)};
  beaver_detail::check(scl_mpc_beaver_mask(T::Field::TAG, out.ed.data(), N, x.data(), y.data(), triple.a.data(), triple.b.data(), N, 1, N,
                                           stream));
  return out;
}

/// the open step inside one process, Shamir shares at the nodes 1..n: e and d from every party's rows
template <typename T>
OpenedMask<T> beaverOpenShamir(const MaskedShares<T>& masked, void* stream = nullptr) {
  const std::size_t n = masked.parties(), N = masked.secrets(), L = DeviceVector<T>::LIMBS;
  const auto lambda = math::computeLagrangeBasis(math::Vector<T>::range(1, n + 1), T{});
  std::vector<std::uint64_t> lam(n * L);
  for (std::size_t i = 0; i < n; ++i) lambda[i].toLimbs(lam.data() + i * L);
  OpenedMask<T> out{DeviceVector<T>(2 * N)};
  check(scl_hip_shamir_recover(T::Field::TAG, out.ed.data(), masked.eRows(), masked.de.stride(), lam.data(), n, N, stream));
  check(scl_hip_shamir_recover(T::Field::TAG, out.ed.data() + N * L, masked.dRows(), masked.de.stride(), lam.data(), n, N, stream));
  return out;
}

/// the open step inside one process, additive shares: the sums of the rows
template <typename T>
OpenedMask<T> beaverOpenAdditive(const MaskedShares<T>& masked, void* stream = nullptr) {
  const std::size_t n = masked.parties(), N = masked.secrets(), L = DeviceVector<T>::LIMBS;
  OpenedMask<T> out{DeviceVector<T>(2 * N)};
  check(scl_hip_additive_recover(T::Field::TAG, out.ed.data(), masked.eRows(), masked.de.stride(), n, N, stream));
  check(scl_hip_additive_recover(T::Field::TAG, out.ed.data() + N * L, masked.dRows(), masked.de.stride(), n, N, stream));
  return out;
}

/// every party's [z]; the first `ed_parties` rows add e d (Shamir: all of them -- a constant is its own sharing; additive: 1,
/// row 0 being party 0)
template <typename T>
ShareMatrix<T> beaverFinish(const OpenedMask<T>& opened, const Triple<ShareMatrix<T>>& triple, std::size_t ed_parties, void* stream = nullptr) {
  const std::size_t n = triple.a.parties(), N = triple.a.secrets();
  if (opened.secrets() != N || triple.b.parties() != n || triple.b.secrets() != N || triple.c.parties() != n || triple.c.secrets() != N)
    detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> z(n, N);
  beaver_detail::check(scl_mpc_beaver_finish(T::Field::TAG, z.data(), z.stride(), opened.e(), opened.d(), triple.a.data(), triple.b.data(),
                                             triple.c.data(), triple.a.stride(), n, ed_parties, N, stream));
  return z;
}

/// one party's [z]; `adds_constant`: this party adds e d (beaver.h:59-61: party 0)
template <typename T>
DeviceVector<T> beaverFinish(const OpenedMask<T>& opened, const Triple<DeviceVector<T>>& triple, bool adds_constant, void* stream = nullptr) {
  const std::size_t N = triple.a.size();
  if (opened.secrets() != N || triple.b.size() != N || triple.c.size() != N) detail::raise(SCL_ERR_SIZE_MISMATCH);
  DeviceVector<T> z(N);
  beaver_detail::check(scl_mpc_beaver_finish(T::Field::TAG, z.data(), N, opened.e(), opened.d(), triple.a.data(), triple.b.data(),
                                             triple.c.data(), N, 1, adds_constant ? 1 : 0, N, stream));
  return z;
}

}  // namespace scl::hip

#endif  // SCL_HIP_HIP_BEAVER_H
