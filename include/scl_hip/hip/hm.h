// include/scl_hip/hip/hm.h -- honest-majority (Damgard-Nielsen) multiplication over device-resident share matrices: one
// dealer's N double sharings in one call (the sharings N calls of ss::doubleShare deal on one util::PRG with this seed from
// block counter0 on), a small matrix applied across share matrices (the extraction with Matrix::hyperInvertible), and the two
// local steps of a product.  Thin calls into the C ABI of libscl_hip_hm.so (include/scl_hip_hm.h), which a program links
// beside libscl_hip.so.
#ifndef SCL_HIP_HIP_HM_H
#define SCL_HIP_HIP_HM_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../scl_hip_hm.h"
#include "../math/lagrange.h"
#include "../math/matrix.h"
#include "../util/prg.h"
#include "device.h"

namespace scl::hip {

namespace hm_detail {
/// a status of libscl_hip_hm.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_hm_last_error); }
}  // namespace hm_detail

/// every party's shares of N secrets, twice: lo of degree t, hi of degree 2t
template <typename T>
struct DoubleSharings {
  ShareMatrix<T> lo;
  ShareMatrix<T> hi;
};

/// AES blocks one double sharing consumes; what a PRG advances by per double sharing
template <typename T>
std::uint64_t doubleBlocks(std::size_t n, std::size_t t) {
  const std::size_t B = scl_hm_double_blocks(T::Field::TAG, n, t);
  if (B == 0) throw std::invalid_argument("not a case the double-sharing dealer accepts");
  return B;
}

/// N double sharings of one dealer at the nodes 1..n, n > 2t.  Where the case takes the two-pass path the scratch is allocated
/// here and released after the stream has run the call.
template <typename T>
DoubleSharings<T> dealDoubleSharings(std::size_t N, std::size_t t, std::size_t n, const std::array<unsigned char, 16>& seed,
                                     std::uint64_t counter0 = 0, void* stream = nullptr) {
  DoubleSharings<T> out{ShareMatrix<T>(n, N), ShareMatrix<T>(n, N)};
  DeviceBuffer scratch(scl_hm_double_scratch_bytes(T::Field::TAG, N, n, t, 0));
  hm_detail::check(scl_hm_double_share_prg(T::Field::TAG, out.lo.data(), out.hi.data(), out.lo.stride(), N, t, n, seed.data(), seed.size(),
                                           counter0, static_cast<std::uint64_t*>(scratch.get()), 0, stream));
  if (scratch.bytes()) check(scl_hip_stream_sync(stream));
  return out;
}

/// the same on a util::PRG, which is advanced by the blocks the sharings consumed
template <typename T>
DoubleSharings<T> dealDoubleSharings(std::size_t N, std::size_t t, std::size_t n, util::PRG& prg, void* stream = nullptr) {
  auto out = dealDoubleSharings<T>(N, t, n, prg.Seed(), prg.counter(), stream);
  prg.advance(N * doubleBlocks<T>(n, t));
  return out;
}

/// Matrix::hyperInvertible(rows, cols) of the mirror (math/matrix.h; the reference's matrix.h:462-475)
template <typename T>
math::Matrix<T> hyperInvertible(std::size_t rows, std::size_t cols) {
  return math::Matrix<T>::hyperInvertible(rows, cols);
}
/// the same at chosen evaluation points: row i is the Lagrange basis of the nodes 1..cols at points[i].  Over GF(2^128), this
/// project's own field, -i = i collides with the nodes; there choose points outside 1..cols (the Python binding defaults to the
/// bit patterns cols + 1 + i).
template <typename T>
math::Matrix<T> hyperInvertible(std::size_t rows, std::size_t cols, const std::vector<T>& points) {
  if (points.size() != rows) throw std::invalid_argument("one evaluation point per row");
  math::Matrix<T> him(rows, cols);
  const auto nodes = math::Vector<T>::range(1, cols + 1);
  for (std::size_t i = 0; i < rows; ++i) {
    const auto r = math::computeLagrangeBasis(nodes, points[i]);
    for (std::size_t j = 0; j < cols; ++j) him(i, j) = r[j];
  }
  return him;
}

/// a matrix on the device, row-major: upload it once, apply it often
template <typename T>
DeviceVector<T> uploadMatrix(const math::Matrix<T>& M) {
  std::vector<T> flat;
  flat.reserve(M.rows() * M.cols());
  for (std::size_t i = 0; i < M.rows(); ++i)
    for (std::size_t j = 0; j < M.cols(); ++j) flat.push_back(M(i, j));
  return DeviceVector<T>(flat);
}

/// out row k = sum_i M[k][i] * (row i of in): M is rows x in.parties(), row-major on the device (uploadMatrix)
template <typename T>
ShareMatrix<T> applyMatrix(const DeviceVector<T>& M, std::size_t rows, const ShareMatrix<T>& in, void* stream = nullptr) {
  const std::size_t n = in.parties(), N = in.secrets();
  if (M.size() != rows * n) detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> out(rows, N);
  hm_detail::check(scl_hm_apply(T::Field::TAG, out.data(), out.stride(), 0, in.data(), in.stride(), 0, M.data(), n, rows, n, 1, N, stream));
  return out;
}

/// every party's [d]_2t = [x]_t [y]_t + [R]_2t in one launch
template <typename T>
ShareMatrix<T> mulMask(const ShareMatrix<T>& x, const ShareMatrix<T>& y, const ShareMatrix<T>& r2, void* stream = nullptr) {
  const std::size_t n = x.parties(), N = x.secrets();
  for (const ShareMatrix<T>* m : {&y, &r2})
    if (m->parties() != n || m->secrets() != N) detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> d(n, N);
  hm_detail::check(scl_hm_mul_mask(T::Field::TAG, d.data(), d.stride(), x.data(), y.data(), r2.data(), x.stride(), n, N, stream));
  return d;
}

/// every party's [z]_t = d - [R]_t, d opened from the shares of all parties (nodes 1..n, at most 64) in the same launch
template <typename T>
ShareMatrix<T> mulFinish(const ShareMatrix<T>& d, const ShareMatrix<T>& r, void* stream = nullptr) {
  const std::size_t n = d.parties(), N = d.secrets(), L = DeviceVector<T>::LIMBS;
  if (r.secrets() != N) detail::raise(SCL_ERR_SIZE_MISMATCH);
  const auto lambda = math::computeLagrangeBasis(math::Vector<T>::range(1, n + 1), T{});
  std::vector<std::uint64_t> lam(n * L);
  for (std::size_t i = 0; i < n; ++i) lambda[i].toLimbs(lam.data() + i * L);
  ShareMatrix<T> z(r.parties(), N);
  hm_detail::check(scl_hm_mul_finish(T::Field::TAG, z.data(), z.stride(), d.data(), d.stride(), lam.data(), n, r.data(), r.stride(),
                                     r.parties(), N, stream));
  return z;
}

}  // namespace scl::hip

#endif
