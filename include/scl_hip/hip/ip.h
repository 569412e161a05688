// include/scl_hip/hip/ip.h -- inner and matrix products of Shamir sharings at one opening each, over device-resident share
// matrices: the local step [d]_2t = sum_k [x_k]_t [y_k]_t + [R]_2t of an inner product and of a batch of small matrix products.
// The open-and-subtract that follows is hip::mulFinish (hip/hm.h).  Thin calls into the C ABI of libscl_hip_ip.so
// (include/scl_hip_ip.h), which a program links beside libscl_hip.so.
#ifndef SCL_HIP_HIP_IP_H
#define SCL_HIP_HIP_IP_H

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "../../scl_hip_ip.h"
#include "device.h"

namespace scl::hip {

namespace ip_detail {
/// a status of libscl_hip_ip.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_ip_last_error); }
}  // namespace ip_detail

/// Every party's [d]_2t = sum_{k<terms} [x_k]_t [y_k]_t + [R]_2t in one launch.  x and y hold the terms one after another:
/// terms * n rows, row k * n + j = party j's shares of term k.  r2 (n rows) may be nullptr: a plain sum of products.
template <typename T>
ShareMatrix<T> dotMask(const ShareMatrix<T>& x, const ShareMatrix<T>& y, std::size_t terms, const ShareMatrix<T>* r2 = nullptr,
                       void* stream = nullptr) {
  if (terms == 0 || x.parties() % terms) detail::raise(SCL_ERR_SIZE_MISMATCH);
  const std::size_t n = x.parties() / terms, N = x.secrets();
  if (y.parties() != x.parties() || y.secrets() != N || (r2 && (r2->parties() != n || r2->secrets() != N))) detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> d(n, N);
  ip_detail::check(scl_ip_dot_mask(T::Field::TAG, d.data(), d.stride(), x.data(), n * x.stride(), y.data(), n * y.stride(),
                                   r2 ? r2->data() : nullptr, x.stride(), terms, n, N, stream));
  return d;
}

/// The output tile a lane of matmulMask owns for this field (rows, columns)
template <typename T>
std::pair<int, int> matmulTile() {
  int ti = 0, tl = 0;
  scl_ip_matmul_tile(T::Field::TAG, &ti, &tl);
  return {ti, tl};
}

/// Every party's [D]_2t = [X]_t [Y]_t + [R]_2t for N independent a x K by K x b products.  The matrices are row-major,
/// party after party: X has n * a * K rows (row (j * a + i) * K + k = party j's shares of entry (i, k)), Y n * K * b, r2 and
/// the result n * a * b.  r2 may be nullptr.  The result viewed as n rows of a * b * N columns is what hip::mulFinish takes.
template <typename T>
ShareMatrix<T> matmulMask(const ShareMatrix<T>& X, const ShareMatrix<T>& Y, std::size_t a, std::size_t K, std::size_t b,
                          const ShareMatrix<T>* r2 = nullptr, void* stream = nullptr) {
  if (a == 0 || K == 0 || b == 0 || X.parties() % (a * K)) detail::raise(SCL_ERR_SIZE_MISMATCH);
  const std::size_t n = X.parties() / (a * K), N = X.secrets();
  if (Y.parties() != n * K * b || Y.secrets() != N || (r2 && (r2->parties() != n * a * b || r2->secrets() != N))) detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> d(n * a * b, N);
  ip_detail::check(scl_ip_matmul_mask(T::Field::TAG, d.data(), d.stride(), a * b * d.stride(), X.data(), X.stride(), a * K * X.stride(), Y.data(),
                                      Y.stride(), K * b * Y.stride(), r2 ? r2->data() : nullptr, r2 ? r2->stride() : 0,
                                      r2 ? a * b * r2->stride() : 0, a, K, b, n, N, stream));
  return d;
}

}  // namespace scl::hip

#endif
