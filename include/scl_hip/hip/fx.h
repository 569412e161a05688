// include/scl_hip/hip/fx.h -- fixed-point arithmetic over the device containers: the bounded random value composed from planes of
// shared bits, and the two local steps of a probabilistic truncation for every party's row at once.  Thin calls into the C ABI of
// libscl_hip_fx.so (include/scl_hip_fx.h, which states the protocol, the ranges and the status), which a program links beside
// libscl_hip.so.  The per-secret host forms are ss/trunc.h.
//
// BIT PLANES are a ShareMatrix of `parties` rows and B * N columns: plane i of a party's row is its columns [i N, (i + 1) N) --
// what one hip::bitsFinish over B * N columns leaves (hip/rb.h), used without a copy.
#ifndef SCL_HIP_HIP_FX_H
#define SCL_HIP_HIP_FX_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../scl_hip_fx.h"
#include "device.h"

namespace scl::hip {

namespace fx_detail {
/// a status of libscl_hip_fx.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_fx_last_error); }
}  // namespace fx_detail

template <typename T>
struct Masked {
  ShareMatrix<T> c;     ///< every party's share of x + 2^(k-1) + r: open it
  ShareMatrix<T> rlow;  ///< every party's share of r'
};

template <typename T>
struct Truncated {
  ShareMatrix<T> shares;              ///< every party's shares of the truncated values; a column whose status is not 0 is 0
  std::vector<unsigned char> status;  ///< per column: 0 ok, 1 the opened c was at or above 2^(B+1)
};

/// Every party's shares of sum_i 2^i b_i: bits holds B planes of N columns per party.
template <typename T>
ShareMatrix<T> composeBits(const ShareMatrix<T>& bits, std::size_t B, void* stream = nullptr) {
  if (B == 0 || bits.secrets() % B) detail::raise(SCL_ERR_SIZE_MISMATCH);
  const std::size_t N = bits.secrets() / B;
  ShareMatrix<T> out(bits.parties(), N);
  fx_detail::check(scl_fx_compose(T::Field::TAG, out.data(), out.stride(), bits.data(), N, bits.stride(), B, bits.parties(), N, stream));
  return out;
}

/// Every party's mask of its shares x of signed k-bit values under its B = bits.secrets() / x.secrets() planes of random bits.
template <typename T>
Masked<T> truncMask(const ShareMatrix<T>& x, const ShareMatrix<T>& bits, std::size_t k, std::size_t shift, void* stream = nullptr) {
  const std::size_t N = x.secrets();
  if (N == 0 || bits.secrets() % N || bits.parties() != x.parties()) detail::raise(SCL_ERR_SIZE_MISMATCH);
  Masked<T> out{ShareMatrix<T>(x.parties(), N), ShareMatrix<T>(x.parties(), N)};
  fx_detail::check(scl_fx_trunc_mask(T::Field::TAG, out.c.data(), out.c.stride(), out.rlow.data(), out.rlow.stride(), x.data(), x.stride(), bits.data(), N,
                                     bits.stride(), k, shift, bits.secrets() / N, x.parties(), N, stream));
  return out;
}

/// The opening of c from its first lambda.size() rows (lambda: their Lagrange basis at 0) and the finish for every party's row.
/// The status bytes are fetched, so the call synchronises the stream.
template <typename T>
Truncated<T> truncFinish(const ShareMatrix<T>& c, const std::vector<T>& lambda, const ShareMatrix<T>& x, const ShareMatrix<T>& rlow, std::size_t shift,
                         std::size_t B, void* stream = nullptr) {
  const std::size_t N = x.secrets();
  if (lambda.empty() || lambda.size() > c.parties() || c.secrets() != N || rlow.secrets() != N || rlow.parties() != x.parties())
    detail::raise(SCL_ERR_SIZE_MISMATCH);
  std::vector<std::uint64_t> lam(lambda.size() * ShareMatrix<T>::LIMBS);
  for (std::size_t j = 0; j < lambda.size(); ++j) lambda[j].toLimbs(lam.data() + j * ShareMatrix<T>::LIMBS);
  Truncated<T> out{ShareMatrix<T>(x.parties(), N), std::vector<unsigned char>(N)};
  DeviceBuffer status(N ? N : 1);
  fx_detail::check(scl_fx_trunc_finish(T::Field::TAG, out.shares.data(), out.shares.stride(), static_cast<unsigned char*>(status.get()), c.data(), c.stride(),
                                       lam.data(), lambda.size(), x.data(), x.stride(), rlow.data(), rlow.stride(), shift, B, x.parties(), N, stream));
  hip::check(scl_hip_stream_sync(stream));
  if (N) hip::check(scl_hip_memcpy_d2h(out.status.data(), status.get(), N, nullptr));
  return out;
}

}  // namespace scl::hip

#endif
