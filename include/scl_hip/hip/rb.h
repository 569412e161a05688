// include/scl_hip/hip/rb.h -- random shared bits over the device containers: batched square roots with a status per element and
// the fused last step of a batch of random bits, b[i][s] = (r[i][s] / sqrt(u[s]) + 1) / 2.  Thin calls into the C ABI of
// libscl_hip_rb.so (include/scl_hip_rb.h, which states the protocol, the canonical-root rule and the status codes), which a
// program links beside libscl_hip.so.  The per-element host forms are ss/random_bit.h.
#ifndef SCL_HIP_HIP_RB_H
#define SCL_HIP_HIP_RB_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../scl_hip_rb.h"
#include "device.h"

namespace scl::hip {

namespace rb_detail {
/// a status of libscl_hip_rb.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_rb_last_error); }
/// the status bytes on the host; synchronises the stream
inline std::vector<unsigned char> download(const DeviceBuffer& status, std::size_t n, void* stream) {
  std::vector<unsigned char> out(n);
  hip::check(scl_hip_stream_sync(stream));
  if (n) hip::check(scl_hip_memcpy_d2h(out.data(), status.get(), n, nullptr));
  return out;
}
}  // namespace rb_detail

template <typename T>
struct Roots {
  DeviceVector<T> values;             ///< the root (or its inverse); 0 where the status is not 0
  std::vector<unsigned char> status;  ///< 0 ok, 1 the input was zero, 2 a non-residue
};

template <typename T>
struct Bits {
  ShareMatrix<T> shares;              ///< every party's shares of the bits; a column whose status is not 0 is 0
  std::vector<unsigned char> status;  ///< per column
};

/// The square root of every element: the one with an even integer value (SCL_RB_ODD_ROOT: the odd one; SCL_RB_INVERSE: its
/// inverse).  The status bytes are fetched, so the call synchronises the stream.
template <typename T>
Roots<T> sqrt(const DeviceVector<T>& a, unsigned flags = 0, void* stream = nullptr) {
  Roots<T> out{DeviceVector<T>(a.size()), {}};
  DeviceBuffer status(a.size() ? a.size() : 1);
  rb_detail::check(scl_rb_sqrt(T::Field::TAG, out.values.data(), static_cast<unsigned char*>(status.get()), a.data(), a.size(), flags, stream));
  out.status = rb_detail::download(status, a.size(), stream);
  return out;
}

/// Every party's shares of the bits from the opened squares u (one per column of r) and the share matrix of r.
template <typename T>
Bits<T> bitsFinish(const DeviceVector<T>& u, const ShareMatrix<T>& r, void* stream = nullptr) {
  if (u.size() != r.secrets()) detail::raise(SCL_ERR_SIZE_MISMATCH);
  Bits<T> out{ShareMatrix<T>(r.parties(), r.secrets()), {}};
  DeviceBuffer status(u.size() ? u.size() : 1);
  rb_detail::check(scl_rb_bits_finish(T::Field::TAG, out.shares.data(), out.shares.stride(), static_cast<unsigned char*>(status.get()), u.data(), r.data(),
                                      r.stride(), r.parties(), r.secrets(), stream));
  out.status = rb_detail::download(status, u.size(), stream);
  return out;
}

}  // namespace scl::hip

#endif
