// include/scl_hip/hip/vf.h -- batch verification over device-resident share matrices: random linear combinations of sharings
// along N, out[r][j] = sum_s rho_j[s] x[r][s] (y[r][s]).  The result -- parties x reps -- is the share matrix
// hip::shamirRecoverD takes with reps columns.  Thin calls into the C ABI of libscl_hip_vf.so (include/scl_hip_vf.h), which a
// program links beside libscl_hip.so.  The per-instance host form is ss/vf.h.
#ifndef SCL_HIP_HIP_VF_H
#define SCL_HIP_HIP_VF_H

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../scl_hip_vf.h"
#include "device.h"

namespace scl::hip {

namespace vf_detail {
/// a status of libscl_hip_vf.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_vf_last_error); }
inline DeviceBuffer scratch(int tag, std::size_t rows, std::size_t reps, std::size_t N, unsigned flags, std::size_t* bytes) {
  *bytes = scl_vf_scratch_bytes(tag, rows, reps, N, flags);
  if (rows && !*bytes) throw std::runtime_error(std::string(scl_hip_status_message(SCL_ERR_BAD_ARG)) + ": combine: reps outside 1..4, or rows * reps * N overflows");
  return DeviceBuffer(*bytes ? *bytes : 16);
}
}  // namespace vf_detail

/// The AES blocks one Vector<T>::random(N, prg) consumes
template <typename T>
std::size_t coinBlocks(std::size_t N) {
  return scl_vf_coin_blocks(T::Field::TAG, N);
}

/// Every row's reps combinations with the coin drawn on the device: rho_j is the j-th consecutive Vector<T>::random(N, prg) of a
/// util::PRG on `seed` whose block counter stands at counter0.  y == nullptr: the plain form.  The result has x.parties() rows
/// of reps columns.  The scratch is allocated here and freed on return, so the call synchronises the stream (as hip::doubleShare
/// does on its two-pass path); a caller that must not synchronise owns the scratch and calls the C ABI.
template <typename T>
ShareMatrix<T> combinePrg(const ShareMatrix<T>& x, const ShareMatrix<T>* y, std::size_t reps, const unsigned char* seed, std::size_t seed_len,
                          std::uint64_t counter0 = 0, void* stream = nullptr) {
  if (y && (y->parties() != x.parties() || y->secrets() != x.secrets())) detail::raise(SCL_ERR_SIZE_MISMATCH);
  std::size_t bytes = 0;
  DeviceBuffer scratch = vf_detail::scratch(T::Field::TAG, x.parties(), reps, x.secrets(), SCL_VF_PRG, &bytes);
  ShareMatrix<T> out(x.parties(), reps);
  vf_detail::check(scl_vf_combine_prg(T::Field::TAG, out.data(), out.stride(), x.data(), y ? y->data() : nullptr, x.stride(), x.parties(), x.secrets(),
                                      reps, seed, seed_len, counter0, static_cast<std::uint64_t*>(scratch.get()), bytes, stream));
  check(scl_hip_stream_sync(stream));  // the scratch is freed on return
  return out;
}

/// The same with the coefficient rows given: rho has reps rows of N columns.
template <typename T>
ShareMatrix<T> combine(const ShareMatrix<T>& x, const ShareMatrix<T>* y, const ShareMatrix<T>& rho, void* stream = nullptr) {
  if (rho.secrets() != x.secrets() || (y && (y->parties() != x.parties() || y->secrets() != x.secrets()))) detail::raise(SCL_ERR_SIZE_MISMATCH);
  std::size_t bytes = 0;
  DeviceBuffer scratch = vf_detail::scratch(T::Field::TAG, x.parties(), rho.parties(), x.secrets(), 0, &bytes);
  ShareMatrix<T> out(x.parties(), rho.parties());
  vf_detail::check(scl_vf_combine(T::Field::TAG, out.data(), out.stride(), x.data(), y ? y->data() : nullptr, x.stride(), rho.data(), rho.stride(),
                                  x.parties(), x.secrets(), rho.parties(), static_cast<std::uint64_t*>(scratch.get()), bytes, stream));
  check(scl_hip_stream_sync(stream));  // the scratch is freed on return
  return out;
}

}  // namespace scl::hip

#endif
