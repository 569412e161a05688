// include/scl_hip/util/digest.h -- scl::util::Digest<BITS> (include/scl/util/digest.h:31-48): a hash value as an array of bytes.
#ifndef SCL_HIP_UTIL_DIGEST_H
#define SCL_HIP_UTIL_DIGEST_H

#include <array>
#include <cstddef>
#include <string>

namespace scl::util {

template <std::size_t BITS>
using Digest = std::array<unsigned char, BITS / 8>;

/// lower-case hex, first byte first
template <typename DIGEST>
std::string digestToString(const DIGEST& digest) {
  static const char* hex = "0123456789abcdef";
  std::string s;
  s.reserve(2 * digest.size());
  for (unsigned char b : digest) {
    s.push_back(hex[b >> 4]);
    s.push_back(hex[b & 15]);
  }
  return s;
}

}  // namespace scl::util

#endif  // SCL_HIP_UTIL_DIGEST_H
