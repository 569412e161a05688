// include/scl_hip/util/iuf_hash.h -- scl::util::IUFHash<HASH> (include/scl/util/iuf_hash.h:41-105): the init / update /
// finalize interface of the hash functions.  HASH supplies hash(bytes, n) and write(); the five update overloads -- raw bytes,
// a byte vector, a byte array, a string view and anything with a seri::Serializer -- all end in the first.
#ifndef SCL_HIP_UTIL_IUF_HASH_H
#define SCL_HIP_UTIL_IUF_HASH_H

#include <array>
#include <cstddef>
#include <string_view>
#include <vector>

#include "../serialization/serializer.h"

namespace scl::util {

template <typename HASH>
struct IUFHash {
  IUFHash<HASH>& update(const unsigned char* bytes, std::size_t n) {
    static_cast<HASH*>(this)->hash(bytes, n);
    return *this;
  }
  IUFHash<HASH>& update(const std::vector<unsigned char>& data) { return update(data.data(), data.size()); }
  template <std::size_t N>
  IUFHash<HASH>& update(const std::array<unsigned char, N>& data) {
    return update(data.data(), N);
  }
  IUFHash<HASH>& update(std::string_view text) { return update(reinterpret_cast<const unsigned char*>(text.data()), text.size()); }
  /// the Serializer image of `data` (an FF: its byteSize() canonical bytes, ff.h:355-391)
  template <typename T>
  IUFHash<HASH>& update(const T& data) {
    std::vector<unsigned char> image(seri::Serializer<T>::sizeOf(data));
    seri::Serializer<T>::write(data, image.data());
    return update(image.data(), image.size());
  }
  auto finalize() { return static_cast<HASH*>(this)->write(); }
};

}  // namespace scl::util

#endif  // SCL_HIP_UTIL_IUF_HASH_H
