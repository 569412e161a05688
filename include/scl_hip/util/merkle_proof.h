// include/scl_hip/util/merkle_proof.h -- scl::util::MerkleProof<DIGEST> (include/scl/util/merkle_proof.h:32-84): the siblings
// on the way from a leaf to the root and, per level, whether the sibling is the LEFT operand.  Image: the path as a vector
// (u32 count, digests), then the bitmap (u32 byte count, bytes).
#ifndef SCL_HIP_UTIL_MERKLE_PROOF_H
#define SCL_HIP_UTIL_MERKLE_PROOF_H

#include <cstddef>
#include <vector>

#include "../serialization/serializer.h"
#include "bitmap.h"

namespace scl {
namespace util {

template <typename DIGEST>
struct MerkleProof {
  std::vector<DIGEST> path;
  Bitmap direction;
};

}  // namespace util

namespace seri {
template <typename DIGEST>
struct Serializer<util::MerkleProof<DIGEST>, void> {
  using Path = Serializer<std::vector<DIGEST>>;
  static std::size_t sizeOf(const util::MerkleProof<DIGEST>& p) { return Path::sizeOf(p.path) + Serializer<util::Bitmap>::sizeOf(p.direction); }
  static std::size_t write(const util::MerkleProof<DIGEST>& p, unsigned char* buf) {
    const std::size_t at = Path::write(p.path, buf);
    return at + Serializer<util::Bitmap>::write(p.direction, buf + at);
  }
  static std::size_t read(util::MerkleProof<DIGEST>& p, const unsigned char* buf) {
    const std::size_t at = Path::read(p.path, buf);
    return at + Serializer<util::Bitmap>::read(p.direction, buf + at);
  }
};
}  // namespace seri
}  // namespace scl

#endif  // SCL_HIP_UTIL_MERKLE_PROOF_H
