// include/scl_hip/util/merkle.h -- scl::util::MerkleTree<HASH, LEAF> (include/scl/util/merkle.h:34-181) on the host, per
// call, as the reference runs it, and with the reference's tree -- not the textbook one: the leaf level is padded to an even
// count by repeating its last digest (a single leaf hashes with itself) and so is every later level of odd size greater
// than one.  Repeating a node is reading it twice, so a level keeps its real count here and the right child's index is
// clamped -- the formulation of the device kernels (csrc/hash_unit.hip), which produce the same digests and the same proofs
// for batches: hip::merkleTree / merklePaths / merkleVerify (hip/merkle.h).
#ifndef SCL_HIP_UTIL_MERKLE_H
#define SCL_HIP_UTIL_MERKLE_H

#include <cstddef>
#include <stdexcept>
#include <vector>

#include "merkle_proof.h"

namespace scl::util {

/// hashing levels over L leaves: max(1, ceil(log2 L)); 0 for no leaves (scl_hip_merkle_depth)
inline std::size_t merkleDepth(std::size_t leaves) {
  if (leaves == 0) return 0;
  std::size_t depth = 1;
  for (std::size_t r = (leaves + 1) / 2; r > 1; r = (r + 1) / 2) ++depth;
  return depth;
}

template <typename HASH, typename LEAF>
struct MerkleTree {
  using DigestType = typename HASH::DigestType;
  using Proof = MerkleProof<DigestType>;

  static DigestType hash(const std::vector<LEAF>& data) { return reduce(data, 0, nullptr); }

  static Proof prove(const std::vector<LEAF>& data, std::size_t index) {
    Proof proof;
    reduce(data, index, &proof.path);
    proof.direction = Bitmap::fromIndex(index, proof.path.size());
    return proof;
  }

  static bool verify(const LEAF& leaf, const DigestType& root, const Proof& proof) {
    DigestType digest = HASH{}.update(leaf).finalize();
    for (std::size_t level = 0; level < proof.path.size(); ++level) {
      const DigestType& sibling = proof.path[level];
      digest = proof.direction.at(level) ? HASH{}.update(sibling).update(digest).finalize()
                                         : HASH{}.update(digest).update(sibling).finalize();
    }
    return digest == root;
  }

 private:
  // the root; with `path`, also the sibling of `index`'s ancestor at every level
  static DigestType reduce(const std::vector<LEAF>& data, std::size_t index, std::vector<DigestType>* path) {
    if (data.empty()) throw std::invalid_argument("MerkleTree: no leaves");  // (the reference reads digests[0] of an empty vector)
    if (path && index >= data.size()) throw std::invalid_argument("MerkleTree: leaf index out of range");
    std::vector<DigestType> level;
    level.reserve(data.size());
    for (const LEAF& leaf : data) level.push_back(HASH{}.update(leaf).finalize());
    do {
      const std::size_t count = level.size(), half = (count + 1) / 2;
      if (path) {
        const std::size_t sibling = (index ^ 1) < count ? (index ^ 1) : index;
        path->push_back(level[sibling]);
        index >>= 1;
      }
      for (std::size_t j = 0; j < half; ++j) {
        const std::size_t right = 2 * j + 1 < count ? 2 * j + 1 : count - 1;
        level[j] = HASH{}.update(level[2 * j]).update(level[right]).finalize();
      }
      level.resize(half);
    } while (level.size() > 1);
    return level[0];
  }
};

}  // namespace scl::util

#endif  // SCL_HIP_UTIL_MERKLE_H
