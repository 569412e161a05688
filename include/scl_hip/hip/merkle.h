// include/scl_hip/hip/merkle.h -- Merkle commitments to device-resident share vectors: the batch form of
// scl::util::MerkleTree<Sha256, FF> (include/scl/util/merkle.h:34-181) over hip::DeviceVector (one tree of N leaves) and
// hip::ShareMatrix (one tree per secret over the n shares dealt: T = secrets, L = parties, no transpose).  Digests, trees and
// paths stay in HBM (DeviceBuffer); a proof that leaves the device is a util::MerkleProof<Digest<256>>, interchangeable with
// the ones util::MerkleTree::prove makes on the host.  Thin calls into the C ABI (scl_hip_merkle_*).
#ifndef SCL_HIP_HIP_MERKLE_H
#define SCL_HIP_HIP_MERKLE_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../util/digest.h"
#include "../util/merkle.h"
#include "device.h"

namespace scl::hip {

using MerkleDigest = util::Digest<256>;
using MerkleProof = util::MerkleProof<MerkleDigest>;

/// digests in HBM with the shape they describe: `leaves` per tree, `trees` side by side (leaf-major, tree-minor)
struct DeviceDigests {
  DeviceBuffer buf;
  std::size_t leaves = 0, trees = 0;
  unsigned char* data() const { return static_cast<unsigned char*>(buf.get()); }
};

/// all levels of a batch of trees (scl_hip_merkle_build's layout; the roots are the last `trees` digests)
struct DeviceMerkleTree {
  DeviceBuffer buf;
  std::size_t leaves = 0, trees = 0;
  unsigned char* data() const { return static_cast<unsigned char*>(buf.get()); }
  std::size_t depth() const { return scl_hip_merkle_depth(leaves); }
  const unsigned char* roots() const { return data() + buf.bytes() - trees * 32; }
  std::vector<MerkleDigest> rootsToHost() const {
    std::vector<MerkleDigest> out(trees);
    if (trees) check(scl_hip_memcpy_d2h(out.data(), roots(), trees * 32, nullptr));
    return out;
  }
};

/// leaf digests of one tree over a vector: leaf s = Sha256(Serializer<T> image of a[s])
template <typename T>
DeviceDigests merkleLeaves(const DeviceVector<T>& a, void* stream = nullptr) {
  DeviceDigests d{DeviceBuffer(a.size() * 32), a.size(), 1};
  check(scl_hip_merkle_leaves(T::Field::TAG, d.data(), a.data(), a.size(), 1, a.size(), stream));
  return d;
}
/// leaf digests of one tree per secret: leaf i of tree s = the digest of party i's share of secret s
template <typename T>
DeviceDigests merkleLeaves(const ShareMatrix<T>& m, void* stream = nullptr) {
  DeviceDigests d{DeviceBuffer(m.parties() * m.secrets() * 32), m.parties(), m.secrets()};
  check(scl_hip_merkle_leaves(T::Field::TAG, d.data(), m.data(), m.stride(), m.parties(), m.secrets(), stream));
  return d;
}

inline DeviceMerkleTree merkleTree(const DeviceDigests& leaves, void* stream = nullptr) {
  DeviceMerkleTree t{DeviceBuffer(scl_hip_merkle_tree_bytes(leaves.leaves, leaves.trees)), leaves.leaves, leaves.trees};
  check(scl_hip_merkle_build(t.data(), leaves.data(), leaves.leaves, leaves.trees, stream));
  return t;
}
template <typename C>
DeviceMerkleTree merkleTree(const C& values, void* stream = nullptr) {
  return merkleTree(merkleLeaves(values, stream), stream);
}

/// MerkleTree::hash for every tree of the batch, levels not kept
inline std::vector<MerkleDigest> merkleRoot(const DeviceDigests& leaves, void* stream = nullptr) {
  DeviceBuffer roots(leaves.trees * 32);
  check(scl_hip_merkle_root(static_cast<unsigned char*>(roots.get()), leaves.data(), leaves.leaves, leaves.trees, stream));
  std::vector<MerkleDigest> out(leaves.trees);
  if (leaves.trees) check(scl_hip_memcpy_d2h(out.data(), roots.get(), leaves.trees * 32, stream));
  check(scl_hip_stream_sync(stream));
  return out;
}
template <typename C>
std::vector<MerkleDigest> merkleRoot(const C& values, void* stream = nullptr) {
  return merkleRoot(merkleLeaves(values, stream), stream);
}

namespace detail {
inline DeviceBuffer uploadIndices(const std::vector<std::uint64_t>& idx, void* stream) {
  DeviceBuffer b(idx.size() * 8);
  if (!idx.empty()) check(scl_hip_memcpy_h2d(b.get(), idx.data(), idx.size() * 8, stream));
  return b;
}
inline std::vector<MerkleProof> proofsToHost(const DeviceBuffer& path, std::size_t depth, const std::vector<std::uint64_t>& leaf,
                                             void* stream) {
  const std::size_t k = leaf.size();
  std::vector<MerkleDigest> flat(depth * k);
  if (!flat.empty()) check(scl_hip_memcpy_d2h(flat.data(), path.get(), flat.size() * 32, stream));
  check(scl_hip_stream_sync(stream));
  std::vector<MerkleProof> out(k);
  for (std::size_t q = 0; q < k; ++q) {
    for (std::size_t l = 0; l < depth; ++l) out[q].path.push_back(flat[l * k + q]);
    out[q].direction = util::Bitmap::fromIndex(leaf[q], depth);
  }
  return out;
}
}  // namespace detail

/// MerkleTree::prove for leaves `leaf[q]` of trees `tree[q]` (tree empty: tree 0 throughout)
inline std::vector<MerkleProof> merklePaths(const DeviceMerkleTree& t, const std::vector<std::uint64_t>& leaf,
                                            const std::vector<std::uint64_t>& tree = {}, void* stream = nullptr) {
  for (std::uint64_t i : leaf)
    if (i >= t.leaves) check(SCL_ERR_INVALID_RANGE);
  const std::vector<std::uint64_t> zeros(tree.empty() ? leaf.size() : 0, 0);
  const DeviceBuffer li = detail::uploadIndices(leaf, stream), ti = detail::uploadIndices(tree.empty() ? zeros : tree, stream);
  const DeviceBuffer path(t.depth() * leaf.size() * 32);
  check(scl_hip_merkle_paths(static_cast<unsigned char*>(path.get()), t.data(), t.leaves, t.trees, static_cast<const std::uint64_t*>(li.get()),
                             static_cast<const std::uint64_t*>(ti.get()), 0, leaf.size(), stream));
  return detail::proofsToHost(path, t.depth(), leaf, stream);
}
/// party p's proof in every tree of the batch (one per secret)
inline std::vector<MerkleProof> merklePathsOfParty(const DeviceMerkleTree& t, std::size_t party, void* stream = nullptr) {
  const DeviceBuffer path(t.depth() * t.trees * 32);
  check(scl_hip_merkle_paths(static_cast<unsigned char*>(path.get()), t.data(), t.leaves, t.trees, nullptr, nullptr, party, t.trees, stream));
  return detail::proofsToHost(path, t.depth(), std::vector<std::uint64_t>(t.trees, party), stream);
}

/// MerkleTree::verify for leaves[q] against roots[q] with proofs[q] (all of one depth); one flag per query
template <typename T>
std::vector<bool> merkleVerify(const std::vector<T>& leaves, const std::vector<MerkleDigest>& roots, const std::vector<MerkleProof>& proofs,
                               void* stream = nullptr) {
  const std::size_t k = leaves.size(), depth = proofs.empty() ? 0 : proofs[0].path.size();
  if (proofs.size() != k || roots.size() != k) check(SCL_ERR_SIZE_MISMATCH);
  std::vector<MerkleDigest> flat(depth * k);
  std::vector<std::uint64_t> index(k, 0);
  for (std::size_t q = 0; q < k; ++q) {
    if (proofs[q].path.size() != depth) check(SCL_ERR_SIZE_MISMATCH);
    for (std::size_t l = 0; l < depth; ++l) {
      flat[l * k + q] = proofs[q].path[l];
      if (l < 64 && proofs[q].direction.at(l)) index[q] |= std::uint64_t(1) << l;
    }
  }
  const DeviceVector<T> dleaves(leaves);
  const DeviceDigests digests = merkleLeaves(dleaves, stream);
  const DeviceBuffer dpath(flat.size() * 32), droots(k * 32), dok(k), dindex = detail::uploadIndices(index, stream);
  if (!flat.empty()) check(scl_hip_memcpy_h2d(dpath.get(), flat.data(), flat.size() * 32, stream));
  if (k) check(scl_hip_memcpy_h2d(droots.get(), roots.data(), k * 32, stream));
  check(scl_hip_merkle_verify(static_cast<unsigned char*>(dok.get()), digests.data(), static_cast<const std::uint64_t*>(dindex.get()), 0,
                              static_cast<const unsigned char*>(dpath.get()), depth, static_cast<const unsigned char*>(droots.get()),
                              nullptr, k, k, stream));
  std::vector<unsigned char> ok(k);
  if (k) check(scl_hip_memcpy_d2h(ok.data(), dok.get(), k, stream));
  check(scl_hip_stream_sync(stream));
  return std::vector<bool>(ok.begin(), ok.end());
}

}  // namespace scl::hip

#endif  // SCL_HIP_HIP_MERKLE_H
