// tests/cxx/test_merkle_api.cc -- the commitment half of the C++ mirror: util::Sha256, util::Bitmap, util::MerkleProof and
// util::MerkleTree (include/scl_hip/util/) on the host, and with --device the hip:: batch calls against them.
//
//   test_merkle_api <cases-file> [--device]
// The cases file is written by the Python test that drives this binary (tests/test_merkle_host.py); one case per line:
//   sha <message hex | -> <split> <digest hex>          Sha256 of the message, absorbed as [0, split) then [split, end);
//                                                        the digest comes from hashlib
//   tree <field> <L> <leaves hex> <root hex> <index> <proof image hex>
//                                                        a tree the REFERENCE hashed (tests/golden/golden_merkle.json)
// Besides those it restates the three cases of the reference's test/scl/util/test_merkle.cc:42-123 with Sha256 where the
// reference has Hash<256>.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <string_view>
#include <vector>

#include "scl_hip/scl.h"

#include "check.hpp"

using namespace scl;

using Digest = util::Digest<256>;
using StrTree = util::MerkleTree<util::Sha256, std::string_view>;

static Digest digestOf(const std::string& hex) {
  Digest d{};
  const auto b = unhex(hex);
  if (b.size() == d.size()) std::memcpy(d.data(), b.data(), d.size());
  return d;
}
static Digest H(std::string_view s) { return util::Sha256{}.update(s).finalize(); }
static Digest H(const Digest& l, const Digest& r) { return util::Sha256{}.update(l).update(r).finalize(); }

static void reference_cases() {
  // "Merkle hash": four and eight leaves
  const Digest abcd = H(H(H("a"), H("b")), H(H("c"), H("d")));
  REQUIRE(StrTree::hash({"a", "b", "c", "d"}) == abcd);
  const Digest xyvu = H(H(H("x"), H("y")), H(H("v"), H("u")));
  REQUIRE(StrTree::hash({"a", "b", "c", "d", "x", "y", "v", "u"}) == H(abcd, xyvu));
  // "Merkle hash odd size input": three leaves, the last one repeated
  REQUIRE(StrTree::hash({"a", "b", "c"}) == H(H(H("a"), H("b")), H(H("c"), H("c"))));
  // "Merkle proof": five leaves, index 3
  const std::vector<std::string_view> five = {"a", "b", "c", "d", "e"};
  const Digest ab = H(H("a"), H("b")), cd = H(H("c"), H("d")), ee = H(H("e"), H("e"));
  const Digest root = H(H(ab, cd), H(ee, ee));
  REQUIRE(StrTree::hash(five) == root);
  const auto proof = StrTree::prove(five, 3);
  REQUIRE(proof.path.size() == 3);
  REQUIRE(proof.path.size() == 3 && proof.path[0] == H("c") && proof.path[1] == ab && proof.path[2] == H(ee, ee));
  REQUIRE(proof.direction == util::Bitmap::fromStdVecBool({true, true, false}));
  REQUIRE(StrTree::verify("d", root, proof));
  REQUIRE(!StrTree::verify("c", root, proof));
  using Sr = seri::Serializer<StrTree::Proof>;
  REQUIRE(Sr::sizeOf(proof) == 2 * 4 + 3 * 32 + 1);
  std::vector<unsigned char> image(Sr::sizeOf(proof));
  REQUIRE(Sr::write(proof, image.data()) == image.size());
  StrTree::Proof back;
  REQUIRE(Sr::read(back, image.data()) == image.size());
  REQUIRE(back.path == proof.path && back.direction == proof.direction);
  REQUIRE(StrTree::verify("d", root, back));
  // one leaf hashes with itself; every index of a tree proves; the directions are the index's bits
  REQUIRE(StrTree::hash({"a"}) == H(H("a"), H("a")));
  for (std::size_t i = 0; i < five.size(); ++i) {
    const auto p = StrTree::prove(five, i);
    REQUIRE(StrTree::verify(five[i], root, p));
    REQUIRE(p.direction == util::Bitmap::fromIndex(i, 3));
  }
  // Bitmap
  util::Bitmap bm(10);
  bm.set(9, true);
  bm.set(0, true);
  REQUIRE(bm.numberOfBlocks() == 2 && bm.count() == 2 && bm.at(9) && !bm.at(8));
  REQUIRE((bm ^ bm).count() == 0 && (bm | ~bm).count() == 16 && (bm & bm) == bm);
  REQUIRE(util::Bitmap().numberOfBlocks() == 1);
  REQUIRE(util::digestToString(H("abc")).substr(0, 8) == "ba7816bf");
}

static void sha_case(const std::string& msg_hex, std::size_t split, const std::string& want) {
  const auto msg = unhex(msg_hex);
  util::Sha256 h;
  h.update(msg.data(), split).update(msg.data() + split, msg.size() - split);
  REQUIRE(h.finalize() == digestOf(want));
  REQUIRE(util::Sha256{}.update(msg).finalize() == digestOf(want));
}

template <typename F>
static void tree_case(std::size_t L, const std::string& leaves_hex, const std::string& root_hex, std::size_t index,
                      const std::string& image_hex, bool device) {
  using E = math::FF<F>;
  using Tree = util::MerkleTree<util::Sha256, E>;
  const auto bytes = unhex(leaves_hex);
  REQUIRE(bytes.size() == L * E::byteSize());
  std::vector<E> leaves;
  for (std::size_t i = 0; i < L; ++i) leaves.push_back(E::read(bytes.data() + i * E::byteSize()));
  const Digest root = digestOf(root_hex);
  REQUIRE(Tree::hash(leaves) == root);
  const auto proof = Tree::prove(leaves, index);
  const auto image = unhex(image_hex);
  using Sr = seri::Serializer<typename Tree::Proof>;
  std::vector<unsigned char> mine(Sr::sizeOf(proof));
  Sr::write(proof, mine.data());
  REQUIRE(mine == image);
  typename Tree::Proof theirs;
  REQUIRE(Sr::read(theirs, image.data()) == image.size());
  REQUIRE(Tree::verify(leaves[index], root, theirs));
  REQUIRE(util::merkleDepth(L) == proof.path.size());
  REQUIRE(scl_hip_merkle_depth(L) == proof.path.size());
  if (!device) return;
  // the device's tree and proofs against the host's, both ways, for every leaf
  const hip::DeviceVector<E> dv(leaves);
  const hip::DeviceMerkleTree tree = hip::merkleTree(dv);
  REQUIRE(tree.rootsToHost().at(0) == root);
  REQUIRE(hip::merkleRoot(dv).at(0) == root);
  std::vector<std::uint64_t> all(L);
  for (std::size_t i = 0; i < L; ++i) all[i] = i;
  const std::vector<hip::MerkleProof> dproofs = hip::merklePaths(tree, all);
  std::vector<hip::MerkleProof> hproofs;
  for (std::size_t i = 0; i < L; ++i) {
    hproofs.push_back(Tree::prove(leaves, i));
    REQUIRE(dproofs[i].path == hproofs[i].path && dproofs[i].direction == hproofs[i].direction);
    REQUIRE(Tree::verify(leaves[i], root, dproofs[i]));  // a device-built proof under the host's verify
  }
  const std::vector<Digest> roots(L, root);
  const std::vector<bool> ok = hip::merkleVerify(leaves, roots, hproofs);  // host-built proofs under the device's verify
  for (std::size_t i = 0; i < L; ++i) REQUIRE(ok[i]);
  if (L > 1) {  // and a proof that belongs to another leaf fails on both sides
    std::vector<E> shifted(leaves.begin() + 1, leaves.end());
    shifted.push_back(leaves[0] + E::one());
    const std::vector<bool> bad = hip::merkleVerify(shifted, roots, hproofs);
    for (std::size_t i = 0; i < L; ++i) REQUIRE(bad[i] == Tree::verify(shifted[i], root, hproofs[i]));
    REQUIRE(!bad[L - 1]);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_merkle_api <cases-file> [--device]\n");
    return 2;
  }
  const bool device = argc > 2 && std::string(argv[2]) == "--device";
  reference_cases();
  std::ifstream in(argv[1]);
  std::string line;
  int sha = 0, trees = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string kind;
    ls >> kind;
    if (kind == "sha") {
      std::string msg, want;
      std::size_t split;
      ls >> msg >> split >> want;
      sha_case(msg, split, want);
      ++sha;
    } else if (kind == "tree") {
      std::string field, leaves, root, image;
      std::size_t L, index;
      ls >> field >> L >> leaves >> root >> index >> image;
      if (field == "Mersenne61") tree_case<math::ff::Mersenne61>(L, leaves, root, index, image, device);
      else if (field == "Mersenne127") tree_case<math::ff::Mersenne127>(L, leaves, root, index, image, device);
      else if (field == "Secp256k1Scalar") tree_case<math::ff::Secp256k1Scalar>(L, leaves, root, index, image, device);
      else if (field == "Secp256k1Field") tree_case<math::ff::Secp256k1Field>(L, leaves, root, index, image, device);
      else REQUIRE(!"unknown field in the cases file");
      ++trees;
    }
  }
  std::printf("merkle api%s: %d sha cases, %d trees, %d checks, %d failures\n", device ? " (device)" : "", sha, trees, g_checks, g_fail);
  return g_fail ? 1 : 0;
}
