#!/usr/bin/env python3
"""Generate tests/golden/golden_merkle.json from the REAL reference's MerkleTree<Sha256, FF<F>>.

The reference's tree (include/scl/util/merkle.h:74-162) is not the textbook one -- the leaf level is padded to even by
repeating its last digest, one leaf included, and so is every later level of odd size greater than one -- and hashlib cannot
say so.  This script writes a small harness of its own against the reference's headers (MerkleTree, Sha256, Vector::random,
the FF serializer), compiles it with the translation units the oracle's `make ref` uses plus src/scl/util/sha256.cc into a
temporary directory OUTSIDE the repository, runs it and keeps what it prints: per field and leaf count the leaves' wire bytes,
the root and one proof (path + Bitmap bytes + the Serializer image of the proof).  Nothing compiled is kept.  Run in the build
container only:

    python tests/golden/make_golden_merkle.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCL_REFERENCE", "/root/reference")
GMP_SO = os.environ.get("GMP_SO", "/usr/lib/x86_64-linux-gnu/libgmp.so.10")
SIZES = [1, 2, 3, 5, 8, 33]
TUS = ["src/scl/math/fields/mersenne61.cc", "src/scl/math/fields/mersenne127.cc", "src/scl/util/prg.cc", "src/scl/util/str.cc",
       "src/scl/math/fields/secp256k1_scalar.cc", "src/scl/math/fields/secp256k1_field.cc", "src/scl/math/fields/ff_ops_gmp.cc",
       "src/scl/math/number.cc", "src/scl/util/sha256.cc"]

HARNESS = r"""
#include <cstdio>
#include <string>
#include <vector>

#include "scl/math/fields/mersenne127.h"
#include "scl/math/fields/mersenne61.h"
#include "scl/math/fields/secp256k1_field.h"
#include "scl/math/fields/secp256k1_scalar.h"
#include "scl/math/ff.h"
#include "scl/math/vector.h"
#include "scl/serialization/serializer.h"
#include "scl/util/merkle.h"
#include "scl/util/prg.h"
#include "scl/util/sha256.h"

using namespace scl;

static void hex(const unsigned char* p, std::size_t n) {
  for (std::size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
}

template <typename F>
static void field(const char* name, const char* code, const std::vector<std::size_t>& sizes, bool last) {
  using E = math::FF<F>;
  using Tree = util::MerkleTree<util::Sha256, E>;
  std::printf("\"%s\":[", name);
  for (std::size_t k = 0; k < sizes.size(); ++k) {
    const std::size_t L = sizes[k], index = 2 * L / 3;
    // PRG::create keeps 16 bytes of a seed (prg.cc:88-101): what tells the trees apart comes first
    const std::string seed = std::to_string(L) + "-" + code + "-merkle";
    auto prg = util::PRG::create(seed);
    const std::vector<E> leaves = math::Vector<E>::random(L, prg).toStlVector();
    std::printf("{\"L\":%zu,\"seed\":\"%s\",\"leaves\":\"", L, seed.c_str());
    for (const E& e : leaves) {
      unsigned char buf[64];
      const std::size_t n = seri::Serializer<E>::write(e, buf);
      hex(buf, n);
    }
    const auto root = Tree::hash(leaves);
    std::printf("\",\"root\":\"");
    hex(root.data(), root.size());
    const auto proof = Tree::prove(leaves, index);
    std::printf("\",\"index\":%zu,\"path\":[", index);
    for (std::size_t i = 0; i < proof.path.size(); ++i) {
      std::printf("%s\"", i ? "," : "");
      hex(proof.path[i].data(), proof.path[i].size());
      std::printf("\"");
    }
    std::vector<unsigned char> image(seri::Serializer<typename Tree::Proof>::sizeOf(proof));
    seri::Serializer<typename Tree::Proof>::write(proof, image.data());
    std::printf("],\"proof_image\":\"");
    hex(image.data(), image.size());
    std::printf("\",\"verifies\":%s}%s", Tree::verify(leaves[index], root, proof) ? "true" : "false", k + 1 < sizes.size() ? "," : "");
  }
  std::printf("]%s", last ? "" : ",");
}

int main(int argc, char** argv) {
  std::vector<std::size_t> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back(std::stoul(argv[i]));
  std::printf("{");
  field<math::ff::Mersenne61>("Mersenne61", "m61", sizes, false);
  field<math::ff::Mersenne127>("Mersenne127", "m127", sizes, false);
  field<math::ff::Secp256k1Scalar>("Secp256k1Scalar", "k1s", sizes, false);
  field<math::ff::Secp256k1Field>("Secp256k1Field", "k1f", sizes, true);
  std::printf("}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_merkle_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", "-idirafter", "/opt/conda/include",
                        "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe] + [str(s) for s in SIZES], check=True, capture_output=True, text=True).stdout
    doc = {"generator": "tests/golden/make_golden_merkle.py",
           "source": "the reference's util::MerkleTree<util::Sha256, math::FF<F>> (include/scl/util/merkle.h, src/scl/util/sha256.cc) "
                     "over math::Vector<FF<F>>::random(L, PRG::create(seed)); leaves = the concatenated Serializer<FF> images; "
                     "proof_image = Serializer<MerkleProof> of prove(leaves, index)",
           "fields": json.loads(out)}
    for cases in doc["fields"].values():
        assert all(c["verifies"] for c in cases)
    path = os.path.join(HERE, "golden_merkle.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
