#!/usr/bin/env python3
"""Generate tests/golden/golden_rb.json from the REAL reference: square roots over the secp256k1 prime field by its
math::details::sqrt (src/scl/math/fields/secp256k1_field.cc:142-157, the root point decompression takes).

This script writes a small harness of its own against the reference's headers, compiles it with the reference's field and PRG
translation units into a temporary directory OUTSIDE the repository, runs it and keeps what it prints.  Elements are their
FF::write images (byteSize bytes, in hex).  Nothing compiled is kept.  Run in the build container only:

    python tests/golden/make_golden_rb.py

Contents: x = Vector::random(16) off the PRG "rb squares" over Secp256k1Field; y = x^2 element by element, then 0 and 1: 18
squares.  Recorded: y and details::sqrt(y).  The reference returns whichever root y^((p+1)/4) is -- even or odd; the harness
requires root^2 == y and nothing else.  The test that reads the fixture normalises to the even root before it compares.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SCL_REFERENCE", "/root/reference")
GMP_SO = os.environ.get("GMP_SO", "/usr/lib/x86_64-linux-gnu/libgmp.so.10")
TUS = ["src/scl/util/prg.cc", "src/scl/util/str.cc", "src/scl/math/fields/secp256k1_field.cc", "src/scl/math/fields/ff_ops_gmp.cc",
       "src/scl/math/number.cc"]

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <string>

#include "scl/math/curves/secp256k1.h"
#include "scl/math/ff.h"
#include "scl/math/vector.h"
#include "scl/util/prg.h"
#include "secp256k1_helpers.h"

using namespace scl;
using Field = math::FF<math::ff::Secp256k1Field>;

static std::string image(const Field& v) {  // the FF::write image, in hex
  unsigned char buf[64];
  v.write(buf);
  std::string s;
  char h[3];
  for (std::size_t i = 0; i < Field::byteSize(); ++i) {
    std::snprintf(h, sizeof h, "%02x", buf[i]);
    s += h;
  }
  return s;
}

int main() {
  const unsigned char seed[] = "rb squares";
  auto prg = util::PRG::create(seed, sizeof seed - 1);
  const auto x = math::Vector<Field>::random(16, prg);
  std::printf("{\"field\":\"secp256k1_field\",\"cases\":[");
  for (std::size_t i = 0; i < 18; ++i) {
    const Field y = i < 16 ? x[i] * x[i] : Field((int)(i - 16));
    const Field r = math::details::sqrt(y);
    if (!(r * r == y)) {
      std::fprintf(stderr, "harness: the reference's root does not square to y\n");
      return 1;
    }
    std::printf("%s\n{\"y\":\"%s\",\"root\":\"%s\"}", i ? "," : "", image(y).c_str(), image(r).c_str());
  }
  std::printf("]}\n");
  return 0;
}
"""


def main():
    if not os.path.isdir(os.path.join(REF, "include", "scl")):
        sys.exit(f"the reference is not at {REF}: this generator runs in the build container only")
    with tempfile.TemporaryDirectory(prefix="golden_rb_") as tmp:
        src, exe = os.path.join(tmp, "harness.cc"), os.path.join(tmp, "harness")
        with open(src, "w") as fh:
            fh.write(HARNESS)
        subprocess.run(["g++", "-std=c++20", "-O2", "-march=x86-64-v3", "-maes", f"-I{REF}/include", f"-I{REF}/src/scl/math/fields",
                        "-idirafter", "/opt/conda/include", "-o", exe, src] + [os.path.join(REF, t) for t in TUS] + [GMP_SO], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    d = json.loads(out)
    assert d["field"] == "secp256k1_field" and len(d["cases"]) == 18 and all(len(c["y"]) == len(c["root"]) == 64 for c in d["cases"])
    assert int(d["cases"][16]["y"], 16) == 0 and int(d["cases"][17]["y"], 16) == 1
    head = {"generator": "tests/golden/make_golden_rb.py",
            "source": "the reference's math::details::sqrt over Secp256k1Field on squares of Vector::random off the PRG 'rb squares', "
                      "then 0 and 1; elements are FF::write images (byteSize bytes, in hex); the root is whichever y^((p+1)/4) is"}
    path = os.path.join(HERE, "golden_rb.json")
    with open(path, "w") as fh:       # the harness's own line structure: one case per line
        fh.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"data":' + out.strip() + "}\n")
    with open(path) as fh:
        assert json.load(fh)["data"] == d
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
