"""Merkle commitments, the host half: the C++ mirror's util::Sha256 / Bitmap / MerkleProof / MerkleTree
(tests/cxx/test_merkle_api.cc) against hashlib and against trees the REFERENCE hashed (tests/golden/golden_merkle.json), the
Python model of the reference's tree shape (tests/merkle_model.py) that checks the kernels in tests/test_gpu_merkle.py, and the new corner of the ABI."""
import ctypes as C
import os
import subprocess
import sys

from cxx_support import ROOT, mirror_binary
from merkle_model import ELEMENT_BYTES, golden, golden_leaves, model_levels, model_path, model_tree_bytes, model_verify, sha, write_cases


def test_model_reproduces_the_reference_trees():
    """roots, paths and the proofs' wire images of MerkleTree<Sha256, FF<F>> as the reference computed them, L in
    {1, 2, 3, 5, 8, 33} over four fields: the padding rules and the one-leaf tree, which hashlib alone cannot pin"""
    fields = golden()
    assert set(fields) == set(ELEMENT_BYTES)
    for field, cases in fields.items():
        assert [c["L"] for c in cases] == [1, 2, 3, 5, 8, 33]
        for c in cases:
            digests = [sha(x) for x in golden_leaves(field, c)]
            levels = model_levels(digests)
            assert levels[-1][0].hex() == c["root"], (field, c["L"])
            path = model_path(levels, c["index"])
            assert [p.hex() for p in path] == c["path"], (field, c["L"])
            depth = len(path)
            assert depth == max(1, (c["L"] - 1).bit_length())
            # Serializer<MerkleProof>: u32 count, digests, u32 bitmap bytes, the index's low `depth` bits little-endian
            nbytes = max(1, (depth + 7) // 8)
            image = depth.to_bytes(4, "little") + b"".join(path) + nbytes.to_bytes(4, "little") + \
                (c["index"] & ((1 << depth) - 1)).to_bytes(nbytes, "little")
            assert image.hex() == c["proof_image"], (field, c["L"])
            assert model_verify(digests[c["index"]], c["index"], path, levels[-1][0])
            assert model_tree_bytes(digests, c["L"], 1) == b"".join(b"".join(lv) for lv in levels)


def test_cxx_mirror_hashes_and_proves_like_hashlib_and_the_reference(tmp_path):
    """util::Sha256 (empty, "abc", the 55 / 56 / 64-byte boundaries, split updates), the three cases of the reference's
    test_merkle.cc with Sha256, and every fixture tree through MerkleTree::hash / prove / verify and the proof's Serializer"""
    cases = str(tmp_path / "cases.txt")
    n = write_cases(cases)
    r = subprocess.run([mirror_binary("merkle"), cases], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n - 24} sha cases, 24 trees" in r.stdout and " 0 failures" in r.stdout, r.stdout


def test_shape_helpers_of_the_abi_agree_with_the_model():
    """scl_hip_merkle_depth / _level_size / _tree_bytes: the one description of the tree's shape the ABI, the mirror and the
    tests share"""
    import scl_amd as scl
    for L in list(range(1, 70)) + [1000, 1001, 100003, 2 ** 20 + 1, 2 ** 22 + 3]:
        sizes, n = [L], L
        while True:
            n = (n + 1) // 2
            sizes.append(n)
            if n == 1:
                break
        if L < 70:
            assert sizes == [len(lv) for lv in model_levels([bytes(32)] * L)]
        assert scl.merkle_depth(L) == len(sizes) - 1
        assert [scl.merkle_level_size(L, l) for l in range(len(sizes) + 2)] == sizes + [0, 0]
        for T in (1, 3, 100003):
            assert scl.merkle_tree_bytes(L, T) == 32 * T * sum(sizes)
    assert scl.merkle_depth(0) == 0 and scl.merkle_tree_bytes(0, 5) == 0 and scl.merkle_level_size(0, 0) == 0


def test_bad_shapes_are_refused_before_anything_is_launched():
    """L = 0 (the reference reads digests[0] of an empty vector), T = 0, a host leaf index >= L, a ring tag"""
    import scl_amd as scl
    buf = (C.c_ubyte * 4096)()
    p = C.c_void_p((C.addressof(buf) + 63) & ~63)
    for L, T in ((0, 1), (1, 0)):
        assert scl.lib.scl_hip_merkle_build(p, p, L, T, None) == scl.ERR_BAD_ARG
        assert scl.lib.scl_hip_merkle_root(p, p, L, T, None) == scl.ERR_BAD_ARG
        assert scl.lib.scl_hip_merkle_paths(p, p, L, T, None, None, 0, 1, None) == scl.ERR_BAD_ARG
    assert scl.lib.scl_hip_merkle_paths(p, p, 5, 1, None, None, 5, 1, None) == scl.ERR_INVALID_RANGE
    assert scl.lib.scl_hip_merkle_paths(p, p, 5, 1, None, None, 3, 3, None) == scl.ERR_INVALID_RANGE
    assert scl.lib.scl_hip_merkle_paths(p, p, 5, 4, None, None, 4, 5, None) == scl.ERR_INVALID_RANGE
    assert scl.lib.scl_hip_merkle_verify(p, p, None, 8, p, 3, p, None, 1, 1, None) == scl.ERR_INVALID_RANGE
    assert scl.lib.scl_hip_merkle_leaves(scl.Z2K(64), p, p, 4, 1, 4, None) == scl.ERR_BAD_ARG
    assert scl.lib.scl_hip_merkle_leaves(scl.M61, C.c_void_p(p.value + 8), p, 4, 1, 4, None) == scl.ERR_BAD_ARG


def test_generated_abi_files_are_current_and_export_the_new_entry_points():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_capi_route.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    exports = open(os.path.join(ROOT, "secure-computation-library_amd", "csrc", "exports.map")).read()
    route = open(os.path.join(ROOT, "secure-computation-library_amd", "csrc", "capi_route.cc")).read()
    for name in ("sha256", "merkle_leaves", "merkle_depth", "merkle_level_size", "merkle_tree_bytes", "merkle_build", "merkle_root",
                 "merkle_paths", "merkle_verify"):
        assert f"scl_hip_{name};" in exports
    assert "scl_hip_merkle_leaves__m61" in route and "scl_hip_merkle_build__" not in route   # only the leaf kernel is per family
    import scl_amd as scl
    assert scl.lib.scl_hip_abi_version() == 2
