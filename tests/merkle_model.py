"""The Python model of the reference's Merkle tree (include/scl/util/merkle.h:74-162 of the reference) over hashlib, the reader
of tests/golden/golden_merkle.json -- trees the REFERENCE hashed -- and the cases file it becomes for tests/cxx/test_merkle_api.cc.
tests/test_merkle_host.py pins the model to the fixture; tests/test_gpu_merkle.py and the red-zone tests compare the kernels
against it.  Standard library only.

A level keeps its real node count; "repeat the last digest" (the leaf level when odd -- one leaf included -- and every later level
of odd size greater than one) is the right child's index clamped to the last node."""
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_merkle.json")
ELEMENT_BYTES = {"Mersenne61": 8, "Mersenne127": 16, "Secp256k1Scalar": 32, "Secp256k1Field": 32}
SHA_LENGTHS = [0, 3, 55, 56, 63, 64, 65, 119, 120, 300]


def sha(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def model_levels(leaf_digests):
    """[level 0 = the leaf digests, level 1, .., [root]]"""
    levels = [list(leaf_digests)]
    while True:
        cur = levels[-1]
        levels.append([sha(cur[2 * j] + cur[min(2 * j + 1, len(cur) - 1)]) for j in range((len(cur) + 1) // 2)])
        if len(levels[-1]) == 1:
            return levels


def model_path(levels, index):
    """the sibling at every level below the root; direction[l] = bit l of the index"""
    return [lv[min((index >> l) ^ 1, len(lv) - 1)] for l, lv in enumerate(levels[:-1])]


def model_verify(leaf_digest, index, path, root):
    d = leaf_digest
    for l, s in enumerate(path):
        d = sha(s + d) if (index >> l) & 1 else sha(d + s)
    return d == root


def model_tree_bytes(leaf_digests, L, T):
    """scl_hip_merkle_build's buffer for T trees of L leaves, leaf digests laid out [leaf][tree]"""
    per_tree = [model_levels([leaf_digests[j * T + t] for j in range(L)]) for t in range(T)]
    return b"".join(per_tree[t][l][j] for l in range(len(per_tree[0])) for j in range(len(per_tree[0][l])) for t in range(T))


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["fields"]


def golden_leaves(field, case):
    raw, nb = bytes.fromhex(case["leaves"]), ELEMENT_BYTES[field]
    assert len(raw) == case["L"] * nb, (field, len(raw), case["L"], nb)
    return [raw[i * nb:(i + 1) * nb] for i in range(case["L"])]


def write_cases(path, sizes=None):
    """the cases file of test_merkle_api: hashlib digests and the reference's trees"""
    lines = []
    for n in SHA_LENGTHS:
        msg = bytes((7 * i + n) & 0xFF for i in range(n))
        for split in sorted({0, n // 3, n}):
            lines.append(f"sha {msg.hex() or '-'} {split} {sha(msg).hex()}")
    lines.append(f"sha {b'abc'.hex()} 1 {sha(b'abc').hex()}")
    for field, cases in golden().items():
        for c in cases:
            if sizes is None or c["L"] in sizes:
                lines.append(f"tree {field} {c['L']} {c['leaves']} {c['root']} {c['index']} {c['proof_image']}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return len(lines)
