"""Merkle commitments on the GPU: scl_hip_sha256 and scl_hip_merkle_* (csrc/sha256.hpp, hash_unit.hip) against hashlib and the
Python model of the reference's tree (tests/merkle_model.py, pinned to trees the reference hashed by tests/test_merkle_host.py) -- never
against the library.  Leaf digests of the large trees are random 32-byte strings: the kernels above the leaf level see digests
only."""
import subprocess

import numpy as np
import pytest
import torch

from cxx_support import mirror_binary
from merkle_model import golden, golden_leaves, model_levels, model_path, model_tree_bytes, sha, write_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scl():
    import scl_amd
    assert torch.cuda.is_available()
    return scl_amd


def dev_bytes(b) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def host_bytes(t: torch.Tensor) -> bytes:
    return t.detach().cpu().numpy().tobytes()


def random_digests(count, seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    return raw, [raw[i].tobytes() for i in range(count)]


def test_batched_sha256_equals_hashlib(scl):
    """every length around the one- and two-block padding boundaries and one of many blocks, small and large batches, every
    row of every batch; a dense stride, a larger aligned one (the word loads) and a larger odd one (the byte loads)"""
    rng = np.random.default_rng(256)
    for count in (1, 63, 100003):
        for n in (0, 1, 8, 31, 32, 55, 56, 63, 64, 65, 119, 120, 1000):
            for stride in sorted({max(n, 1), n + 4 + (-n) % 4, n + 3}):
                msgs = rng.integers(0, 256, size=(count, stride), dtype=np.uint8)
                got = scl.sha256(torch.from_numpy(msgs).cuda(), n).cpu().numpy().tobytes()
                rows = msgs[:, :n].tobytes()
                want = b"".join(sha(rows[i * n:(i + 1) * n]) for i in range(count))
                if got != want:
                    bad = [i for i in range(count) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
                    raise AssertionError(f"count {count} length {n} stride {stride}: {len(bad)} rows differ, first {bad[:8]}")


def test_leaf_digests_hash_the_wire_image_of_every_field(scl):
    """digest = SHA-256 of the element bytes scl_hip_wire_pack writes behind its count word (pinned to the reference's Packet
    goldens elsewhere), 0, 1 and p - 1 included, as one tree and as a share matrix window with a row pitch; rings refused"""
    import oracle_lib as O
    port = O.Port()
    for f in (scl.M61, scl.M127, scl.MONT128, scl.GF2_128, scl.SECP256K1_SCALAR, scl.SECP256K1_FIELD):
        nb, N = 8 * scl.limbs(f), 1031
        a = scl.vector_random(f, N, b"merkle-leaves")
        one = scl.to_device(np.asarray(port.from_int(f, 1)).reshape(1, -1))
        a[0].zero_()
        a[1].copy_(one[0])
        a[2:3].copy_(scl.ew(f, scl.NEG, one))           # p - 1 (GF(2^128): 1 again)
        image = host_bytes(scl.wire_pack(f, a))[4:]
        want = [sha(image[i * nb:(i + 1) * nb]) for i in range(N)]
        got = scl.merkle_leaves(f, a).cpu().numpy()
        assert [got[i].tobytes() for i in range(N)] == want, f
        # a [4][200] window of a [4][257] matrix: digest (row, col) at row * cols + col
        wide = a[:4 * 257].reshape(4, 257, -1)
        win = scl.merkle_leaves(f, wide[:, :200]).cpu().numpy()
        assert win.shape == (4, 200, 32)
        assert all(win[r, c].tobytes() == want[r * 257 + c] for r in range(4) for c in range(200)), f
    for K in (1, 64, 128):
        z = torch.zeros(8, 2 if K > 64 else 1, dtype=torch.int64, device="cuda")
        with pytest.raises(scl.SclError) as e:
            scl.merkle_leaves(scl.Z2K(K), z)
        assert e.value.status == scl.ERR_BAD_ARG


@pytest.mark.parametrize("L,T", [(L, 1) for L in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1000, 1001, 100003, 2 ** 20 + 1)] +
                         [(10, 100003), (40, 5000), (128, 2000), (3, 1)])
def test_every_node_of_a_built_tree_equals_the_model(scl, L, T):
    raw, digests = random_digests(L * T, 1000 * L + T)
    leaves = torch.from_numpy(raw.reshape((L, T, 32) if T > 1 else (L, 32))).cuda()
    tree = scl.merkle_build(leaves)
    want = model_tree_bytes(digests, L, T)
    assert tree.numel() == len(want) == scl.merkle_tree_bytes(L, T)
    assert host_bytes(tree) == want
    assert host_bytes(scl.merkle_root(leaves)) == want[-32 * T:]
    # building in place over a buffer that already holds level 0
    again = torch.zeros_like(tree)
    again[:L * T * 32].copy_(leaves.reshape(-1))
    scl._chk(scl.lib.scl_hip_merkle_build(scl._dev(again), scl._dev(again), L, T, scl._stream()))
    assert torch.equal(again, tree)


def test_root_only_of_a_long_tree(scl):
    L = 2 ** 22 + 3
    raw, digests = random_digests(L, 22)
    root = scl.merkle_root(torch.from_numpy(raw).cuda())
    assert host_bytes(root) == model_levels(digests)[-1][0]


def test_reference_trees_through_the_device_path(scl):
    """tests/golden/golden_merkle.json: the reference's leaves enter as their wire image (scl_hip_wire_unpack), leave as the
    reference's root and the reference's proof"""
    tags = {"Mersenne61": scl.M61, "Mersenne127": scl.M127, "Secp256k1Scalar": scl.SECP256K1_SCALAR, "Secp256k1Field": scl.SECP256K1_FIELD}
    for field, cases in golden().items():
        f = tags[field]
        for c in cases:
            L = c["L"]
            image = L.to_bytes(4, "little") + b"".join(golden_leaves(field, c))
            a = scl.wire_unpack(f, dev_bytes(image))
            assert a.shape[0] == L
            leaves = scl.merkle_leaves(f, a)
            assert host_bytes(scl.merkle_root(leaves)).hex() == c["root"], (field, L)
            tree = scl.merkle_build(leaves)
            assert host_bytes(tree[-32:]).hex() == c["root"]
            path = scl.merkle_paths(tree, L, 1, leaf_index=[c["index"]])
            assert [host_bytes(path[l, 0]).hex() for l in range(path.shape[0])] == c["path"], (field, L)
            ok = scl.merkle_verify(leaves[c["index"]:c["index"] + 1], path, tree[-32:], leaf=c["index"])
            assert ok.tolist() == [1]


def _flip(t: torch.Tensor, rows, byte, bit):
    """flip one bit of row r of a [rows][32] (or [rows]) tensor, for r in rows"""
    t = t.clone()
    idx = torch.as_tensor(rows, device=t.device)
    if t.dim() == 1:
        t[idx] ^= (1 << bit)
    else:
        t[idx, byte] ^= (1 << bit)
    return t


def _check_tampering(scl, leaf_digests, path, roots, leaf_index, root_index, victims):
    """a flipped bit in (a) the leaf digest, (b) one path digest, (c) the index, (d) the root fails exactly the tampered queries"""
    k, depth = path.shape[1], path.shape[0]
    want = np.ones(k, np.uint8)
    want[victims] = 0
    li = torch.as_tensor(leaf_index, dtype=torch.int64, device="cuda")
    ri = torch.as_tensor(root_index, dtype=torch.int64, device="cuda")
    clean = scl.merkle_verify(leaf_digests, path, roots, leaf_index=li, root_index=ri)
    assert clean.cpu().numpy().all()
    a = scl.merkle_verify(_flip(leaf_digests, victims, 5, 3), path, roots, leaf_index=li, root_index=ri)
    assert np.array_equal(a.cpu().numpy(), want)
    bad_path = path.clone()
    for lvl in range(depth):
        rows = [v for v in victims if v % depth == lvl]
        if rows:
            bad_path[lvl] = _flip(path[lvl], rows, 31, 0)
    b = scl.merkle_verify(leaf_digests, bad_path, roots, leaf_index=li, root_index=ri)
    assert np.array_equal(b.cpu().numpy(), want)
    c = scl.merkle_verify(leaf_digests, path, roots, leaf_index=_flip(li, victims, 0, 0), root_index=ri)
    assert np.array_equal(c.cpu().numpy(), want)
    # (d) every query gets a root of its own, the victims' copies are damaged
    own = roots.reshape(-1, 32)[ri].contiguous()
    d = scl.merkle_verify(leaf_digests, path, _flip(own, victims, 0, 7), leaf_index=li)
    assert np.array_equal(d.cpu().numpy(), want)
    # indices out of range are flagged, not followed
    e = scl.merkle_verify(leaf_digests, path, roots, leaf_index=_flip(li, victims, 0, 40), root_index=ri)
    assert np.array_equal(e.cpu().numpy(), want)
    g = scl.merkle_verify(leaf_digests, path, roots, leaf_index=li, root_index=_flip(ri, victims, 0, 33))
    assert np.array_equal(g.cpu().numpy(), want)


def test_paths_and_verify_one_tree(scl):
    """every index of a 33-leaf tree (regular pattern and index array), then 10^4 random indices of a 100003-leaf tree with one
    query in a hundred tampered with.  (The tampered index is flipped in bit 0, and the victims avoid the last leaf of an odd
    level 0: there the sibling IS the node, SHA256(h || h) either way -- the reference's tree cannot tell those two apart.)"""
    raw, digests = random_digests(33, 33)
    leaves = torch.from_numpy(raw).cuda()
    tree = scl.merkle_build(leaves)
    levels = model_levels(digests)
    regular = scl.merkle_paths(tree, 33, 1, k=33)
    listed = scl.merkle_paths(tree, 33, 1, leaf_index=list(range(33)), tree_index=[0] * 33)
    assert torch.equal(regular, listed) and regular.shape == (6, 33, 32)
    for i in range(33):
        assert [host_bytes(regular[l, i]) for l in range(6)] == model_path(levels, i)
    ok = scl.merkle_verify(leaves, regular, tree[-32:], leaf_index=list(range(33)))
    assert ok.cpu().numpy().all()
    with pytest.raises(scl.SclError) as e:
        scl.merkle_paths(tree, 33, 1, first_leaf=1, k=33)
    assert e.value.status == scl.ERR_INVALID_RANGE

    L, k = 100003, 10 ** 4
    raw, digests = random_digests(L, L)
    leaves = torch.from_numpy(raw).cuda()
    tree = scl.merkle_build(leaves)
    levels = model_levels(digests)
    idx = np.random.default_rng(7).integers(0, L - 1, size=k)
    idx[0], idx[1] = L - 1, 0
    path = scl.merkle_paths(tree, L, 1, leaf_index=idx)
    hp = path.cpu().numpy()
    for q in range(k):
        assert [hp[l, q].tobytes() for l in range(hp.shape[0])] == model_path(levels, int(idx[q])), q
    victims = list(range(37, k, 100))
    _check_tampering(scl, leaves[torch.from_numpy(idx).cuda()].contiguous(), path, tree[-32:], idx, np.zeros(k, np.int64), victims)
    # an index past the last leaf is clamped to it
    far = scl.merkle_paths(tree, L, 1, leaf_index=[L + 5, 2 ** 62])
    assert torch.equal(far[:, 0], path[:, 0]) and torch.equal(far[:, 1], path[:, 0])


def test_paths_and_verify_one_party_in_every_tree(scl):
    """the dealer's shape: 100003 trees of 10 leaves (the SoA share matrix), party 0, a middle party and party n - 1 in all of
    them by the regular pattern"""
    L, T = 10, 100003
    raw, digests = random_digests(L * T, 10)
    leaves = torch.from_numpy(raw.reshape(L, T, 32)).cuda()
    tree = scl.merkle_build(leaves)
    roots = tree[-32 * T:]
    per_tree = [model_levels([digests[j * T + t] for j in range(L)]) for t in range(T)]
    assert host_bytes(roots) == b"".join(lv[-1][0] for lv in per_tree)
    for party in (0, 4, L - 1):
        path = scl.merkle_paths(tree, L, T, first_leaf=party)
        assert path.shape == (4, T, 32)
        hp = path.cpu().numpy()
        for t in range(T):
            assert [hp[l, t].tobytes() for l in range(4)] == model_path(per_tree[t], party), (party, t)
        ok = scl.merkle_verify(leaves[party], path, roots, leaf=party)
        assert ok.cpu().numpy().all()
        if party != L - 1 or L % 2 == 0:
            _check_tampering(scl, leaves[party].contiguous(), path, roots, np.full(T, party, np.int64), np.arange(T), list(range(11, T, 100)))
    with pytest.raises(scl.SclError) as e:
        scl.merkle_paths(tree, L, T, first_leaf=L)
    assert e.value.status == scl.ERR_INVALID_RANGE


def test_device_and_host_proofs_are_interchangeable(scl, tmp_path):
    """tests/cxx/test_merkle_api --device: hip::merkleTree / merklePaths build the reference's fixture trees on the GPU, every
    device-built proof verifies under the host mirror's MerkleTree::verify and every host-built one under hip::merkleVerify"""
    cases = str(tmp_path / "cases.txt")
    write_cases(cases)
    r = subprocess.run(["timeout", "-k", "10", "300", mirror_binary("merkle"), cases, "--device"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "(device)" in r.stdout and "24 trees" in r.stdout and " 0 failures" in r.stdout, r.stdout


def test_the_whole_chain_captures_into_a_hip_graph(scl):
    """leaves -> build -> paths -> verify on one stream, captured (torch.cuda.CUDAGraph, single branch) and replayed on new
    shares with identical output: no host read, no allocation behind the library's back"""
    f, n, N = scl.M61, 10, 4099
    shares = scl.vector_random(f, n * N, b"graph-merkle-0").reshape(n, N, 1)
    depth = scl.merkle_depth(n)
    leaves = torch.empty(n, N, 32, dtype=torch.uint8, device="cuda")
    tree = torch.empty(scl.merkle_tree_bytes(n, N), dtype=torch.uint8, device="cuda")
    path = torch.empty(depth, N, 32, dtype=torch.uint8, device="cuda")
    roots = torch.empty(N, 32, dtype=torch.uint8, device="cuda")
    ok = torch.empty(N, dtype=torch.uint8, device="cuda")
    party = 7

    def step():
        st = scl._stream()
        scl.merkle_leaves(f, shares, out=leaves)
        scl._chk(scl.lib.scl_hip_merkle_build(scl._dev(tree), scl._dev(leaves), n, N, st))
        roots.copy_(tree[-32 * N:].reshape(N, 32))
        scl._chk(scl.lib.scl_hip_merkle_paths(scl._dev(path), scl._dev(tree), n, N, None, None, party, N, st))
        scl._chk(scl.lib.scl_hip_merkle_verify(scl._dev(ok), scl._dev(leaves[party]), None, party, scl._dev(path), depth, scl._dev(roots),
                                               None, N, N, st))

    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.synchronize()
    for rep in range(3):
        shares.copy_(scl.vector_random(f, n * N, b"graph-merkle-%d" % (rep + 1)).reshape(n, N, 1))
        for t in (leaves, tree, path, roots, ok):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        captured = [t.clone() for t in (leaves, tree, path, roots, ok)]
        step()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(captured, (leaves, tree, path, roots, ok)))
        assert ok.cpu().numpy().all()
        # and the captured output is the model's, on a sample of the trees
        image = host_bytes(scl.wire_pack(f, shares.reshape(-1, 1)))[4:]
        hl = leaves.cpu().numpy()
        for t in range(0, N, 211):
            lv = model_levels([sha(image[(i * N + t) * 8:(i * N + t) * 8 + 8]) for i in range(n)])
            assert [hl[i, t].tobytes() for i in range(n)] == lv[0]
            assert host_bytes(roots[t]) == lv[-1][0]
            assert [host_bytes(path[l, t]) for l in range(depth)] == model_path(lv, party)
