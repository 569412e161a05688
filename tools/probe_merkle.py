#!/usr/bin/env python3
"""Times the Merkle kernels (csrc/sha256.hpp, hash_unit.hip) and writes profiles/probe_merkle.json.

Shapes (L leaves, T trees): one long tree (10^7, 1), the dealer's batches (10, 10^7), (40, 10^6), (128, 10^6), and the raw
batched hash (10^7 messages of 64 bytes = two compressions each).  Per shape: HIP-event time of scl_hip_merkle_build over
ready leaf digests (median of `--reps`), compressions per second (a node is two compressions: the data block and the padding
block), and for scale the same tree hashed with hashlib on one host core in the same run (on a sample of the trees, scaled).

    python tools/probe_merkle.py [--reps 5] [--out profiles/probe_merkle.json]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-computation-library_amd"))


def host_tree_seconds(L, T, budget_nodes=400_000):
    """hashlib on one core: whole trees until `budget_nodes` nodes are hashed, scaled to T trees"""
    sha = hashlib.sha256
    leaf = [bytes([i & 255]) * 32 for i in range(min(L, budget_nodes))]
    if L > budget_nodes:                      # one long tree: time one level's worth of node hashes, scale by the node count
        t0 = time.perf_counter()
        for j in range(budget_nodes // 2):
            sha(leaf[2 * j] + leaf[2 * j + 1]).digest()
        return (time.perf_counter() - t0) / (budget_nodes // 2) * nodes_of(L) * T
    trees = max(1, min(T, budget_nodes // max(1, nodes_of(L))))
    t0 = time.perf_counter()
    for _ in range(trees):
        cur = leaf
        while True:
            cur = [sha(cur[2 * j] + cur[min(2 * j + 1, len(cur) - 1)]).digest() for j in range((len(cur) + 1) // 2)]
            if len(cur) == 1:
                break
    return (time.perf_counter() - t0) / trees * T


def nodes_of(L):
    total, n = 0, L
    while True:
        n = (n + 1) // 2
        total += n
        if n == 1:
            return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_merkle.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t = scl.Timer()
            t.start()
            fn()
            t.stop()
            ms.append(t.elapsed_ms())
        return statistics.median(ms)

    rows = []
    for L, T in ((10 ** 7, 1), (10, 10 ** 7), (40, 10 ** 6), (128, 10 ** 6)):
        leaves = torch.randint(0, 256, (L, T, 32), dtype=torch.uint8, device="cuda")
        tree = torch.empty(scl.merkle_tree_bytes(L, T), dtype=torch.uint8, device="cuda")
        tree[:L * T * 32].copy_(leaves.reshape(-1))
        del leaves
        ms = timed(lambda: scl._chk(scl.lib.scl_hip_merkle_build(scl._dev(tree), scl._dev(tree), L, T, scl._stream())))
        comp = 2 * nodes_of(L) * T
        host_s = host_tree_seconds(L, T)
        rows.append({"shape": "build", "L": L, "T": T, "ms": round(ms, 4), "compressions": comp,
                     "compressions_per_s": round(comp / (ms * 1e-3), 1), "hashlib_one_core_s": round(host_s, 3),
                     "speedup_vs_hashlib": round(host_s / (ms * 1e-3), 1)})
        print(json.dumps(rows[-1]), flush=True)
        del tree
    # leaf digests of field elements (one compression each) and the raw batched hash (64-byte messages: two compressions)
    N = 10 ** 7
    a = scl.vector_random(scl.M61, N, b"probe-merkle")
    out = torch.empty(N, 32, dtype=torch.uint8, device="cuda")
    ms = timed(lambda: scl.merkle_leaves(scl.M61, a, out=out))
    rows.append({"shape": "leaves Mersenne61", "count": N, "ms": round(ms, 4), "compressions": N, "compressions_per_s": round(N / (ms * 1e-3), 1)})
    print(json.dumps(rows[-1]), flush=True)
    msgs = torch.randint(0, 256, (N, 64), dtype=torch.uint8, device="cuda")
    ms = timed(lambda: scl._chk(scl.lib.scl_hip_sha256(scl._dev(out), scl._dev(msgs), 64, 64, N, scl._stream())))
    t0 = time.perf_counter()
    blob = bytes(64)
    for _ in range(200_000):
        hashlib.sha256(blob).digest()
    host_s = (time.perf_counter() - t0) / 200_000 * N
    rows.append({"shape": "sha256 of 64-byte messages", "count": N, "ms": round(ms, 4), "compressions": 2 * N,
                 "compressions_per_s": round(2 * N / (ms * 1e-3), 1), "hashlib_one_core_s": round(host_s, 3),
                 "speedup_vs_hashlib": round(host_s / (ms * 1e-3), 1)})
    print(json.dumps(rows[-1]), flush=True)
    slower = [r for r in rows if "hashlib_one_core_s" in r and r["ms"] * 1e-3 >= r["hashlib_one_core_s"]]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/probe_merkle.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, fh, indent=1)
    if slower:
        sys.exit(f"slower on the device than hashlib on one core: {slower}")


if __name__ == "__main__":
    main()
