#!/usr/bin/env python3
"""Times Pedersen VSS on the GPU (csrc/pedersen_unit.hip) against the compositions the library offered before it, and writes
profiles/probe_pedersen.json.

For N in {10^5, 10^6} secrets, in one run:
  * scl_hip_pedersen_commit for (n, t) = (10, 3) against its composition: per commitment row two scl_hip_ec_mul_base launches
    (one per table) and an scl_hip_ec_ew add -- 8 + 4 launches and two point round trips through HBM per commitment;
  * scl_hip_ec_matmul of a 7 x 10 matrix with 10 x N points -- vandermonde(7, 10), and drawn full-width scalars -- against 7
    calls of scl_hip_ec_lincomb;
  * scl_hip_pedersen_verify for one party, on its own.
HIP-event time; one warm-up call that is not timed, a warm-up window, then the median of `--reps` windows of at least `--window`
seconds.  `of_ceiling` is the rate over the static ceiling of DESIGN.md section 12 (1.28e11 field products a second at four
waves per SIMD, from section 10's ~335 vector instructions a product and 3.6 issue cycles an instruction).  `fused_slower` is set
where the fused form is slower than its composition by more than the spread between the composition's windows.

    python tools/probe_pedersen.py [--reps 5] [--window 0.25] [--sizes 100000,1000000] [--out profiles/probe_pedersen.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-computation-library_amd"))

Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
PRODUCTS_PER_S = 1.28e11  # 1 024 SIMDs x 2.4 GHz x 64 lanes / (335 x 3.6)


def chain_products(matrix):
    """field products per output COLUMN of ec_matmul: per row 8 a doubling from the row's top bit down, 12 a set bit"""
    total = 0
    for row in matrix:
        if any(row):
            total += 8 * max(v.bit_length() for v in row) + 12 * sum(bin(v).count("1") for v in row)
    return total


def lincomb_products(matrix):
    """the same rows through k_ec_lincomb: all 256 doublings each"""
    return sum(8 * 256 + 12 * sum(bin(v).count("1") for v in row) for row in matrix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_pedersen.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scl_amd as scl

    def window(fn, calls):
        t = scl.Timer()
        t.start()
        for _ in range(calls):
            fn()
        t.stop()
        return t.elapsed_ms() / calls

    def timed(fn):
        """(median, fastest, slowest) per-call milliseconds over --reps windows of at least --window seconds each"""
        fn()
        torch.cuda.synchronize()
        calls = max(1, int(args.window * 1e3 / max(window(fn, 3), 1e-3)) + 1)
        window(fn, calls)  # warm-up: as long as a measured window
        ms = sorted(window(fn, calls) for _ in range(args.reps))
        return statistics.median(ms), ms[0], ms[-1], calls

    def mont(values):
        return scl.to_device(np.array([[(v % Q * (1 << 256) % Q >> (64 * i)) & (2 ** 64 - 1) for i in range(4)] for v in values],
                                      dtype=np.uint64).reshape(len(values), 4))

    f, t, n, rows_m, p = scl.SECP256K1_SCALAR, 3, 10, 7, 10
    gtable = scl.ec_base_table()
    h = scl.to_host(scl.ec_mul_base(gtable, mont([42])))[0]
    htable = scl.ec_base_table(h)
    rng = np.random.default_rng(12)
    matrices = {"vandermonde(7,10)": [[(i + 1) ** k for k in range(p)] for i in range(rows_m)],
                "full-width 7x10": [[int.from_bytes(rng.bytes(32), "big") % Q for _ in range(p)] for _ in range(rows_m)]}
    out_rows = []

    def record(call, N, fused, composed, products, composed_products, unit):
        ms, lo, hi, calls = fused
        row = {"call": call, "N": N, "ms": round(ms, 4), "ms_fastest_window": round(lo, 4), "ms_slowest_window": round(hi, 4),
               "calls_per_window": calls, "per_s": round(N / (ms * 1e-3), 1), "unit": unit, "field_products_per_unit": products,
               "ceiling_per_s": round(PRODUCTS_PER_S / products, 1), "of_ceiling": round(N / (ms * 1e-3) / (PRODUCTS_PER_S / products), 3)}
        if composed is not None:
            cms, clo, chi, ccalls = composed
            row.update({"composition_ms": round(cms, 4), "composition_ms_fastest_window": round(clo, 4),
                        "composition_ms_slowest_window": round(chi, 4), "composition_calls_per_window": ccalls,
                        "composition_field_products_per_unit": composed_products, "speedup_vs_composition": round(cms / ms, 3),
                        "fused_slower": bool(ms - cms > max(chi - clo, hi - lo))})
        out_rows.append(row)
        print(json.dumps(row), flush=True)

    for N in [int(s) for s in args.sizes.split(",")]:
        secrets = torch.stack([scl.vector_random(f, N, b"probe-pedersen-s"), scl.vector_random(f, N, b"probe-pedersen-r")])
        shares = scl.shamir_share_prg_packed(f, secrets, t, n, b"probe-pedersen-seed")
        com, com2, scratch = scl.ec_empty(t + 1, N), scl.ec_empty(t + 1, N), scl.ec_empty(2 * N)
        tmp = scl.ec_empty(N)
        ok = torch.empty(N, dtype=torch.uint8, device="cuda")

        def composed_commit():
            for k in range(t + 1):
                a, b = (secrets[0], secrets[1]) if k == 0 else (shares[0, k - 1], shares[1, k - 1])
                scl.ec_mul_base(gtable, a, out=com2[k])
                scl.ec_mul_base(htable, b, out=tmp)
                scl.ec_ew(scl.ADD, com2[k], tmp, out=com2[k])

        fused = timed(lambda: scl.pedersen_commit(gtable, htable, secrets, shares, t, out=com))
        composed = timed(composed_commit)
        assert bool(scl.ec_equal(com.reshape(-1, 12), com2.reshape(-1, 12)).all())
        record("pedersen_commit (10,3)", N, fused, composed, (t + 1) * (128 * 11 + 2), (t + 1) * (2 * 705 + 12), "secret")
        lam = scl.feldman_lambda(t, 7)
        verify = timed(lambda: scl.pedersen_verify(gtable, htable, shares[0, 6], shares[1, 6], com, lam, scratch=scratch, out=ok))
        assert bool(ok.all())
        record("pedersen_verify (10,3), index 7", N, verify, None, chain_products([scalars_of(scl, lam)]) + 128 * 11 + 2 + 4, None, "secret")
        del secrets, shares, com, com2, scratch, tmp
        points = scl.ec_empty(p, N)
        for k in range(p):
            scl.ec_mul_base(gtable, scl.vector_random(f, N, b"probe-pedersen-p%d" % k), out=points[k])
        dst, dst2 = scl.ec_empty(rows_m, N), scl.ec_empty(rows_m, N)
        for name, matrix in matrices.items():
            M = mont([v for row in matrix for v in row]).reshape(rows_m, p, 4)

            def composed_matmul():
                for i in range(rows_m):
                    scl.ec_lincomb(points, M[i], out=dst2[i])

            fused = timed(lambda: scl.ec_matmul(M, points, out=dst))
            composed = timed(composed_matmul)
            assert bool(scl.ec_equal(dst.reshape(-1, 12), dst2.reshape(-1, 12)).all())
            record(f"ec_matmul {name}", N, fused, composed, chain_products(matrix), lincomb_products(matrix), "column of 7 points")
        del points, dst, dst2
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/probe_pedersen.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                   "field_products_per_s_ceiling": PRODUCTS_PER_S, "rows": out_rows}, fh, indent=1)


def scalars_of(scl, t):
    """SECP256K1_SCALAR elements on the device -> integers"""
    rinv = pow(1 << 256, -1, Q)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % Q for row in scl.to_host(t).reshape(-1, 4)]


if __name__ == "__main__":
    main()
