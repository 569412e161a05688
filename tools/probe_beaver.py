#!/usr/bin/env python3
"""Times the fused Beaver kernels (csrc/beaver_unit.hip) against the compositions they replace and writes profiles/probe_beaver.json.

In one process and one run, per field (Mersenne61, Mersenne127, GF(2^128), the secp256k1 scalar field), rows = 1, N in {10^6, 10^7}:

  finish   scl_mpc_beaver_finish (e d added)          against  six scl_hip_ew calls with two temporaries:
                                                               t1 = e b, t2 = d a, t1 += t2, t2 = e d, t1 += t2, z = t1 + c
  mask     scl_mpc_beaver_mask                        against  two scl_hip_ew SUB calls (equal traffic: the launch count differs)

The compositions go through entry points the engine has had all along; nothing here times one build of the new code against
another.  HIP events around windows of back-to-back calls on one stream, one warm-up window that is not timed, then the median of
`--reps` windows (as tools/probe_ecdsa.py).  Recorded per row: milliseconds, elements per second, the algorithmic bytes (finish
6 N elements fused and 18 N composed, mask 6 N both) over the time as a fraction of the 8 TB/s HBM peak, and the ratio of the
composition's time to the fused call's.  Both results are compared before anything is timed.  Exits non-zero if the fused finish
is slower than its composition for any field at the largest N; that is the only condition.

    python tools/probe_beaver.py [--reps 5] [--window 0.1] [--counts 1000000 10000000] [--out profiles/probe_beaver.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-computation-library_amd"))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--counts", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_beaver.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl
    import scl_amd.mpc as mpc

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

    fields = (("m61", scl.M61), ("m127", scl.M127), ("gf2_128", scl.GF2_128), ("secp256k1_scalar", scl.SECP256K1_SCALAR))
    rows = []
    for name, f in fields:
        esz = 8 * scl.limbs(f)
        for n in args.counts:
            v = {k: scl.vector_random(f, n, b"probe-beaver-" + k.encode()) for k in ("x", "y", "a", "b", "c", "e", "d")}
            z, zc, t1, t2 = (scl.empty(f, n) for _ in range(4))
            de, dec = scl.empty(f, 2, n), scl.empty(f, 2, n)

            def finish_fused():
                mpc.beaver_finish(f, v["e"], v["d"], v["a"], v["b"], v["c"], 1, out=z)

            def finish_composed():
                scl.ew(f, scl.MUL, v["e"], v["b"], out=t1)
                scl.ew(f, scl.MUL, v["d"], v["a"], out=t2)
                scl.ew(f, scl.ADD, t1, t2, out=t1)
                scl.ew(f, scl.MUL, v["e"], v["d"], out=t2)
                scl.ew(f, scl.ADD, t1, t2, out=t1)
                scl.ew(f, scl.ADD, t1, v["c"], out=zc)

            def mask_fused():
                mpc.beaver_mask(f, v["x"], v["y"], v["a"], v["b"], out=de)

            def mask_composed():
                scl.ew(f, scl.SUB, v["x"], v["a"], out=dec[0])
                scl.ew(f, scl.SUB, v["y"], v["b"], out=dec[1])

            finish_fused(), finish_composed(), mask_fused(), mask_composed()
            torch.cuda.synchronize()
            assert torch.equal(z, zc) and torch.equal(de, dec), f"{name} n={n}: the fused call and the composition disagree"
            for what, fused, composed, fused_elems, composed_elems in (("finish", finish_fused, finish_composed, 6, 18),
                                                                       ("mask", mask_fused, mask_composed, 6, 6)):
                got = {"fused": timed(fused), "composed": timed(composed)}
                for form, elems in (("fused", fused_elems), ("composed", composed_elems)):
                    ms, fastest, slowest, calls = got[form]
                    rows.append({"call": what, "form": form, "field": name, "n": n, "rows": 1, "launches": 1 if form == "fused" else
                                 {"finish": 6, "mask": 2}[what], "ms": round(ms, 5), "ms_fastest_window": round(fastest, 5),
                                 "ms_slowest_window": round(slowest, 5), "calls_per_window": calls, "elements_per_s": round(n / (ms * 1e-3), 1),
                                 "bytes_moved": elems * n * esz, "hbm_fraction_of_8TBps": round(elems * n * esz / (ms * 1e-3) / HBM_PEAK, 4),
                                 "composed_over_fused": round(got["composed"][0] / got["fused"][0], 3)})
                    print(json.dumps(rows[-1]), flush=True)
            del v, z, zc, t1, t2, de, dec
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/probe_beaver.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                   "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, fh, indent=1)
    top = max(args.counts)
    bad = [r for r in rows if r["call"] == "finish" and r["form"] == "fused" and r["n"] == top and r["composed_over_fused"] < 1.0]
    if bad:
        sys.exit(f"the fused finish is slower than the six-call composition at n = {top}: {bad}")


if __name__ == "__main__":
    main()
