#!/usr/bin/env python3
"""Times the random-bit kernels (csrc/rb_unit.hip) beside the engine's per-element inverse and writes profiles/probe_rb.json.

In one process and one run, at N = 2^24:

  yardstick    scl_hip_ew INV with scl_hip_set_tuning("inv_batch", -1): one Fermat chain per element -- a chain within 5 % of the
               square root's; 2 N elements of traffic
  copy         scl_hip_stream_copy of N elements: the copy kernel's rate on this box, the rate the row traffic is charged at
  sqrt         scl_rb_sqrt, all five prime fields (Mont128 at 2^128 - 159)
  bits_finish  scl_rb_bits_finish for rows in {1, 10} over Mersenne61, Mersenne127 and the secp256k1 order: (2 rows + 1) N
               elements and N bytes

Inputs are uniform (about half of them non-residues for sqrt; the chain does not depend on the data) -- for bits_finish u is a
vector of squares, so every column takes the path of a live bit.  Every row records milliseconds, elements per second, bytes per
second, and where the yardstick exists its time and the ratio; the rows = 10 rows also record the bound of the issue, the
yardstick's time plus the row traffic, 2 rows N elements, at the same-run copy rate.  HIP events around windows of
back-to-back calls on one stream, one warm-up window that is not timed, then the median of `--reps` windows; the candidates of
a field alternate window by window, so a drift of the clock meets all of them (as tools/probe_vf.py).  The tool only measures and
never fails on a figure; docs/kernels/rb.md states the targets.

    python tools/probe_rb.py [--reps 5] [--window 0.2] [--count 16777216] [--out profiles/probe_rb.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-computation-library_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--count", type=int, default=1 << 24)
    ap.add_argument("--fields", nargs="+", default=["m61", "m127", "mont128", "secp256k1_scalar", "secp256k1_field"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_rb.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl
    import scl_amd.rb as rb

    def window(fn, calls):
        t = scl.Timer()
        t.start()
        for _ in range(calls):
            fn()
        t.stop()
        return t.elapsed_ms() / calls

    def timed_together(fns):
        """{name: (median, fastest, slowest, calls)} per-call milliseconds; the candidates alternate window by window"""
        calls = {}
        for k, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            calls[k] = max(1, int(args.window * 1e3 / max(window(fn, 3), 1e-3)) + 1)
            window(fn, calls[k])  # warm-up: as long as a measured window
        ms = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, fn in fns.items():
                ms[k].append(window(fn, calls[k]))
        return {k: (statistics.median(v), min(v), max(v), calls[k]) for k, v in ms.items()}

    all_fields = {"m61": scl.M61, "m127": scl.M127, "mont128": scl.MONT128, "secp256k1_scalar": scl.SECP256K1_SCALAR,
                  "secp256k1_field": scl.SECP256K1_FIELD}
    finish_fields = ("m61", "m127", "secp256k1_scalar")
    N = args.count
    out_rows = []

    def record(call, name, got, elements, extra_bytes=0, **extra):
        ms, fastest, slowest, calls = got
        esz = 8 * scl.limbs(all_fields[name])
        row = {"call": call, "field": name, "N": N, "ms": round(ms, 5), "ms_fastest_window": round(fastest, 5), "ms_slowest_window": round(slowest, 5),
               "calls_per_window": calls, "elements_per_s": round(N / (ms * 1e-3), 1), "elements_moved": elements,
               "bytes_per_s": round((elements * esz + extra_bytes) / (ms * 1e-3), 1)}
        row.update(extra)
        out_rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    scl.set_mont128_prime(2 ** 128 - 159)
    scl.set_tuning("inv_batch", -1)
    try:
        for name in args.fields:
            f = all_fields[name]
            a = scl.vector_random(f, N, b"probe-rb-a")
            u = scl.ew(f, scl.MUL, a, a)                    # squares: every column of bits_finish is live
            out, inv_out, copy_out = scl.empty(f, N), scl.empty(f, N), scl.empty(f, N)
            status = torch.empty(N, dtype=torch.uint8, device="cuda")
            fns = {"inv": lambda: scl.ew(f, scl.INV, a, out=inv_out), "copy": lambda: scl.stream_copy(copy_out, a),
                   "sqrt": lambda: rb.sqrt(f, a, 0, out=out, status=status)}
            shares = {}
            if name in finish_fields:
                for rows in (1, 10):
                    r = scl.vector_random(f, rows * N, b"probe-rb-r").view(rows, N, scl.limbs(f))
                    shares[rows] = (r, torch.empty_like(r))
                    fns["finish%d" % rows] = (lambda rows=rows: rb.bits_finish(f, u, shares[rows][0], out=shares[rows][1], status=status))
            got = timed_together(fns)
            esz = 8 * scl.limbs(f)
            yard = record('scl_hip_ew INV, set_tuning("inv_batch", -1)', name, got["inv"], 2 * N)
            copy = record("scl_hip_stream_copy", name, got["copy"], 2 * N)
            copy_rate = copy["bytes_per_s"]
            record("scl_rb_sqrt", name, got["sqrt"], 2 * N, N, yardstick_ms=yard["ms"], over_yardstick=round(got["sqrt"][0] / yard["ms"], 4))
            for rows in sorted(shares):
                traffic_ms = 2 * rows * N * esz / copy_rate * 1e3
                g = got["finish%d" % rows]
                record("scl_rb_bits_finish", name, g, (2 * rows + 1) * N, N, rows=rows, yardstick_ms=yard["ms"], over_yardstick=round(g[0] / yard["ms"], 4),
                       bound_ms=round(yard["ms"] * 1.25 if rows == 1 else yard["ms"] + traffic_ms, 5),
                       bound="1.25 x yardstick" if rows == 1 else "yardstick + 2 rows N elements at the copy rate")
            del a, u, out, inv_out, copy_out, status, shares, fns
            torch.cuda.empty_cache()
    finally:
        scl.set_tuning("inv_batch", 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        head = {"tool": "tools/probe_rb.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window}
        fh.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in out_rows) + "\n]}\n")  # one row per line


if __name__ == "__main__":
    main()
