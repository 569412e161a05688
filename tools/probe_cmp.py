#!/usr/bin/env python3
"""Times the comparison kernels (csrc/cmp_unit.hip) beside the composition the parent tree offers and writes profiles/probe_cmp.json.

In one process and one run, over Mersenne61 and Mersenne127, rows in {1, 10} and w in {16, 40, max}, N chosen per row so that the
call's working set is about `--bytes` (1.5 GiB: several times the 256 MB Infinity Cache):

  level       scl_cmp_level_mask at the node count of the tree's second level made even, cnt = 2 (ceil(w / 2) // 2): 8 rows N
              elements per pair
  yardstick   the same level from the calls the parent tree has, over a de-interleaved layout (lt_lo, eq_lo, lt_hi, eq_hi, r_lt,
              r_eq each [pairs rows][N], contiguous): scl_hm_mul_mask(eq_hi, lt_lo, r_lt) -> t, scl_hm_mul_mask(eq_hi, eq_lo, r_eq)
              -> d_eq, scl_hip_ew ADD(t, lt_hi) -> d_lt: 11 rows N elements per pair
  first       scl_cmp_first_mask at m = 4: (m + (w + 4 ceil(w / 2)) rows + 1) N elements and N bytes.  No composition of existing
              calls produces it: there is no yardstick
  finish      scl_cmp_finish (SCL_CMP_TRUNC): (4 rows + 1) N elements and N bytes
  copy        scl_hip_stream_copy of a buffer of `--bytes` / 2: the copy kernel's rate in this run, the rate the computed bounds
              are charged at

Every row records milliseconds with the fastest and the slowest window, bytes per second, the computed bound (the call's traffic at
the same-run copy rate) and the fraction of it reached; a level row also the yardstick's time, the ratio and `not_slower`: level <=
yardstick + the row's own window spread (slowest - fastest of either), and whether both gave the same words.  HIP events around
windows of back-to-back calls on one stream, one warm-up window that is not timed, then the median of `--reps` windows; the
candidates of a row alternate window by window, so a drift of the clock meets all of them (as tools/probe_fx.py).  The tool only
measures and never fails on a figure; docs/kernels/cmp.md states what is expected.

    python tools/probe_cmp.py [--reps 5] [--window 0.2] [--bytes 1610612736] [--out profiles/probe_cmp.json]
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
    ap.add_argument("--bytes", type=int, default=3 << 29)
    ap.add_argument("--fields", nargs="+", default=["m61", "m127"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_cmp.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl
    import scl_amd.cmp as cmp
    import scl_amd.fx as fx
    import scl_amd.hm as hm

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
    out_rows = []

    def record(call, name, got, N, elements, copy_rate, extra_bytes=0, **extra):
        ms, fastest, slowest, calls = got
        esz = 8 * scl.limbs(all_fields[name])
        nbytes = elements * esz + extra_bytes
        row = {"call": call, "field": name, "N": N, "ms": round(ms, 5), "ms_fastest_window": round(fastest, 5), "ms_slowest_window": round(slowest, 5),
               "calls_per_window": calls, "elements_moved": elements, "bytes_per_s": round(nbytes / (ms * 1e-3), 1)}
        if copy_rate:
            row["bound_ms"] = round(nbytes / copy_rate * 1e3, 5)
            row["fraction_of_bound"] = round(row["bound_ms"] / ms, 4)
        row.update(extra)
        out_rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    scl.set_mont128_prime(2 ** 128 - 159)
    for name in args.fields:
        f = all_fields[name]
        L, esz, top = scl.limbs(f), 8 * scl.limbs(f), fx.max_bits(f)
        src = scl.vector_random(f, args.bytes // 2 // esz, b"probe-cmp-copy")
        dst = torch.empty_like(src)
        copy = lambda: scl.stream_copy(dst, src)
        for rows in (1, 10):
            for w in (16, 40, top - 1):
                B, m = w + 1, 4
                # ---- a later level against the composition ----
                cnt = 2 * (((w + 1) // 2) // 2)
                pairs = cnt // 2
                N = min(1 << 25, args.bytes // (8 * pairs * rows * esz) // 512 * 512)
                nodes = scl.vector_random(f, rows * 2 * cnt * N, b"probe-cmp-nodes").view(rows, 2 * cnt, N, L).transpose(0, 1)
                r2 = scl.vector_random(f, rows * cnt * N, b"probe-cmp-r2").view(rows, cnt, N, L).transpose(0, 1)
                d = scl.empty(f, rows, cnt, N).transpose(0, 1)
                level = lambda: cmp.level_mask(f, nodes, r2, out=d)
                # the de-interleaved layout: [pairs rows][N] each, the pair index outermost
                quad = nodes.reshape(pairs, 4, rows, N, L)
                lt_lo, eq_lo, lt_hi, eq_hi = (quad[:, i].reshape(pairs * rows, N, L).contiguous() for i in range(4))
                r_lt, r_eq = (r2.reshape(pairs, 2, rows, N, L)[:, i].reshape(pairs * rows, N, L).contiguous() for i in range(2))
                t, d_lt, d_eq = (scl.empty(f, pairs * rows, N) for _ in range(3))

                def yard():
                    hm.mul_mask(f, eq_hi, lt_lo, r_lt, out=t)
                    hm.mul_mask(f, eq_hi, eq_lo, r_eq, out=d_eq)
                    scl.ew(f, scl.ADD, t, lt_hi, out=d_lt)

                got = timed_together({"yardstick": yard, "level": level, "copy": copy})
                want_lt, want_eq = (d.reshape(pairs, 2, rows, N, L)[:, i].reshape(pairs * rows, N, L) for i in range(2))
                same = torch.equal(d_lt, want_lt) and torch.equal(d_eq, want_eq)
                lv, yd = got["level"], got["yardstick"]
                rate = record("scl_hip_stream_copy", name, got["copy"], src.shape[0], 2 * src.shape[0], None)["bytes_per_s"]
                y = record("2 scl_hm_mul_mask + scl_hip_ew ADD", name, yd, N, 11 * pairs * rows * N, rate, rows=rows, w=w, cnt=cnt)
                spread = max(lv[2] - lv[1], yd[2] - yd[1])
                record("scl_cmp_level_mask", name, lv, N, 8 * pairs * rows * N, rate, rows=rows, w=w, cnt=cnt, yardstick_ms=y["ms"],
                       over_yardstick=round(lv[0] / y["ms"], 4), window_spread_ms=round(spread, 5), not_slower=bool(lv[0] <= y["ms"] + spread),
                       equals_yardstick=same)
                del nodes, r2, d, quad, lt_lo, eq_lo, lt_hi, eq_hi, r_lt, r_eq, want_lt, want_eq, t, d_lt, d_eq
                torch.cuda.empty_cache()
                # ---- the first level ----
                half = (w + 1) // 2
                per_col = m + (w + 4 * half) * rows + 1
                N = min(1 << 25, args.bytes // (per_col * esz) // 512 * 512)
                bits = scl.vector_random(f, rows * w * N, b"probe-cmp-bits").view(rows, w, N, L).transpose(0, 1)
                r2 = scl.vector_random(f, rows * 2 * half * N, b"probe-cmp-r2").view(rows, 2 * half, N, L).transpose(0, 1)
                d = scl.empty(f, rows, 2 * half, N).transpose(0, 1)
                csh = scl.vector_random(f, m * N, b"probe-cmp-csh").view(m, N, L)
                cmod, status, lam = scl.empty(f, N), torch.empty(N, dtype=torch.uint8, device="cuda"), scl.lagrange_basis(f, m)
                got = timed_together({"first": lambda: cmp.first_mask(f, csh, bits, r2, w, B, lam=lam, out=d, cmod=cmod, status=status), "copy": copy})
                rate = record("scl_hip_stream_copy", name, got["copy"], src.shape[0], 2 * src.shape[0], None)["bytes_per_s"]
                record("scl_cmp_first_mask", name, got["first"], N, per_col * N, rate, N, rows=rows, w=w, B=B, m=m)
                del bits, r2, d, csh
                torch.cuda.empty_cache()
                # ---- the finish ----
                N = min(1 << 25, args.bytes // ((4 * rows + 1) * esz) // 512 * 512)
                lt, rlow, x = (scl.vector_random(f, rows * N, b"probe-cmp-" + t).view(rows, N, L) for t in (b"lt", b"rlow", b"x"))
                cmod, status, y = scl.vector_random(f, N, b"probe-cmp-cmod"), torch.zeros(N, dtype=torch.uint8, device="cuda"), scl.empty(f, rows, N)
                got = timed_together({"finish": lambda: cmp.finish(f, lt, cmod, status, rlow, x, w, cmp.TRUNC, out=y), "copy": copy})
                rate = record("scl_hip_stream_copy", name, got["copy"], src.shape[0], 2 * src.shape[0], None)["bytes_per_s"]
                record("scl_cmp_finish", name, got["finish"], N, (4 * rows + 1) * N, rate, N, rows=rows, w=w, what="SCL_CMP_TRUNC")
                del lt, rlow, x, cmod, status, y
                torch.cuda.empty_cache()
        del src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        head = {"tool": "tools/probe_cmp.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window, "bytes": args.bytes}
        fh.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in out_rows) + "\n]}\n")  # one row per line


if __name__ == "__main__":
    main()
