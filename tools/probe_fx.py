#!/usr/bin/env python3
"""Times the truncation kernels (csrc/fx_unit.hip) beside the composition the parent tree offers and writes profiles/probe_fx.json.

In one process and one run, over Mersenne61 and Mersenne127, rows in {1, 10} and B in {16, 40, max}, N chosen per row so that the
call's working set, (B + 3) rows N elements, is about `--bytes` (1.5 GiB: several times the 256 MB Infinity Cache):

  yardstick   scl_hm_apply with the 2 x B matrix of powers of two (row 0: 2^i; row 1: 2^i below `shift`, else 0; n = B, batch =
              rows, in_stride = plane_stride, in_batch_stride = row_stride), then the two scl_hip_ew additions that form
              c = (x + r) + 2^(k-1): at least (B + 8) rows N elements
  mask        scl_fx_trunc_mask: (B + 3) rows N elements
  copy        scl_hip_stream_copy of a buffer of `--bytes` / 2: the copy kernel's rate in this run, the rate the computed bounds
              are charged at
and per field and rows, at m = 4 and B = 40, N from (m + 3 rows) N elements:
  hm_finish   scl_hm_mul_finish: (m + 2 rows) N elements
  finish      scl_fx_trunc_finish: (m + 3 rows) N elements and N bytes (no branch of the kernel depends on the data)

Every row records milliseconds with the fastest and the slowest window, bytes per second, the computed bound (the call's traffic at
the same-run copy rate) and the fraction of it reached; a mask row also the yardstick's time, the ratio and `not_slower`: mask <=
yardstick + the row's own window spread (slowest - fastest of either); a finish row the ratio to hm_finish and the ratio of
the two traffics.  HIP events around windows of back-to-back calls on one stream, one warm-up window that is not timed, then the
median of `--reps` windows; the candidates of a row alternate window by window, so a drift of the clock meets all of them (as
tools/probe_rb.py).  The tool only measures and never fails on a figure; docs/kernels/fx.md states what is expected.

    python tools/probe_fx.py [--reps 5] [--window 0.2] [--bytes 1610612736] [--out profiles/probe_fx.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_fx.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scl_amd as scl
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
        src = scl.vector_random(f, args.bytes // 2 // esz, b"probe-fx-copy")
        dst = torch.empty_like(src)
        copy = lambda: scl.stream_copy(dst, src)
        for rows in (1, 10):
            for B in (16, 40, top):
                k, shift = B - 8, (B - 8) // 2
                N = min(1 << 25, args.bytes // ((B + 3) * rows * esz) // 512 * 512)
                bits = scl.vector_random(f, rows * B * N, b"probe-fx-bits").view(rows, B, N, L)      # plane_stride N, row_stride B N
                x = scl.vector_random(f, rows * N, b"probe-fx-x").view(rows, N, L)
                c, rlow, t, yc = (scl.empty(f, rows, N) for _ in range(4))
                rr = scl.empty(f, 2, rows, N)                                                        # r and r' of the yardstick
                bias = scl.to_device(np.tile(hm.element(f, 1 << (k - 1)), (rows * N, 1))).view(rows, N, L)
                M = scl.to_device(np.stack([np.stack([hm.element(f, 1 << i) for i in range(B)]),
                                            np.stack([hm.element(f, (1 << i) if i < shift else 0) for i in range(B)])]))
                planes = bits.transpose(0, 1)

                def yard():
                    hm.apply_matrix(f, M, bits, out=rr.transpose(0, 1))
                    scl.ew(f, scl.ADD, x, rr[0], out=t)
                    scl.ew(f, scl.ADD, t, bias, out=yc)

                got = timed_together({"yardstick": yard, "mask": lambda: fx.trunc_mask(f, x, planes, k, shift, out=c, rlow=rlow), "copy": copy})
                same = torch.equal(c, yc) and torch.equal(rlow, rr[1])
                cp = record("scl_hip_stream_copy", name, got["copy"], src.shape[0], 2 * src.shape[0], None)
                rate = cp["bytes_per_s"]
                y = record("scl_hm_apply 2 x B + 2 scl_hip_ew ADD", name, got["yardstick"], N, (B + 8) * rows * N, rate, rows=rows, B=B)
                spread = max(got["mask"][2] - got["mask"][1], got["yardstick"][2] - got["yardstick"][1])
                record("scl_fx_trunc_mask", name, got["mask"], N, (B + 3) * rows * N, rate, rows=rows, B=B, k=k, shift=shift, yardstick_ms=y["ms"],
                       over_yardstick=round(got["mask"][0] / y["ms"], 4), window_spread_ms=round(spread, 5),
                       not_slower=bool(got["mask"][0] <= y["ms"] + spread), equals_yardstick=same)
                del bits, x, c, rlow, t, yc, rr, bias, M, planes
                torch.cuda.empty_cache()
            m, B, shift = 4, 40, 16
            N = min(1 << 25, args.bytes // ((m + 3 * rows) * esz) // 512 * 512)
            csh = scl.vector_random(f, m * N, b"probe-fx-csh").view(m, N, L)
            x = scl.vector_random(f, rows * N, b"probe-fx-x").view(rows, N, L)
            rlow = scl.vector_random(f, rows * N, b"probe-fx-rlow").view(rows, N, L)
            y, z = scl.empty(f, rows, N), scl.empty(f, rows, N)
            status = torch.empty(N, dtype=torch.uint8, device="cuda")
            lam = scl.lagrange_basis(f, m)
            got = timed_together({"hm_finish": lambda: hm.mul_finish(f, csh, x, lam=lam, out=z),
                                  "finish": lambda: fx.trunc_finish(f, csh, x, rlow, shift, B, lam=lam, out=y, status=status), "copy": copy})
            rate = record("scl_hip_stream_copy", name, got["copy"], src.shape[0], 2 * src.shape[0], None)["bytes_per_s"]
            h = record("scl_hm_mul_finish", name, got["hm_finish"], N, (m + 2 * rows) * N, rate, rows=rows, m=m)
            record("scl_fx_trunc_finish", name, got["finish"], N, (m + 3 * rows) * N, rate, N, rows=rows, m=m, B=B, shift=shift, hm_finish_ms=h["ms"],
                   over_hm_finish=round(got["finish"][0] / h["ms"], 4), traffic_ratio=round((m + 3 * rows) / (m + 2 * rows), 4))
            del csh, x, rlow, y, z, status
            torch.cuda.empty_cache()
        del src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        head = {"tool": "tools/probe_fx.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window, "bytes": args.bytes}
        fh.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in out_rows) + "\n]}\n")  # one row per line


if __name__ == "__main__":
    main()
