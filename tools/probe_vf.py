#!/usr/bin/env python3
"""Times the batch-verification kernels (csrc/vf_unit.hip) beside their compositions from entry points that exist without them and
writes profiles/probe_vf.json.

In one process and one run, per field (Mersenne61, Mersenne127, the secp256k1 scalar field), rows in {10, 1}, N in {10^6, 10^7},
plain and product form, reps in {1, 2}:

  call         scl_vf_combine_prg                                  rows N elements of x (2 rows N in the product form)
  two-pass     reps x scl_hip_vector_random, then scl_vf_combine   the call's own two-pass form (what a field that does not fuse runs)
  composition  reps x scl_hip_vector_random, then per row (scl_hip_ew MUL once per row in the product form, then) reps x
               scl_hip_dot: (reps + 2 reps rows (+ 3 rows)) N elements and reps rows host round trips
  matmul       reps x scl_hip_vector_random into the columns of a [N][reps] matrix, then scl_hip_matmul of x [rows][N] with it
               (K = N), after rows scl_hip_ew MUL in the product form -- where scl_hip_matmul accepts the shape; its refusal is
               recorded otherwise
  copy         scl_hip_stream_copy of as many elements as the call reads: the copy kernel's rate on this box
  coin         scl_hip_vector_random of one coefficient vector: the AES block rate beside the call's

The composition and the call are compared on the device once per shape, before anything is timed (`equal`).  Every row records
milliseconds, the elements the call moves by the count of include/scl_hip_vf.h, bytes per second, and that rate as a fraction of
the 8 TB/s peak and of the copy kernel's rate at the same shape; the call's rows also record the ratio of the fastest composition's
time to theirs (above 1: the call is faster), of its own two-pass form's, and its AES blocks per second beside
scl_hip_vector_random's.  HIP events around windows of back-to-back calls on one stream, one warm-up window that is not timed, then
the median of `--reps` windows (as tools/probe_ip.py).  The condition this run checks is stated in DESIGN.md section 17; the tool
only measures and never fails on a figure.

    python tools/probe_vf.py [--reps 5] [--window 0.2] [--counts 1000000 10000000] [--rows 10 1] [--out profiles/probe_vf.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-computation-library_amd"))
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--counts", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--rows", type=int, nargs="+", default=[10, 1])
    ap.add_argument("--fields", nargs="+", default=["m61", "m127", "secp256k1_scalar"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_vf.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import scl_amd as scl
    import scl_amd.vf as vf

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

    seed = b"probe-vf"
    all_fields = {"m61": scl.M61, "m127": scl.M127, "secp256k1_scalar": scl.SECP256K1_SCALAR}
    out_rows = []

    def record(step, call, name, shape, elements, got, copy_rate=None, **extra):
        ms, fastest, slowest, calls = got
        esz = 8 * scl.limbs(all_fields[name])
        rate = elements * esz / (ms * 1e-3)
        row = {"step": step, "call": call, "field": name, **shape, "ms": round(ms, 5), "ms_fastest_window": round(fastest, 5),
               "ms_slowest_window": round(slowest, 5), "calls_per_window": calls, "elements_moved": elements, "bytes_per_s": round(rate, 1),
               "fraction_of_8TBs": round(rate / PEAK, 4)}
        if copy_rate:
            row["fraction_of_copy"] = round(rate / copy_rate, 4)
        row.update(extra)
        out_rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    def filled(f, *shape, counter):
        v = scl.empty(f, *shape)
        flat = v.view(-1, scl.limbs(f))
        scl.vector_random(f, flat.shape[0], b"probe-vf-data", counter0=counter << 40, out=flat)
        return v

    for name in args.fields:
        f = all_fields[name]
        L = scl.limbs(f)
        for N in args.counts:
            B = vf.coin_blocks(f, N)
            coin_buf = scl.empty(f, N)
            coin = record("coin", "scl_hip_vector_random", name, {"N": N}, N, timed(lambda: scl.vector_random(f, N, seed, 0, out=coin_buf)))
            coin_rate = B / (coin["ms"] * 1e-3)
            coin["aes_blocks_per_s"] = round(coin_rate, 1)
            for rows in args.rows:
                x, y = filled(f, rows, N, counter=1), filled(f, rows, N, counter=2)
                tmp = scl.empty(f, N)
                for prod in (False, True):
                    moved = (2 if prod else 1) * rows * N
                    src = (x if not prod else torch.cat([x, y])).view(-1, L)
                    dst = scl.empty(f, src.shape[0])
                    copy = record("copy", "scl_hip_stream_copy", name, {"N": N, "rows": rows, "form": "product" if prod else "plain"}, 2 * moved,
                                  timed(lambda: scl.stream_copy(dst, src)))
                    cr = copy["bytes_per_s"]
                    del src, dst
                    for reps in (1, 2):
                        shape = {"N": N, "rows": rows, "reps": reps, "form": "product" if prod else "plain"}
                        rho = scl.empty(f, reps, N)
                        out, out2 = scl.empty(f, rows, reps), scl.empty(f, rows, reps)
                        s_prg = torch.empty(vf.scratch_bytes(f, rows, reps, N, vf.PRG) // 8, dtype=torch.int64, device="cuda")
                        s_rows = torch.empty(vf.scratch_bytes(f, rows, reps, N, 0) // 8, dtype=torch.int64, device="cuda")
                        yy = y if prod else None

                        def draw():
                            for j in range(reps):
                                scl.vector_random(f, N, seed, j * B, out=rho[j])

                        def composition(keep=None):
                            draw()
                            for r in range(rows):
                                m = scl.ew(f, scl.MUL, x[r], y[r], out=tmp) if prod else x[r]
                                for j in range(reps):
                                    v = scl.dot(f, rho[j], m)
                                    if keep is not None:
                                        keep[r, j] = v.reshape(-1)

                        def two_pass():
                            draw()
                            vf.combine(f, x, rho, yy, out=out2, scratch=s_rows)

                        def call():
                            vf.combine_prg(f, x, yy, seed=seed, counter0=0, reps=reps, out=out, scratch=s_prg)

                        # compared on the device before anything is timed
                        want = np.zeros((rows, reps, L), dtype=np.uint64)
                        composition(want)
                        two_pass()
                        call()
                        torch.cuda.synchronize()
                        equal = bool(np.array_equal(scl.to_host(out), want) and torch.equal(out, out2))
                        comps = [record("combine", f"{reps} x scl_hip_vector_random + per row ({'scl_hip_ew MUL + ' if prod else ''}{reps} x scl_hip_dot)", name,
                                        shape, (reps + 2 * reps * rows + (3 * rows if prod else 0)) * N, timed(composition), cr,
                                        launches=reps + rows * (reps * 2 + (1 if prod else 0)), host_round_trips=reps * rows)]
                        try:
                            rho_t = scl.empty(f, N, reps)
                            xm = scl.empty(f, rows, N)

                            def matmul():
                                draw()
                                rho_t.copy_(rho.transpose(0, 1))
                                if prod:
                                    for r in range(rows):
                                        scl.ew(f, scl.MUL, x[r], y[r], out=xm[r])
                                return scl.matmul(f, xm if prod else x, rho_t)
                            mm_equal = bool(np.array_equal(scl.to_host(matmul()), want))
                            once = window(matmul, 1)
                            mm_call, mm_moved = f"{reps} x scl_hip_vector_random + scl_hip_matmul (K = N)", (reps * 3 + rows + (3 * rows if prod else 0)) * N
                            if once > 10 * comps[0]["ms"]:      # (a wavefront per row at K = N: one call is enough to rule it out)
                                record("combine", mm_call, name, shape, mm_moved, (once, once, once, 1), cr, equal=mm_equal, windows="one call: over ten compositions")
                            else:
                                comps.append(record("combine", mm_call, name, shape, mm_moved, timed(matmul), cr, equal=mm_equal))
                            del rho_t, xm
                        except scl.SclError as e:
                            row = {"step": "combine", "call": "scl_hip_matmul (K = N)", "field": name, **shape, "refused": str(e)[:200]}
                            out_rows.append(row)
                            print(json.dumps(row), flush=True)
                        tp = record("combine", f"{reps} x scl_hip_vector_random + scl_vf_combine", name, shape, (2 * reps + moved // N) * N, timed(two_pass), cr)
                        got = timed(call)
                        best = min(c["ms"] for c in comps)
                        fused = vf.launch_shape(f, reps, True)[3]
                        record("combine", "scl_vf_combine_prg", name, shape, moved, got, cr, path="fused" if fused else "two-pass",
                               composition_over_this=round(best / got[0], 3), two_pass_over_this=round(tp["ms"] / got[0], 3), equal=equal,
                               aes_blocks_per_s=round(reps * B / (got[0] * 1e-3), 1),
                               aes_rate_over_vector_random=round(reps * B / (got[0] * 1e-3) / coin_rate, 3))
                        del rho, out, out2, s_prg, s_rows
                        torch.cuda.empty_cache()
                del x, y, tmp
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        head = {"tool": "tools/probe_vf.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window}
        fh.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in out_rows) + "\n]}\n")  # one row per line


if __name__ == "__main__":
    main()
