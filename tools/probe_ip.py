#!/usr/bin/env python3
"""Times the inner- and matrix-product kernels (csrc/ip_unit.hip) beside their compositions from entry points that exist without
them and writes profiles/probe_ip.json.

In one process and one run, per field (Mersenne61, Mersenne127, the secp256k1 scalar field) at (n, t) = (10, 3), so 10 rows:

  dot      scl_ip_dot_mask, terms in {8, 64}, N in {10^6, 10^7}   beside  scl_hm_mul_mask, then scl_hip_ew MUL and ADD per further
                                                                         term: 2 terms - 1 launches, (6 terms - 2) rows N elements
  matmul   scl_ip_matmul_mask, 4 x 4 x 4, batch 10, N = 10^6       beside  the same composition per output entry (its operands laid
                                                                         out [entry][batch][N], so that every call is one dense
                                                                         matrix), and beside a b calls of scl_ip_dot_mask through
                                                                         term strides: what the tile buys
  copy     scl_hip_stream_copy of one operand onto the other (terms rows N elements read and as many written, about what the dot
           call moves): the copy kernel's rate on this box

A shape whose two operands take more than `--budget` GiB (128 by default: under half the card, which other work shares) is left
out and recorded as such.  64 terms of 10 rows at N = 10^7 are 95 GiB for Mersenne61, which runs, 191 GiB for Mersenne127 and
381 GiB for the secp256k1 order, which the default budget leaves out (the last does not fit the card at all).  The composition and the call are compared on
the device once per shape (`equal`).

Every row records milliseconds, the elements the call moves by the count of include/scl_hip_ip.h, bytes per second, and that rate
as a fraction of the 8 TB/s peak and of the copy kernel's rate at the same shape; the extension's rows also record the ratio of
the composition's time to theirs (above 1: the fused call is faster).  HIP events around windows of back-to-back calls on one
stream, one warm-up window that is not timed, then the median of `--reps` windows (as tools/probe_hm.py).  The condition this run
checks is stated in DESIGN.md section 16; the tool only measures and never fails on a figure.

    python tools/probe_ip.py [--reps 5] [--window 0.2] [--budget 128] [--counts 1000000 10000000] [--terms 8 64] [--out profiles/probe_ip.json]
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
    ap.add_argument("--terms", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--matmul-count", type=int, default=10 ** 6)
    ap.add_argument("--budget", type=float, default=128.0, help="GiB the two operands of a dot shape may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_ip.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl
    import scl_amd.hm as hm
    import scl_amd.ip as ip

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

    seed = b"probe-ip"
    rows_n = 10
    fields = (("m61", scl.M61), ("m127", scl.M127), ("secp256k1_scalar", scl.SECP256K1_SCALAR))
    rows = []

    def record(step, call, name, shape, elements, got, copy_rate=None, **extra):
        ms, fastest, slowest, calls = got
        esz = 8 * scl.limbs(dict(fields)[name])
        rate = elements * esz / (ms * 1e-3)
        row = {"step": step, "call": call, "field": name, **shape, "ms": round(ms, 5), "ms_fastest_window": round(fastest, 5),
               "ms_slowest_window": round(slowest, 5), "calls_per_window": calls, "elements_moved": elements, "bytes_per_s": round(rate, 1),
               "fraction_of_8TBs": round(rate / PEAK, 4)}
        if copy_rate:
            row["fraction_of_copy"] = round(rate / copy_rate, 4)
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    def filled(f, *shape):
        v = scl.empty(f, *shape)
        flat = v.view(-1, scl.limbs(f))
        filled.counter += 1
        scl.vector_random(f, flat.shape[0], seed, counter0=filled.counter << 40, out=flat)
        return v
    filled.counter = 0

    for name, f in fields:
        L = scl.limbs(f)
        esz = 8 * L
        for N in args.counts:
            for terms in args.terms:
                shape = {"N": N, "terms": terms, "rows": rows_n}
                need = 2 * terms * rows_n * N * esz
                if need > args.budget * 2 ** 30:
                    row = {"step": "dot", "field": name, **shape, "skipped": f"x and y take {need / 2 ** 30:.0f} GiB, over the budget of {args.budget:.0f} GiB"}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    continue
                x, y = filled(f, terms, rows_n, N), filled(f, terms, rows_n, N)
                r, out, tmp, ref = filled(f, rows_n, N), scl.empty(f, rows_n, N), scl.empty(f, rows_n, N), scl.empty(f, rows_n, N)
                moved = (2 * terms + 2) * rows_n * N
                half = terms * rows_n * N                                      # copy: all of x onto y, about the bytes the call moves
                src, dst = x.view(-1, L), y.view(-1, L)
                copy = record("copy", "scl_hip_stream_copy", name, shape, 2 * half, timed(lambda: scl.stream_copy(dst, src)))
                cr = copy["bytes_per_s"]
                scl.vector_random(f, terms * rows_n * N, seed, counter0=77 << 40, out=y.view(-1, L))    # (the copy wrote over y)

                def composition(o=ref):
                    hm.mul_mask(f, x[0], y[0], r, out=o)
                    for k in range(1, terms):
                        scl.ew(f, scl.MUL, x[k], y[k], out=tmp)
                        scl.ew(f, scl.ADD, o, tmp, out=o)
                comp = record("dot", f"scl_hm_mul_mask + {terms - 1} x (scl_hip_ew MUL + ADD)", name, shape, (6 * terms - 2) * rows_n * N, timed(composition), cr,
                              launches=2 * terms - 1)
                got = timed(lambda: ip.dot_mask(f, x, y, r, out=out))
                torch.cuda.synchronize()
                record("dot", "scl_ip_dot_mask", name, shape, moved, got, cr, launches=1, composition_over_this=round(comp["ms"] / got[0], 3),
                       equal=bool(torch.equal(out, ref)))
                del x, y, r, out, tmp, ref, src, dst
                torch.cuda.empty_cache()

        # the matrix form
        a, K, b, batch, N = 4, 4, 4, rows_n, args.matmul_count
        ti, tl = ip.matmul_tile(f)
        shape = {"N": N, "a": a, "K": K, "b": b, "batch": batch, "tile": [ti, tl]}
        X, Y, R2 = filled(f, batch, a, K, N), filled(f, batch, K, b, N), filled(f, batch, a, b, N)
        D, D2 = scl.empty(f, batch, a, b, N), scl.empty(f, batch, a, b, N)
        # the composition's own layout: [entry][batch][N], every call one dense matrix of `batch` rows
        Xc, Yc, Rc = X.permute(1, 2, 0, 3, 4).contiguous(), Y.permute(1, 2, 0, 3, 4).contiguous(), R2.permute(1, 2, 0, 3, 4).contiguous()
        Dc, tmp = scl.empty(f, a, b, batch, N), scl.empty(f, batch, N)
        moved = (-(-b // tl) * a * K + -(-a // ti) * K * b + 2 * a * b) * batch * N
        half = min(moved // 2, a * K * batch * N, a * b * batch * N)
        copy = record("copy", "scl_hip_stream_copy", name, shape, 2 * half, timed(lambda: scl.stream_copy(D2.view(-1, L)[:half], X.view(-1, L)[:half])))
        cr = copy["bytes_per_s"]

        def composition():
            for i in range(a):
                for l in range(b):
                    hm.mul_mask(f, Xc[i, 0], Yc[0, l], Rc[i, l], out=Dc[i, l])
                    for k in range(1, K):
                        scl.ew(f, scl.MUL, Xc[i, k], Yc[k, l], out=tmp)
                        scl.ew(f, scl.ADD, Dc[i, l], tmp, out=Dc[i, l])
        comp = record("matmul", f"{a * b} x (scl_hm_mul_mask + {K - 1} x (scl_hip_ew MUL + ADD))", name, shape, a * b * (6 * K - 2) * batch * N,
                      timed(composition), cr, launches=a * b * (2 * K - 1))

        def dots():
            for i in range(a):
                for l in range(b):
                    ip.dot_mask(f, X[:, i].transpose(0, 1), Y[:, :, l].transpose(0, 1), R2[:, i, l], out=D2[:, i, l])
        dd = record("matmul", f"{a * b} x scl_ip_dot_mask", name, shape, a * b * (2 * K + 2) * batch * N, timed(dots), cr, launches=a * b)
        got = timed(lambda: ip.matmul_mask(f, X, Y, R2, out=D))
        torch.cuda.synchronize()
        record("matmul", "scl_ip_matmul_mask", name, shape, moved, got, cr, launches=1, composition_over_this=round(comp["ms"] / got[0], 3),
               dots_over_this=round(dd["ms"] / got[0], 3), equal=bool(torch.equal(D, D2) and torch.equal(D.permute(1, 2, 0, 3, 4), Dc)))
        del X, Y, R2, D, D2, Xc, Yc, Rc, Dc, tmp
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        head = {"tool": "tools/probe_ip.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                "shape": {"rows": rows_n}}
        fh.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")  # one row per line


if __name__ == "__main__":
    main()
