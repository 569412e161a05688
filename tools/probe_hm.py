#!/usr/bin/env python3
"""Times the honest-majority multiplication kernels (csrc/hm_unit.hip) beside their compositions from the engine's entry points
and writes profiles/probe_hm.json.

In one process and one run, per field (Mersenne61, Mersenne127, the secp256k1 scalar field) at (n, t) = (10, 3) and N in
{10^6, 10^7} columns:

  apply          scl_hm_apply, the 7 x 10 hyper-invertible matrix over one party's 10 rows  beside  7 scl_hip_shamir_recover calls
                 (row k of M as lambda) and beside one scl_hip_matmul of the same operands
  mask           scl_hm_mul_mask over 10 rows              beside  scl_hip_ew MUL then ADD over the same 10 N elements
  finish         scl_hm_mul_finish, m = 10, 10 rows         beside  scl_hip_shamir_recover then 10 scl_hip_ew SUB calls
  double share   scl_hm_double_share_prg                   beside  scl_hip_shamir_share_prg at (10, 3), in AES blocks per second:
                 B per double sharing for the dealer, ceil((t+1) E / 16) per secret for the engine's call
  copy           scl_hip_stream_copy of as many bytes as apply moves: the copy kernel's rate on this box

Every row records milliseconds, the elements the call moves by the count of include/scl_hip_hm.h, bytes per second, and that rate
as a fraction of the 8 TB/s peak and of the copy kernel's rate at the same N; the extension's rows also record the ratio of the
fastest composition's time to theirs (above 1: the fused call is faster).  HIP events around windows of back-to-back calls on
one stream, one warm-up window that is not timed, then the median of `--reps` windows (as tools/probe_triples.py).  The
condition this run checks is stated in DESIGN.md section 15; the tool only measures and never fails on a figure.

    python tools/probe_hm.py [--reps 5] [--window 0.1] [--counts 1000000 10000000] [--out profiles/probe_hm.json]
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
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--counts", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_hm.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl
    import scl_amd.hm as hm

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

    seed = b"probe-hm"
    n, t = 10, 3
    m = n - t
    fields = (("m61", scl.M61), ("m127", scl.M127), ("secp256k1_scalar", scl.SECP256K1_SCALAR))
    rows = []

    def record(step, call, name, N, elements, got, copy_rate=None, **extra):
        ms, fastest, slowest, calls = got
        esz = 8 * scl.limbs(dict(fields)[name])
        rate = elements * esz / (ms * 1e-3)
        row = {"step": step, "call": call, "field": name, "N": N, "ms": round(ms, 5), "ms_fastest_window": round(fastest, 5),
               "ms_slowest_window": round(slowest, 5), "calls_per_window": calls, "elements_moved": elements, "bytes_per_s": round(rate, 1),
               "fraction_of_8TBs": round(rate / PEAK, 4)}
        if copy_rate:
            row["fraction_of_copy"] = round(rate / copy_rate, 4)
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    for name, f in fields:
        L = scl.limbs(f)
        M = hm.hyper_invertible(f, m, n)
        Md = scl.to_device(M)
        lam = scl.lagrange_basis(f, n)
        for N in args.counts:
            mats = [scl.empty(f, n, N) for _ in range(4)]            # x / in, y, r, and an output of n rows
            x, y, r, out = mats
            for k, v in enumerate((x, y, r)):
                scl.vector_random(f, n * N, seed, counter0=k << 40, out=v.view(n * N, L))
            vec = scl.empty(f, N)
            scl.vector_random(f, N, seed, counter0=3 << 40, out=vec)
            # copy: as many bytes as apply moves, read + written
            half = (n + m) * N // 2
            src, dst = x.view(-1, L)[:half], out.view(-1, L)[:half]
            got = timed(lambda: scl.stream_copy(dst, src))
            copy = record("copy", "scl_hip_stream_copy", name, N, 2 * half, got)
            cr = copy["bytes_per_s"]

            # apply
            rec = record("apply", "7 x scl_hip_shamir_recover", name, N, (n + 1) * m * N,
                         timed(lambda: [scl.shamir_recover(f, x, lam=M[k], out=out[k]) for k in range(m)]), cr)
            mm = record("apply", "scl_hip_matmul", name, N, (n + m) * N, timed(lambda: matmul(f, Md, x, out, m, n, N)), cr)
            ap_ = timed(lambda: hm.apply_matrix(f, Md, x, out=out[:m]))
            record("apply", "scl_hm_apply", name, N, (n + m) * N, ap_, cr, kernel="thin (n <= 16: the inputs of a column in registers)",
                   fastest_composition_over_this=round(min(rec["ms"], mm["ms"]) / ap_[0], 3), recover_over_this=round(rec["ms"] / ap_[0], 3),
                   matmul_over_this=round(mm["ms"] / ap_[0], 3))

            # mask
            def mul_add():
                scl.ew(f, scl.MUL, x, y, out=out)
                scl.ew(f, scl.ADD, out, r, out=out)
            comp = record("mask", "scl_hip_ew MUL + ADD", name, N, 6 * n * N, timed(mul_add), cr)
            got = timed(lambda: hm.mul_mask(f, x, y, r, out=out))
            record("mask", "scl_hm_mul_mask", name, N, 4 * n * N, got, cr, fastest_composition_over_this=round(comp["ms"] / got[0], 3))

            # finish
            def recover_sub():
                scl.shamir_recover(f, x, lam=lam, out=vec)
                for k in range(n):
                    scl.ew(f, scl.SUB, vec, r[k], out=out[k])
            comp = record("finish", "scl_hip_shamir_recover + 10 x scl_hip_ew SUB", name, N, (n + 1 + 3 * n) * N, timed(recover_sub), cr)
            got = timed(lambda: hm.mul_finish(f, x, r, lam=lam, out=out))
            record("finish", "scl_hm_mul_finish", name, N, (n + 2 * n) * N, got, cr, fastest_composition_over_this=round(comp["ms"] / got[0], 3))

            # double share: AES blocks per second beside the engine's PRG-driven share call
            B, per_secret = hm.double_blocks(f, n, t), scl.blocks_per_secret(f, t)
            need = hm.double_scratch_bytes(f, N, n, t)
            scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda") if need else None
            eng = timed(lambda: scl.shamir_share_prg(f, vec, t, n, seed, out=out))
            eng_rate = N * per_secret / (eng[0] * 1e-3)
            record("double share", "scl_hip_shamir_share_prg", name, N, (n + 1) * N, eng, cr, blocks_per_item=per_secret, aes_blocks_per_s=round(eng_rate, 1))
            got = timed(lambda: hm.double_share(f, N, t, n, seed, out=(x, y), scratch=scratch))
            rate = N * B / (got[0] * 1e-3)
            record("double share", "scl_hm_double_share_prg", name, N, 2 * n * N + (2 * (1 + 3 * t) * N if need else 0), got, cr, blocks_per_item=B,
                   aes_blocks_per_s=round(rate, 1), path="two-pass" if need else "fused", block_rate_over_engine_share=round(rate / eng_rate, 3))
            del mats, x, y, r, out, vec, src, dst, scratch
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        head = {"tool": "tools/probe_hm.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                "shape": {"n": n, "t": t, "m": m}}
        fh.write(json.dumps(head)[:-1] + ', "rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n")  # one row per line


def matmul(f, Md, x, out, m, n, N):
    """scl_hip_matmul of the m x n matrix and the n x N share matrix, into the first m rows of out"""
    import ctypes as C
    import scl_amd as scl
    rc = scl.lib.scl_hip_matmul(f, C.c_void_p(out.data_ptr()), C.c_size_t(N), C.c_void_p(Md.data_ptr()), C.c_size_t(n), C.c_void_p(x.data_ptr()),
                                C.c_size_t(N), C.c_size_t(m), C.c_size_t(n), C.c_size_t(N), scl._stream())
    if rc:
        raise scl.SclError(rc, scl.lib.scl_hip_last_error().decode())


if __name__ == "__main__":
    main()
