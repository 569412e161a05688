#!/usr/bin/env python3
"""Times the triple dealer (csrc/triples_unit.hip) beside the engine's closest PRG-driven calls and writes profiles/probe_triples.json.

In one process and one run, per field (Mersenne61, Mersenne127, the secp256k1 scalar field) and N in {10^6, 10^7} triples:

  additive n = 3      scl_prep_triples_additive_prg     beside  scl_hip_additive_share_prg at n = 3 (one sharing of N secrets)
  Shamir (10, 3)      scl_prep_triples_shamir_prg       beside  scl_hip_shamir_share_prg at (10, 3)
  (both)              scl_hip_prg_blocks over as many blocks as the triples consume: the AES rate with one 16-byte store per block
  composition         two vector_random, one MUL and three *_share_prg calls: the order-free way to triples from existing entry
                      points.  For information only: it draws fewer blocks and deals OTHER triples than the reference, so it is
                      not a bar.

Every row records milliseconds, items per second and AES blocks per second (items/s times the blocks one item consumes: B per
triple for the dealer, n - 1 or ceil((t+1) E / 16) blocks per secret for the engine's share calls), and the dealer's rows the
ratio of their block rate to the engine call's.  HIP events around windows of back-to-back calls on one stream, one warm-up
window that is not timed, then the median of `--reps` windows (as tools/probe_beaver.py).  The expectation this run checks is
stated in DESIGN.md section 14; the tool only measures and never fails on a figure.

    python tools/probe_triples.py [--reps 5] [--window 0.1] [--counts 1000000 10000000] [--out profiles/probe_triples.json]
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
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--counts", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_triples.json"))
    args = ap.parse_args()
    import torch
    import scl_amd as scl
    import scl_amd.prep as prep

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

    seed = b"probe-triples"
    n_add, n_sh, t_sh = 3, 10, 3
    fields = (("m61", scl.M61), ("m127", scl.M127), ("secp256k1_scalar", scl.SECP256K1_SCALAR))
    rows = []

    def record(call, scheme, name, N, blocks_per_item, got, **extra):
        ms, fastest, slowest, calls = got
        row = {"call": call, "scheme": scheme, "field": name, "n_items": N, "blocks_per_item": blocks_per_item, "ms": round(ms, 5),
               "ms_fastest_window": round(fastest, 5), "ms_slowest_window": round(slowest, 5), "calls_per_window": calls,
               "items_per_s": round(N / (ms * 1e-3), 1), "aes_blocks_per_s": round(N * blocks_per_item / (ms * 1e-3), 1)}
        row.update(extra)
        rows.append(row)
        print(json.dumps(row), flush=True)
        return row

    for name, f in fields:
        bpe = (8 * scl.limbs(f) + 15) // 16
        for N in args.counts:
            for scheme, n, t in (("additive", n_add, None), ("shamir", n_sh, t_sh)):
                shamir = t is not None
                B = prep.triple_blocks(f, prep.SHAMIR if shamir else prep.ADDITIVE, n, t or 0)
                per_secret = scl.blocks_per_secret(f, t) if shamir else (n - 1) * bpe
                abc = [scl.empty(f, n, N) for _ in range(3)]
                shares = scl.empty(f, n, N)
                secrets, a, b, c = (scl.empty(f, N) for _ in range(4))
                scl.vector_random(f, N, seed, out=secrets)
                need = prep.triples_scratch_bytes(f, N, n, t, 0) if shamir else 0
                scratch = torch.empty(need // 8, dtype=torch.int64, device="cuda") if need else None
                blocks_out = torch.empty(N * B * 16, dtype=torch.uint8, device="cuda")

                def deal():
                    if shamir:
                        prep.deal_triples_shamir(f, N, t, n, seed, out=abc, scratch=scratch)
                    else:
                        prep.deal_triples_additive(f, N, n, seed, out=abc)

                def engine_share():
                    if shamir:
                        scl.shamir_share_prg(f, secrets, t, n, seed, out=shares)
                    else:
                        scl.additive_share_prg(f, secrets, n, seed, out=shares)

                def blocks():
                    scl.prg_blocks(N * B, seed, out=blocks_out)

                def composition():
                    scl.vector_random(f, N, seed, counter0=0, out=a)
                    scl.vector_random(f, N, seed, counter0=1 << 40, out=b)
                    scl.ew(f, scl.MUL, a, b, out=c)
                    for k, v in enumerate((a, b, c)):
                        if shamir:
                            scl.shamir_share_prg(f, v, t, n, seed, out=abc[k], counter0=(k + 2) << 40)
                        else:
                            scl.additive_share_prg(f, v, n, seed, out=abc[k], counter0=(k + 2) << 40)

                path = "two-pass" if need else ("fused" if shamir else "one launch")
                eng = record("scl_hip_shamir_share_prg" if shamir else "scl_hip_additive_share_prg", scheme, name, N, per_secret, timed(engine_share),
                             parties=n, threshold=t)
                record("scl_hip_prg_blocks", scheme, name, N, B, timed(blocks), parties=n, threshold=t)
                got = timed(deal)
                rate = N * B / (got[0] * 1e-3)
                record("scl_prep_triples_shamir_prg" if shamir else "scl_prep_triples_additive_prg", scheme, name, N, B, got, parties=n, threshold=t,
                       path=path, block_rate_over_engine_share=round(rate / eng["aes_blocks_per_s"], 3))
                record("composition (information only)", scheme, name, N, 2 * bpe + 3 * per_secret, timed(composition), parties=n, threshold=t)
                del abc, shares, secrets, a, b, c, scratch, blocks_out
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/probe_triples.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                   "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
