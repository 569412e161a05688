#!/usr/bin/env python3
"""Times Feldman VSS on the GPU (csrc/ec_unit.hip) and writes profiles/probe_feldman.json.

For (n, t) = (10, 3) and N in {2^12, 2^16, 2^20} secrets: HIP-event time of scl_hip_feldman_commit, of scl_hip_feldman_verify
for one party, and of raw scl_hip_ec_mul_base over N scalars (one warm-up call that is not timed, then the median of `--reps`;
the first repetitions of a short kernel run on a clock that is still ramping, which the median leaves out).  In the same run the
host mirror (math::EC, ss::feldman* of include/scl_hip/, the same point functions) does the same work on one core for a sample
of secrets, scaled to N.  Exits non-zero if the device is slower than that one core at N = 2^16.

    python tools/probe_feldman.py [--reps 5] [--window 0.25] [--out profiles/probe_feldman.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "secure-computation-library_amd"))

HOST = r"""
#include <chrono>
#include <cstdio>
#include "scl_hip/scl.h"
using namespace scl;
using EC = math::EC<math::ec::Secp256k1>;
using FF = EC::ScalarField;
int main() {
  auto prg = util::PRG::create("probe-feldman");
  const int sample = 24;
  double commit = 0, verify = 0, mul = 0;
  bool all = true;
  const auto lb = math::computeLagrangeBasis(math::Vector<FF>::range(4), 7);  // made once, outside the timing, as on the device
  for (int i = 0; i < sample; ++i) {
    const FF secret = FF::random(prg);
    const auto shares = ss::shamirSecretShare(secret, 3, 10, prg);
    auto t0 = std::chrono::steady_clock::now();
    std::vector<EC> c{secret * EC::generator()};
    for (int k = 0; k < 3; ++k) c.push_back(shares[k] * EC::generator());
    auto t1 = std::chrono::steady_clock::now();
    EC v;
    for (int k = 0; k < 4; ++k) v += lb[k] * c[k];
    all = all && v == EC::generator() * shares[6];
    auto t2 = std::chrono::steady_clock::now();
    all = all && !(secret * EC::generator()).isPointAtInfinity();
    auto t3 = std::chrono::steady_clock::now();
    commit += std::chrono::duration<double>(t1 - t0).count();
    verify += std::chrono::duration<double>(t2 - t1).count();
    mul += std::chrono::duration<double>(t3 - t2).count();
  }
  std::printf("{\"ok\":%s,\"commit_s\":%.9f,\"verify_s\":%.9f,\"mul_s\":%.9f}\n", all ? "true" : "false", commit / sample,
              verify / sample, mul / sample);
  return all ? 0 : 1;
}
"""


def host_seconds_per_secret():
    """the mirror on one core: seconds per secret for commit, verify and one multiplication"""
    build = os.path.join(ROOT, "tools", "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(build, "probe_feldman_host.cc"), os.path.join(build, "probe_feldman_host")
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    with open(src, "w") as fh:
        fh.write(HOST)
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src, f"-L{lib}", "-lscl_hip",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_feldman.json"))
    args = ap.parse_args()
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

    host = host_seconds_per_secret()
    f, t, n = scl.SECP256K1_SCALAR, 3, 10
    gtable = scl.ec_base_table()
    rows = []
    for N in (2 ** 12, 2 ** 16, 2 ** 20):
        secrets = scl.vector_random(f, N, b"probe-feldman")
        shares = scl.shamir_share_prg(f, secrets, t, n, b"probe-feldman-seed")
        com, scratch, pts = scl.ec_empty(t + 1, N), scl.ec_empty(2 * N), scl.ec_empty(N)
        ok = torch.empty(N, dtype=torch.uint8, device="cuda")
        lam = scl.feldman_lambda(t, 7)
        ms_commit = timed(lambda: scl.feldman_commit(gtable, secrets, shares, t, out=com))
        ms_verify = timed(lambda: scl.feldman_verify(gtable, shares[6], com, lam, scratch=scratch, out=ok))
        ms_mul = timed(lambda: scl.ec_mul_base(gtable, secrets, out=pts))
        assert bool(ok.all())
        for what, ms, host_s in (("feldman_commit", ms_commit, host["commit_s"]), ("feldman_verify", ms_verify, host["verify_s"]),
                                 ("ec_mul_base", ms_mul, host["mul_s"])):
            ms, fastest, slowest, calls = ms
            rows.append({"call": what, "n": n, "t": t, "N": N, "ms": round(ms, 4), "ms_fastest_window": round(fastest, 4),
                         "ms_slowest_window": round(slowest, 4), "calls_per_window": calls, "per_s": round(N / (ms * 1e-3), 1),
                         "host_one_core_s": round(host_s * N, 4), "speedup_vs_one_core": round(host_s * N / (ms * 1e-3), 1)})
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/probe_feldman.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                   "host_seconds_per_secret": host, "rows": rows}, fh, indent=1)
    slower = [r for r in rows if r["N"] == 2 ** 16 and r["speedup_vs_one_core"] < 1.0]
    if slower:
        sys.exit(f"slower on the device than the host mirror on one core at N = 2^16: {slower}")


if __name__ == "__main__":
    main()
