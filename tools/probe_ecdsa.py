#!/usr/bin/env python3
"""Times batched ECDSA on the GPU (csrc/ecdsa_unit.hip) and writes profiles/probe_ecdsa.json.

For n in {10^5, 10^6} signatures: HIP-event time of scl_hip_ec_mul (a point and a scalar per lane), scl_hip_ecdsa_sign,
scl_hip_ecdsa_verify with a key per lane and scl_hip_ecdsa_verify_base with one signer's table (one warm-up call that is not
timed, then the median of `--reps` windows, as tools/probe_feldman.py does), and of scl_hip_ec_lincomb with m = 1 at the same
count: the 1-bit chain the window ladder of ec_mul has to beat.  In the same run the host mirror (util::ECDSA and math::EC of
include/scl_hip/, the same point functions) does the same work on one core for a sample of signatures, scaled to n: ec_mul
against the host's pt_mul_window (the same ladder; EC::operator*, the 1-bit chain, is recorded beside it as mul_bit_ladder_s),
ec_lincomb_m1 against that 1-bit chain, sign and verify against util::ECDSA::Sign / verify.  The mirror has no table form of
verification, so ecdsa_verify_base too is set against the host's full verify (its row says so).  Exits
non-zero if ec_mul is slower than lincomb(m = 1) or the device is slower than that one core, at either count.

    python tools/probe_ecdsa.py [--reps 5] [--window 0.25] [--out profiles/probe_ecdsa.json]
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
#include <vector>
#include "scl_hip/util/sha256.h"
#include "scl_hip/util/sign.h"
using namespace scl;
using EC = math::EC<math::ec::Secp256k1>;
using FF = EC::ScalarField;
int main() {
  auto prg = util::PRG::create("probe-ecdsa");
  const int sample = 24;
  double mul = 0, bit = 0, sign = 0, verify = 0;
  namespace secp = sclhip::secp;
  bool all = true;
  for (int i = 0; i < sample; ++i) {
    const FF sk = FF::random(prg), k = FF::random(prg);
    const EC pk = util::ECDSA::derive(sk);
    const auto digest = util::Sha256{}.update(std::vector<unsigned char>(40, (unsigned char)i)).finalize();
    std::uint64_t p[secp::POINT_LIMBS], table[secp::MUL_TABLE_ENTRIES * secp::POINT_LIMBS];
    sclhip::U256 kl;
    pk.toLimbs(p);
    k.toLimbs(kl.w);
    auto tb = std::chrono::steady_clock::now();
    const EC slow = k * pk;  // EC::operator*: the 1-bit chain
    auto t0 = std::chrono::steady_clock::now();
    secp::pt_store(p, secp::pt_mul_window(secp::pt_load(p), secp::scalar_plain(kl), table, secp::POINT_LIMBS));
    auto t1 = std::chrono::steady_clock::now();
    all = all && EC::fromLimbs(p) == slow && !slow.isPointAtInfinity();
    bit += std::chrono::duration<double>(t0 - tb).count();
    const auto sig = util::ECDSA::Sign(sk, digest, prg);
    auto t2 = std::chrono::steady_clock::now();
    all = all && util::ECDSA::verify(pk, sig, digest);
    auto t3 = std::chrono::steady_clock::now();
    mul += std::chrono::duration<double>(t1 - t0).count();
    sign += std::chrono::duration<double>(t2 - t1).count();
    verify += std::chrono::duration<double>(t3 - t2).count();
  }
  std::printf("{\"ok\":%s,\"mul_s\":%.9f,\"mul_bit_ladder_s\":%.9f,\"sign_s\":%.9f,\"verify_s\":%.9f}\n", all ? "true" : "false",
              mul / sample, bit / sample, sign / sample, verify / sample);
  return all ? 0 : 1;
}
"""


def host_seconds_per_signature():
    """the mirror on one core: seconds per multiplication (window ladder, and the 1-bit chain), signature and verification"""
    build = os.path.join(ROOT, "tools", "_build")
    os.makedirs(build, exist_ok=True)
    src, exe = os.path.join(build, "probe_ecdsa_host.cc"), os.path.join(build, "probe_ecdsa_host")
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    if not os.path.exists(src) or open(src).read() != HOST:
        with open(src, "w") as fh:
            fh.write(HOST)
    newest = max(os.path.getmtime(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(newest, os.path.getmtime(src)):  # (minutes: the mirror's headers)
        subprocess.run(["g++", "-std=c++20", "-O2", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src, f"-L{lib}", "-lscl_hip",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--counts", type=int, nargs="+", default=[10 ** 5, 10 ** 6])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_ecdsa.json"))
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

    host = host_seconds_per_signature()
    f = scl.SECP256K1_SCALAR
    gtable = scl.ec_base_table()
    rows = []
    for n in args.counts:
        sk, nonces = scl.vector_random(f, n, b"probe-ecdsa-sk"), scl.vector_random(f, n, b"probe-ecdsa-k")
        pk = scl.ec_mul_base(gtable, sk)
        digests = scl.sha256(scl.prg_blocks(2 * n, b"probe-ecdsa-msg").reshape(n, 32))
        scratch, pts = scl.ec_mul_scratch(n), scl.ec_empty(n)
        sig = torch.empty(n, 8, dtype=torch.int64, device="cuda")
        ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        ms_mul = timed(lambda: scl.ec_mul(pk, nonces, scratch=scratch, out=pts))
        ms_lin = timed(lambda: scl.ec_lincomb(pk.reshape(1, n, 12), nonces[:1], out=pts))
        ms_sign = timed(lambda: scl.ecdsa_sign(gtable, sk, nonces, digests, out=sig))
        ms_verify = timed(lambda: scl.ecdsa_verify(gtable, pk, sig, digests, scratch=scratch, out=ok))
        assert bool((ok == 1).all())
        # one signer: every signature under key 0
        scl.ecdsa_sign(gtable, sk[:1], nonces, digests, out=sig)
        qtable = scl.ec_base_table(scl.to_host(pk[:1])[0])
        ms_base = timed(lambda: scl.ecdsa_verify_base(gtable, qtable, sig, digests, out=ok))
        assert bool((ok == 1).all())
        for what, ms, host_s in (("ec_mul", ms_mul, host["mul_s"]), ("ec_lincomb_m1", ms_lin, host["mul_bit_ladder_s"]), ("ecdsa_sign", ms_sign, host["sign_s"]),
                                 ("ecdsa_verify", ms_verify, host["verify_s"]), ("ecdsa_verify_base", ms_base, host["verify_s"])):
            ms, fastest, slowest, calls = ms
            rows.append({"call": what, "n": n, "ms": round(ms, 4), "ms_fastest_window": round(fastest, 4), "ms_slowest_window": round(slowest, 4),
                         "calls_per_window": calls, "per_s": round(n / (ms * 1e-3), 1), "host_one_core_s": round(host_s * n, 4),
                         "speedup_vs_one_core": round(host_s * n / (ms * 1e-3), 1),
                         "host_form": {"ec_mul": "pt_mul_window", "ec_lincomb_m1": "EC::operator* (1-bit chain)", "ecdsa_sign": "ECDSA::Sign",
                                       "ecdsa_verify": "ECDSA::verify", "ecdsa_verify_base": "ECDSA::verify (no table form on the host)"}[what]})
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"tool": "tools/probe_ecdsa.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "window_s": args.window,
                   "host_seconds_per_signature": host, "rows": rows}, fh, indent=1)
    by = {(r["call"], r["n"]): r for r in rows}
    bad = [r for r in rows if r["speedup_vs_one_core"] < 1.0]
    bad += [by[("ec_mul", n)] for n in args.counts if by[("ec_mul", n)]["ms"] > by[("ec_lincomb_m1", n)]["ms"]]
    if bad:
        sys.exit(f"slower than the host mirror on one core, or ec_mul slower than lincomb(m = 1): {bad}")


if __name__ == "__main__":
    main()
