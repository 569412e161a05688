"""The host side the translation units of csrc/ share (csrc/unit_host.hpp, csrc/aes_key_host.hpp), without a GPU: the PRG's
AES-128 key schedule -- the one piece of host code on which bit-exactness against the reference rests -- through the stand-alone
program tests/cxx/aes_key_check.hip: known answers of FIPS-197, the reference's seed rule (zero-padded or truncated to 16
bytes), and every round-key and table word through a T-table AES against the host AES of include/scl_hip/detail/aes_host.hpp.
The program makes no HIP runtime call; it is compiled by hipcc because it includes the kernels' header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "aes_key_check.hip")
HIPCC = "/opt/rocm/bin/hipcc"


def key_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-arch=gfx950", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    return r.stdout + r.stderr


def test_the_key_schedule_on_the_host(tmp_path):
    """FIPS-197 A.1, the seed rule, and agreement with the host AES at counters 0, 1 and 2^32 - 1 for every seed"""
    out = key_check(tmp_path, "aes_key_check", [])
    assert "aes_key_check: 24 checks, 0 mismatches" in out, out


def test_the_key_schedule_under_the_sanitizers(tmp_path):
    """the same stand-alone program with its host code under -fsanitize=address,undefined: no read past a short seed, no
    out-of-range shift"""
    out = key_check(tmp_path, "aes_key_check_san", ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                                    "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out and "AddressSanitizer" not in out, out
