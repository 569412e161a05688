"""csrc/launch_rules.hpp checked on the CPU through its stand-alone host program, tests/cxx/launch_rules_check.cc: grid_cap against
the four grid rules of capi.hip it replaced, mfma_shape against the expression the matrix-core dispatchers repeated, dispatch_int /
dispatch_of on every value and on the misses around them, residency_pad at the launchers' triples -- once plain and once under
-fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")


def rules_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(CXX, "launch_rules_check.cc")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    return r.stdout + r.stderr


def test_the_launch_rules_against_the_formulas_they_replaced(tmp_path):
    rules_check(tmp_path, "launch_rules_check", ["-O2"])


def test_the_launch_rules_under_the_sanitizers(tmp_path):
    """the same stand-alone host program under -fsanitize=address,undefined: no overflow it does not mean"""
    out = rules_check(tmp_path, "launch_rules_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out and "AddressSanitizer" not in out
