"""Beaver multiplication, the host half: detail/beaver.hpp's per-element functions against the fields' own reduced operations
(tests/cxx/beaver_host_check.cc, plain and under the address and undefined-behaviour sanitizers, as a stand-alone program), and
the helper that compiles the C++ mirror's round trips (tests/cxx/test_beaver_api.cc), which tests/test_gpu_beaver.py runs."""
import os
import subprocess

import extremes as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
RINGS = [str(k) for k in X.RING_BITS]


def beaver_binary():
    """tests/cxx/test_beaver_api.cc compiled against the mirror and both libraries (build() leaves it in place; rebuilt here
    when stale)"""
    src, exe = os.path.join(CXX, "test_beaver_api.cc"), os.path.join(CXX, "_build", "test_beaver_api")
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    newest = max(os.path.getmtime(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(newest, os.path.getmtime(src)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{lib}", "-lscl_hip_mpc", "-lscl_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def host_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++20", "-w", f"-I{ROOT}/include", *flags, "-o", exe, os.path.join(CXX, "beaver_host_check.cc")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, *RINGS], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout and f"{len(RINGS)} rings" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_finish_one_equals_the_reduced_operations(tmp_path):
    """every field struct and the ring widths of extremes.RING_BITS: the two-product, one-fold form == mul / add one at a time,
    at the extreme operands crossed over the five positions and at 10^5 uniform tuples per field, both values of add_ed"""
    host_check(tmp_path, "beaver_host_check", ["-O2"])


def test_finish_one_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    out = host_check(tmp_path, "beaver_host_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out


def test_the_mirror_test_compiles():
    """tests/cxx/test_beaver_api.cc builds against include/scl_hip/hip/beaver.h and links both libraries (it runs on the GPU:
    tests/test_gpu_beaver.py)"""
    exe = beaver_binary()
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip_mpc.so" in needed and "libscl_hip.so" in needed
