"""Beaver multiplication, the host half: detail/beaver.hpp's per-element functions against the fields' own reduced operations
(tests/cxx/beaver_host_check.cc, plain and under the address and undefined-behaviour sanitizers, as a stand-alone program), and
the build of the C++ mirror's round trips (tests/cxx/test_beaver_api.cc), which tests/test_gpu_beaver.py runs."""
import extremes as X
from cxx_support import SANITIZE, host_check, mirror_binary, needed

RINGS = [str(k) for k in X.RING_BITS]


def beaver_check(tmp_path, name, flags):
    return host_check(tmp_path, "beaver_host_check.cc", name, ("-w",) + tuple(flags), args=RINGS, want=(" 0 mismatches", f"{len(RINGS)} rings"))


def test_finish_one_equals_the_reduced_operations(tmp_path):
    """every field struct and the ring widths of extremes.RING_BITS: the two-product, one-fold form == mul / add one at a time,
    at the extreme operands crossed over the five positions and at 10^5 uniform tuples per field, both values of add_ed"""
    beaver_check(tmp_path, "beaver_host_check", ("-O2",))


def test_finish_one_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift, no overflow it does not mean"""
    assert "runtime error" not in beaver_check(tmp_path, "beaver_host_check_san", SANITIZE)


def test_the_mirror_test_compiles():
    """tests/cxx/test_beaver_api.cc builds against include/scl_hip/hip/beaver.h and links both libraries (it runs on the GPU:
    tests/test_gpu_beaver.py)"""
    dynamic = needed(mirror_binary("beaver"))
    assert "libscl_hip_mpc.so" in dynamic and "libscl_hip.so" in dynamic
