"""The host side the translation units of csrc/ share (csrc/unit_host.hpp, csrc/aes_key_host.hpp), without a GPU: the PRG's
AES-128 key schedule -- the one piece of host code on which bit-exactness against the reference rests -- through the stand-alone
program tests/cxx/aes_key_check.hip: known answers of FIPS-197, the reference's seed rule (zero-padded or truncated to 16
bytes), and every round-key and table word through a T-table AES against the host AES of include/scl_hip/detail/aes_host.hpp.
The program makes no HIP runtime call; it is compiled by hipcc because it includes the kernels' header."""
from cxx_support import SANITIZE_HIP_HOST, hip_host_check


def test_the_key_schedule_on_the_host(tmp_path):
    """FIPS-197 A.1, the seed rule, and agreement with the host AES at counters 0, 1 and 2^32 - 1 for every seed"""
    out = hip_host_check(tmp_path, "aes_key_check.hip", "aes_key_check")
    assert "aes_key_check: 24 checks, 0 mismatches" in out, out


def test_the_key_schedule_under_the_sanitizers(tmp_path):
    """the same stand-alone program with its host code under -fsanitize=address,undefined: no read past a short seed, no
    out-of-range shift"""
    out = hip_host_check(tmp_path, "aes_key_check.hip", "aes_key_check_san", SANITIZE_HIP_HOST)
    assert "runtime error" not in out and "AddressSanitizer" not in out, out
