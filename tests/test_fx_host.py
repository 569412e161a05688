"""Probabilistic truncation, the host half: the Python model (tests/fx_support.py) held against the exact form of the issue --
y = floor((x + 2^(k-1)) / 2^shift) + carry - 2^(k-1-shift) -- inside the test of the host forms (alone it would say nothing about
the library), and the stand-alone check of the host forms of detail/fx.hpp (tests/cxx/fx_host_check.cc) over all five prime
fields -- Mont128 at 2^128 - 159 and at 2^127 - 1 -- against the model and the identities, plain and under the address and
undefined-behaviour sanitizers.  Everything is exact.  The reference has no truncation: there is no fixture from it."""
import subprocess

import fx_support as FXS
from cxx_support import SANITIZE, host_check, needed


def model_self_check(name, f, mp):
    """the model against the exact form, before the host forms are held against it: at every shape of the field, the extremes of
    x and seeded values, all-zero, all-one and seeded bits -- mask, open, finish gives exact_trunc and status 0"""
    p = FXS.prime(f, mp)
    assert FXS.max_bits(p) == {"m61": 59, "m127": 125, "mont128_p0": 126, "mont128_p1": 125, "secp_scalar": 254, "secp_field": 254}[name]
    for j, (B, k, shift) in enumerate(FXS.shapes(p) + [(3, 3, 2)]):
        xs = [-(1 << (k - 1)), (1 << (k - 1)) - 1, 0, -1] + [v % (1 << k) - (1 << (k - 1)) for v in FXS.seeded(p, 4, 10 + j)]
        for i, bits in enumerate([[0] * B, [1] * B, FXS.seeded_bits(B, 20 + j)]):
            x = [v % p for v in xs]
            c, rlow = FXS.model_mask(p, x, [[b] * len(x) for b in bits], k, shift)
            assert all(v < 1 << (B + 1) for v in c), (name, B, k, shift)
            y, status = FXS.model_finish(p, c, [x], [rlow], shift, B)
            assert status == [0] * len(x) and y[0] == [FXS.exact_trunc(p, v, bits, k, shift) for v in x], (name, B, k, shift, i)


def lines():
    """the cases file of fx_host_check: per field and shape -- planes of true bits with the extremes of x, planes that are seeded
    elements, planes that are all p - 1; the value opened is the honest c, then 2^(B+1) - 1, 2^(B+1), p - 1 and a seeded element"""
    out = []
    for n, (name, f, mp) in enumerate(FXS.CASES):
        p = FXS.prime(f, mp)
        for j, (B, k, shift) in enumerate(FXS.shapes(p)):
            seed = 1000 * n + 10 * j
            sets = [[[b] for b in FXS.seeded_bits(B, seed)], [[v] for v in FXS.seeded(p, B, seed + 1)], [[p - 1]] * B, [[1]] * B]
            xs = [-(1 << (k - 1)) % p, (1 << (k - 1)) - 1, FXS.seeded(p, 1, seed + 2)[0], p - 1]
            for planes, x in zip(sets, xs):
                (c,), (rlow,) = FXS.model_mask(p, [x], planes, k, shift)
                for opened in (c, (1 << (B + 1)) - 1, 1 << (B + 1), p - 1, FXS.seeded(p, 1, seed + 3)[0]):
                    (y,), (status,) = FXS.model_finish(p, [opened], [[x]], [[rlow]], shift, B)
                    (y,) = y
                    out.append(" ".join([name, str(B), str(k), str(shift)] + [f"{v:x}" for v in (x, c, rlow, opened, y)] + [str(status)] +
                                        [f"{pl[0]:x}" for pl in planes]))
    return out


def test_the_host_forms_equal_the_model_and_the_identities(tmp_path):
    """fx_step, fx_canon, fx_mask_one, fx_finish_col, fx_finish_one and the constants of detail/fx.hpp, every prime field, both
    Mont128 moduli; the model they are held against is checked against the exact form first (model_self_check)"""
    for case in FXS.CASES:
        model_self_check(*case)
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines()) + "\n")
    host_check(tmp_path, "fx_host_check.cc", "fx_host_check", ("-w", "-O2"), args=(str(cases),))


def test_the_host_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: no out-of-range shift in the masks or the rotation, no read
    past the planes"""
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines()) + "\n")
    assert "runtime error" not in host_check(tmp_path, "fx_host_check.cc", "fx_host_check_san", ("-w",) + SANITIZE, args=(str(cases),))


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_mirrors_host_forms():
    """tests/cxx/test_fx_api.cc --host: ss::composeBits, ss::truncMask and ss::truncFinish over the five prime fields -- shares of
    x and of true bits, masked, opened and finished, reconstruct floor(x / 2^shift) or that plus one"""
    exe = FXS.fx_api_binary()
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    dynamic = needed(exe)
    assert "libscl_hip_fx.so" in dynamic and "libscl_hip.so" in dynamic
