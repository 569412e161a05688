"""Exact comparison, the host half.  The reference has no comparison: the yardstick of the device tests is the Python-integer model
of tests/cmp_support.py, so the model is pinned here first -- its tree equals Python's c' < r' for every pair at w = 1..5 and for
seeded pairs at every width at which a tree shape with a lone node appears; its counts equal the loop that defines them; its
mod2m, trunc and ltz equal x % 2^w, x >> w and x < 0 at the corners of x and of the comparison --, then the host forms of
detail/cmp.hpp (tests/cxx/cmp_host_check.cc) are held against vectors the model writes, over all five prime fields -- Mont128 at
2^128 - 159 and at 2^127 - 1 --, plain and as a stand-alone program under the address and undefined-behaviour sanitizers.
Everything is exact."""
import subprocess

import numpy as np

import cmp_support as CS
import fx_support as FXS
from cxx_support import SANITIZE, host_check, needed

P61 = 2 ** 61 - 1


def test_the_models_tree_is_less_than_for_every_pair_at_small_widths():
    for w in range(1, 6):
        pairs = [(c, r) for c in range(1 << w) for r in range(1 << w)]
        cmod = np.array([c for c, _ in pairs], dtype=object)
        bits = [[(r >> i) & 1 for _, r in pairs] for i in range(w)]
        assert CS.model_bit_lt(P61, cmod, bits, w).tolist() == [int(c < r) for c, r in pairs], w


def test_the_models_tree_is_less_than_at_every_tree_shape():
    """seeded pairs, and pairs that differ in one bit only or not at all, at every w in 1..17 and at 59, 63, 64, 65, 125, 127, 128,
    129, 254: every tree shape with a lone node at some level; the prime is one the width fits (the tree works on 0 / 1)"""
    assert set(range(1, 18)) | {59, 63, 64, 65, 125, 127, 128, 129, 254} == set(CS.WIDTHS)
    shapes = set()
    for w in CS.WIDTHS:
        p = FXS.SECP_P if w > 59 else P61
        cs = [v % (1 << w) for v in FXS.seeded(1 << 256, 24, 300 + w)]
        rs = [v % (1 << w) for v in FXS.seeded(1 << 256, 24, 600 + w)]
        for i in range(8):                                               # equal, and one bit apart at a seeded position
            rs[i] = cs[i] ^ ((1 << (cs[i + 8] % w)) if i % 4 else 0)
        cs += [0, (1 << w) - 1, 0, (1 << w) - 1]
        rs += [0, (1 << w) - 1, (1 << w) - 1, 0]
        got = CS.model_bit_lt(p, np.array(cs, dtype=object), [[(r >> i) & 1 for r in rs] for i in range(w)], w)
        assert got.tolist() == [int(c < r) for c, r in zip(cs, rs)], w
        shapes.add(tuple(c % 2 for c in CS.level_counts(w)))
    assert len(shapes) >= 12


def test_levels_and_planes_are_the_loop_that_defines_them():
    for w in range(1, 300):
        cnt, levels, planes = w, 0, 0
        while True:
            cnt, levels = (cnt + 1) // 2, levels + 1
            if cnt == 1:
                planes += 1
                break
            planes += 2 * cnt
        assert (CS.model_levels(w), CS.model_planes(w)) == (levels, planes), w
        assert levels == max(1, (w - 1).bit_length())
    assert CS.model_planes(59) == 119 and CS.model_levels(59) == 6


def corner_cases(p, k, w, B, seed):
    """(x, bits): the corners of x under r' = 0, r' = 2^w - 1 and seeded low bits (x = 0 and x = -2^(k-1) are c' == r')"""
    out = []
    for kind in ("zero", "ones", "any"):
        for x in [-(1 << (k - 1)), -1, 0, 1, (1 << (k - 1)) - 1] + [v % (1 << k) - (1 << (k - 1)) for v in FXS.seeded(p, 3, seed)]:
            out.append((x, CS.corner_bits(w, B, kind, seed + len(out))))
    return out


def test_the_models_pipelines_are_mod_shift_and_sign():
    """mod2m, trunc and ltz of the model equal x % 2^w, x >> w and x < 0: x in {-2^(k-1), -1, 0, 1, 2^(k-1) - 1} and seeded, with
    c' == r', r' = 0 and r' = 2^w - 1 among the cases (checked), at the smallest and the largest shape of every field and w on both
    sides of a limb boundary"""
    for n, (name, f, mp) in enumerate(FXS.CASES):
        p = FXS.prime(f, mp)
        top = FXS.max_bits(p)
        shapes = [(2, 1, 2), (3, 2, 4), (top, top - 1, top), (top // 2, 5, top - 3)] + ([(top, 64, top), (70, 63, 80)] if top > 70 else [])
        for j, (k, w, B) in enumerate(shapes):
            cases = corner_cases(p, k, w, B, 1000 * n + 50 * j)
            x = np.array([v % p for v, _ in cases], dtype=object)
            bits = np.array([b for _, b in cases], dtype=object).T
            hit = set()
            for what, want in ((CS.MOD, lambda v: v % (1 << w)), (CS.TRUNC, lambda v: (v >> w) % p), (CS.LTZ, None)):
                if what == CS.LTZ and w != k - 1:
                    continue
                y, cmod, rlow = CS.model_pipeline(p, x, bits, k, w, what)
                assert y.tolist() == [int(v < 0) if what == CS.LTZ else want(v) for v, _ in cases], (name, k, w, B, what)
                hit |= {"eq" for c, r in zip(cmod, rlow) if c == r} | {"zero" for r in rlow if r == 0} | {"ones" for r in rlow if r == (1 << w) - 1}
            assert hit == {"eq", "zero", "ones"}, (name, k, w, B, hit)


def lines():
    """the cases file of cmp_host_check: the counts; per field the first level's pairs at widths on both sides of every limb
    boundary -- shares that are seeded elements, p - 1, 0 and 1; the opened value in range, at 2^(B+1) and p - 1 --, levels with and
    without a partner, and the finish in its three forms with the status set and clear"""
    out = [f"count {w} {CS.model_levels(w)} {CS.model_planes(w)}" for w in CS.WIDTHS + [2, 100, 200]]
    hx = lambda *vs: " ".join(f"{int(v):x}" for v in vs)
    for n, (name, f, mp) in enumerate(FXS.CASES):
        p = FXS.prime(f, mp)
        top = FXS.max_bits(p)
        ws = sorted({1, 2, 3, 5, top - 1} | {w for w in (63, 64, 65, 127, 128, 129, 191, 192, 193) if w < top})
        for i, w in enumerate(ws):
            B = min(top, w + 3)
            seed = 2000 * n + 20 * i
            for jj, opened in enumerate([FXS.seeded(p, 1, seed)[0] % (1 << (B + 1)), (1 << (B + 1)) - 1, 1 << (B + 1), p - 1]):
                cmod, status = CS.a_open_col(np.array([opened], dtype=object), w, B)
                for j in sorted({0, (w - 1) // 2, ((w + 1) // 2) // 2}):
                    has_hi = 2 * j + 1 < w
                    b = np.array([p - 1, p - 1, p - 1, p - 1] if jj == 1 else FXS.seeded(p, 4, seed + 3 + j) if jj != 3 else [0, 1, 1, 0], dtype=object).reshape(4, 1, 1)
                    planes = np.zeros((w, 1, 1), dtype=object)
                    planes[2 * j] = b[0]
                    if has_hi:
                        planes[2 * j + 1] = b[1]
                    r2 = np.zeros((2 * ((w + 1) // 2), 1, 1), dtype=object)
                    r2[2 * j], r2[2 * j + 1] = b[2], b[3]
                    d = CS.a_first(p, cmod, planes, r2, w)
                    out.append(f"pair {name} {w} {B} {hx(opened, cmod[0])} {status[0]} {j} {int(has_hi)} {hx(b[0, 0, 0], b[1, 0, 0], b[2, 0, 0], b[3, 0, 0], d[2 * j, 0, 0], d[2 * j + 1, 0, 0])}")
            for what in (CS.MOD, CS.TRUNC, CS.LTZ):
                for st in (0, 1):
                    v = np.array(FXS.seeded(p, 5, seed + 9 + what) if st == 0 and i % 2 else [p - 1] * 5, dtype=object)
                    v[0] %= 1 << w
                    y = CS.a_finish(p, v[1:2, None], v[0:1], np.array([st]), v[2:3, None], v[3:4, None], w, what)
                    out.append(f"finish {name} {w} {what} {hx(v[0])} {st} {hx(v[1], v[2], v[3], y[0, 0])}")
        for i, vals in enumerate([FXS.seeded(p, 6, 77 + n), [p - 1] * 6, FXS.seeded(p, 6, 78 + n), [p - 1] * 6, [0, 1, 1, 0, 0, 0]]):
            has_hi = i < 2 or i == 4
            nodes = np.array(vals[:4] if has_hi else vals[:2], dtype=object).reshape(-1, 1, 1)
            d = CS.a_level(p, nodes, np.array(vals[4:], dtype=object).reshape(2, 1, 1))
            out.append(f"level {name} {int(has_hi)} {hx(*vals)} {hx(d[0, 0, 0], d[1, 0, 0])}")
    return out


def test_the_host_forms_equal_the_model(tmp_path):
    """cmp_levels, cmp_planes, cmp_open_col, cmp_leaf, cmp_combine_lt, cmp_combine_eq, cmp_make_finish and cmp_finish_one of
    detail/cmp.hpp, every prime field, both Mont128 moduli"""
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines()) + "\n")
    host_check(tmp_path, "cmp_host_check.cc", "cmp_host_check", ("-w", "-O2"), args=(str(cases),))


def test_the_host_forms_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined, nothing preloaded: no out-of-range shift in the bit masks or
    the rotations, no read past the limbs"""
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines()) + "\n")
    assert "runtime error" not in host_check(tmp_path, "cmp_host_check.cc", "cmp_host_check_san", ("-w",) + SANITIZE, args=(str(cases),))


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_mirrors_host_forms():
    """tests/cxx/test_cmp_api.cc --host: ss::bitLtLeaves, ss::combine, ss::mod2m, ss::truncExact and ss::ltz over the five prime
    fields -- shares of x and of true bits, masked, opened, compared level by level and finished, reconstruct x mod 2^w,
    floor(x / 2^w) and [x < 0] exactly"""
    exe = CS.cmp_api_binary()
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    dynamic = needed(exe)
    assert "libscl_hip_cmp.so" in dynamic and "libscl_hip.so" in dynamic
