"""Red-zone tests for the inner-product extension: no scl_ip_* call writes outside its output windows.

tests/test_gpu_redzones.py pins WHERE every entry point of include/scl_hip.h writes and tests/test_gpu_hm_redzones.py does the same
for include/scl_hip_hm.h; this file does it for include/scl_hip_ip.h, through the raw C ABI with pointers into a tests/redzone.py
arena.  Operands are rows at a pitch larger than N, so the gaps between rows are flanks too; the terms of scl_ip_dot_mask and the
batches of scl_ip_matmul_mask are windows of their own, so everything between two of them is a flank.  Operands are `in` windows,
the in-place forms `inout`.  One-limb windows start 0 and 8 bytes past a 16-byte boundary with even and odd pitches (phase 0 with
an even pitch is the two-per-lane body with the odd last element: the tail lane); wider ones 0, 16 and 48 bytes past a 128-byte
line.  N in {1, 2, 3, 64, 257}.  The matrix shapes are those of tests/test_gpu_ip.py with a clamped tile edge on both axes for
every field -- (5,7,3) and (3,2,5) -- and the 1 x 1 route, at batch 1 and 2.  Each case asserts the return code, arena.check()
and the values (the model's).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that takes
a `_dev` pointer has none."""
import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from abi_support import IP, device_entry_points
from gpu_support import el, esz, fname, gpu_env, limbs, mat, placements, pool, settle
from port_models import model_dot_mask, model_matmul_mask

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 64, 257]


def stride_between(ws, f):
    """the distance in elements between the first two windows of a list (the term or batch stride), 0 for one window"""
    if len(ws) < 2:
        return 0
    d = ws[1].ptr - ws[0].ptr
    assert d % esz(f) == 0 and all(w.ptr - ws[0].ptr == i * d for i, w in enumerate(ws)), "the arena placed the windows unevenly"
    return d // esz(f)


def series(A, name, f, count, rows, N, pitch, align, phase, data):
    """`count` windows of rows x N elements, evenly spaced (every window reserves the same span and flanks)"""
    return [mat(A, "%s%d" % (name, i), f, rows, N, pitch, align, phase, "in", data[i]) for i in range(count)]


def run_dot(env, f):
    """terms 1, 3 and 65 (past Mersenne61's bound) x rows 1, 3: every term of x and of y is a window, the term strides are the
    distances between them; with r2, without it, and in place on r2"""
    scl, ip, port = env
    L = limbs(f)
    for k, N in enumerate(NS):
        for terms, rows in ((1, 1), (3, 3), (65, 1)):
            x, y = [pool(port, f, terms * rows * N, b"rz-dot-" + t).reshape(terms, rows, N, L) for t in (b"x", b"y")]
            r2 = pool(port, f, rows * N, b"rz-dot-r").reshape(rows, N, L)
            want = {True: model_dot_mask(port, f, x, y, r2), False: model_dot_mask(port, f, x, y)}
            for align, phase, pitch in placements(f, N, k + rows)[:: (2 if terms == 65 else 1)]:
                for mode in ("r2", "none", "in place"):
                    note = f"dot_mask {fname(f)} N={N} terms={terms} rows={rows} pitch={pitch} phase={phase} {mode}"
                    A = R.Arena(capacity=R.MAX_CAPACITY if terms == 65 else R.DEFAULT_CAPACITY)
                    wx = series(A, "x", f, terms, rows, N, pitch, align, phase, x)
                    wy = series(A, "y", f, terms, rows, N, pitch, align, phase, y)
                    wr = mat(A, "r2", f, rows, N, pitch, align, phase, "inout" if mode == "in place" else "in", r2)
                    wd = wr if mode == "in place" else mat(A, "d", f, rows, N, pitch + 2, align, phase)
                    rc = ip.lib.scl_ip_dot_mask(f, wd.ptr, pitch if mode == "in place" else pitch + 2, wx[0].ptr, stride_between(wx, f), wy[0].ptr,
                                                stride_between(wy, f), None if mode == "none" else wr.ptr, pitch, terms, rows, N, None)
                    settle(ip.lib.scl_ip_last_error, A, rc, note)
                    assert np.array_equal(el(wd, f), want[mode != "none"]), note


def run_matmul(env, f):
    """(5,7,3) and (3,2,5): a % TI != 0 and b % TL != 0 for every field's tile, so rows and columns past the edge are computed from
    clamped operands and must not be stored; (1,65,1): the inner-product route; batch 1 and 2, each batch of every operand a window
    of its own"""
    scl, ip, port = env
    L = limbs(f)
    ti, tl = ip.matmul_tile(f)
    shapes = ((5, 7, 3), (3, 2, 5), (1, 65, 1))
    assert any(a % ti for a, _, _ in shapes) and any(b % tl for _, _, b in shapes)
    for k, N in enumerate(NS):
        for a, K, b in shapes:
            for batch in (1, 2):
                X = pool(port, f, batch * a * K * N, b"rz-mm-x").reshape(batch, a, K, N, L)
                Y = pool(port, f, batch * K * b * N, b"rz-mm-y").reshape(batch, K, b, N, L)
                R2 = pool(port, f, batch * a * b * N, b"rz-mm-r").reshape(batch, a, b, N, L)
                want = {True: model_matmul_mask(port, f, X, Y, R2), False: model_matmul_mask(port, f, X, Y)}
                pl = placements(f, N, k + a)
                align, phase, pitch = pl[(k + batch + a) % len(pl)]
                for mode in ("r2", "none", "in place"):
                    note = f"matmul_mask {fname(f)} N={N} ({a},{K},{b}) batch={batch} pitch={pitch} phase={phase} {mode}"
                    A = R.Arena(capacity=R.MAX_CAPACITY)
                    flat = lambda M: M.reshape(batch, -1, N, L)
                    wx = series(A, "x", f, batch, a * K, N, pitch, align, phase, flat(X))
                    wy = series(A, "y", f, batch, K * b, N, pitch, align, phase, flat(Y))
                    if mode == "in place":
                        wr = [mat(A, "r2%d" % q, f, a * b, N, pitch, align, phase, "inout", flat(R2)[q]) for q in range(batch)]
                        wd = wr
                    else:
                        wr = series(A, "r2", f, batch, a * b, N, pitch, align, phase, flat(R2))
                        wd = [mat(A, "d%d" % q, f, a * b, N, pitch + 2, align, phase) for q in range(batch)]
                    dp = pitch if mode == "in place" else pitch + 2
                    rc = ip.lib.scl_ip_matmul_mask(f, wd[0].ptr, dp, stride_between(wd, f), wx[0].ptr, pitch, stride_between(wx, f), wy[0].ptr, pitch,
                                                   stride_between(wy, f), None if mode == "none" else wr[0].ptr, pitch, stride_between(wr, f), a, K, b,
                                                   batch, N, None)
                    settle(ip.lib.scl_ip_last_error, A, rc, note)
                    for q in range(batch):
                        assert np.array_equal(el(wd[q], f).reshape(a, b, N, L), want[mode != "none"][q]), f"{note}: batch {q}"


TABLE = {"scl_ip_dot_mask": run_dot, "scl_ip_matmul_mask": run_matmul}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("ip")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(IP)
    assert len(names) == 2 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_ip_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
