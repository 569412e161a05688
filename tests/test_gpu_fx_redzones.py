"""Red-zone tests for the fixed-point extension: no scl_fx_* call writes outside its output windows.

tests/test_gpu_rb_redzones.py pins where the entry points of include/scl_hip_rb.h write; this file does it for
include/scl_hip_fx.h, through the raw C ABI with pointers into a tests/redzone.py arena.  out, c, rlow and y are rows x N elements
at a pitch larger than N (N + 1 and N + 3 among them, the inputs then at N), so the gaps between their rows are flanks: exactly N elements per row
stride are written; the status bytes are an `out` window of exactly N bytes.  The planes, x, csh and (for the finish) rlow are `in`
windows: unchanged.  One-limb windows start 0 and 8 bytes past a 16-byte boundary with even and odd pitches (one and two columns
per lane, and the misaligned pair phase); wider ones 0, 16 and 48 bytes past a 128-byte line; the status window starts at every
byte phase in turn.  N in {1, 2, 3, 65, 257}, rows 1 and 3.  Each case asserts the return code, arena.check() and the values (the
model's).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that takes
a `_dev` pointer has none."""
import numpy as np
import pytest

import fx_support as FXS
import oracle_lib as O
import redzone as R
from abi_support import device_entry_points
from gpu_support import el, fname, gpu_env, mat, placements, settle

FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 65, 257]
ROWS = [1, 3]


def shape_of(f, k):
    """(B, k, shift), small ones in turn: where a call writes does not depend on them, and the planes must fit the arena"""
    return ((5, 4, 2), (24, 20, 9))[k % 2]


def planes_window(A, f, planes, N, pitch, align, phase):
    """the planes [B][rows][N] as ONE `in` window of B * rows rows: plane i of row r is its row r * B + i (plane_stride = pitch,
    row_stride = B * pitch)"""
    B, rows = planes.shape[:2]
    data = FXS.limbs_of(f, np.ascontiguousarray(planes.transpose(1, 0, 2)).reshape(rows * B, N))
    return mat(A, "bits", f, rows * B, N, pitch, align, phase, "in", data)


def cases(f):
    for k, N in enumerate(NS):
        for rows in ROWS:
            tight = [(16, 8 * (k % 2), N)] if O.LIMBS[f] == 1 else [(128, 16, N)]      # inputs at a pitch of N: outputs at N + 1 and N + 3
            for j, (align, phase, pitch) in enumerate(placements(f, N, k + rows) + tight):
                yield k, N, rows, j, align, phase, pitch


def run_compose(env, f):
    scl, fx, port = env
    p = FXS.prime(f)
    for k, N, rows, j, align, phase, pitch in cases(f):
        B = shape_of(f, k + j)[0]
        note = f"compose {fname(f)} N={N} rows={rows} B={B} pitch={pitch} phase={phase}"
        planes = FXS.uniform(p, (B, rows, N), 7000 + 10 * k + rows)
        A = R.Arena()
        wb = planes_window(A, f, planes, N, pitch, align, phase)
        wo = mat(A, "out", f, rows, N, pitch + 1, align, phase)
        rc = fx.lib.scl_fx_compose(f, wo.ptr, pitch + 1, wb.ptr, pitch, B * pitch, B, rows, N, None)
        settle(fx.lib.scl_fx_last_error, A, rc, note)
        assert (FXS.ints_of(f, el(wo, f)) == FXS.a_compose(p, planes)).all(), note


def run_mask(env, f):
    scl, fx, port = env
    p = FXS.prime(f)
    for k, N, rows, j, align, phase, pitch in cases(f):
        B, kk, shift = shape_of(f, k + j)
        note = f"trunc_mask {fname(f)} N={N} rows={rows} (B, k, shift)=({B}, {kk}, {shift}) pitch={pitch} phase={phase}"
        planes, x = FXS.uniform(p, (B, rows, N), 7100 + 10 * k + rows), FXS.uniform(p, (rows, N), 7200 + 10 * k + rows)
        A = R.Arena()
        wb = planes_window(A, f, planes, N, pitch, align, phase)
        wx = mat(A, "x", f, rows, N, pitch, align, phase, "in", FXS.limbs_of(f, x))
        wc = mat(A, "c", f, rows, N, pitch + 1, align, phase)
        wl = mat(A, "rlow", f, rows, N, pitch + 3, align, phase)
        rc = fx.lib.scl_fx_trunc_mask(f, wc.ptr, pitch + 1, wl.ptr, pitch + 3, wx.ptr, pitch, wb.ptr, pitch, B * pitch, kk, shift, B, rows, N, None)
        settle(fx.lib.scl_fx_last_error, A, rc, note)
        c, rlow = FXS.a_mask(p, x, planes, kk, shift)
        assert (FXS.ints_of(f, el(wc, f)) == c).all() and (FXS.ints_of(f, el(wl, f)) == rlow).all(), note


def run_finish(env, f):
    scl, fx, port = env
    p = FXS.prime(f)
    for k, N, rows, j, align, phase, pitch in cases(f):
        B, _, shift = shape_of(f, k + j)
        m = (1, 3, 4)[(k + j) % 3]
        note = f"trunc_finish {fname(f)} N={N} rows={rows} (B, shift)=({B}, {shift}) m={m} pitch={pitch} phase={phase}"
        x, rlow = FXS.uniform(p, (rows, N), 7300 + 10 * k + rows), FXS.uniform(p, (rows, N), 7400 + 10 * k + rows)
        c = FXS.uniform(p, (N,), 7500 + 10 * k + rows) % (1 << (B + 1))
        c[N // 2] = 1 << (B + 1)                                                  # a flagged column
        lam = FXS.limbs_of(f, np.array(FXS.lagrange_at_zero(p, m), dtype=object))
        A = R.Arena()
        ws = mat(A, "csh", f, m, N, pitch, align, phase, "in", FXS.limbs_of(f, FXS.a_share(p, c, m - 1, m, 7600 + k)))
        wx = mat(A, "x", f, rows, N, pitch, align, phase, "in", FXS.limbs_of(f, x))
        wl = mat(A, "rlow", f, rows, N, pitch + 1, align, phase, "in", FXS.limbs_of(f, rlow))
        wy = mat(A, "y", f, rows, N, pitch + 3, align, phase)
        wst = A.window("status", N, 16, (3 * k + 7 * j + rows) % 16, kind="out")
        rc = fx.lib.scl_fx_trunc_finish(f, wy.ptr, pitch + 3, wst.ptr, ws.ptr, pitch, lam.ctypes.data, m, wx.ptr, pitch, wl.ptr, pitch + 1, shift, B,
                                        rows, N, None)
        settle(fx.lib.scl_fx_last_error, A, rc, note)
        y, status = FXS.a_finish(p, c, x, rlow, shift, B)
        assert (FXS.ints_of(f, el(wy, f)) == y).all() and wst.read().reshape(-1).tolist() == status.tolist() and status[N // 2] == 1, note


TABLE = {"scl_fx_compose": run_compose, "scl_fx_trunc_mask": run_mask, "scl_fx_trunc_finish": run_finish}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("fx")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(FXS.FX)
    assert len(names) == 3 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_fx_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
