"""Red-zone tests for the comparison extension: no scl_cmp_* call writes outside its output windows.

tests/test_gpu_fx_redzones.py pins where the entry points of include/scl_hip_fx.h write; this file does it for
include/scl_hip_cmp.h, through the raw C ABI with pointers into a tests/redzone.py arena.  A node array d of P planes x rows x N
elements is ONE `out` window of rows * P rows at a pitch larger than N (N + 1 and N + 3 among them, the inputs then at N), so the
gaps between its planes are flanks: exactly N elements per plane and row are written -- under SCL_CMP_LT_ONLY the one plane 0; cmod
is an `out` window of exactly N elements, the status of exactly N bytes, out of the finish rows x N.  The planes, csh, r2, the
nodes, lt, rlow, x -- and for the finish cmod and the status -- are `in` windows: unchanged.  One-limb windows start 0 and 8 bytes
past a 16-byte boundary with even and odd pitches (one and two columns per lane, and the misaligned pair phase); wider ones 0, 16
and 48 bytes past a 128-byte line; the status window starts at every byte phase in turn.  N in {1, 2, 3, 65, 257}, rows 1 and 3.
Each case asserts the return code, arena.check() and the values (the model's).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that takes
a `_dev` pointer has none."""
import numpy as np
import pytest

import cmp_support as CS
import fx_support as FXS
import oracle_lib as O
import redzone as R
from abi_support import device_entry_points
from gpu_support import el, fname, gpu_env, mat, placements, settle

FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 65, 257]
ROWS = [1, 3]


def planes_window(A, name, f, planes, N, pitch, align, phase, kind="in"):
    """planes [P][rows][N] as ONE window of P * rows rows: plane q of row r is its row r * P + q (plane_stride = pitch,
    row_stride = P * pitch); `out`: the shape alone"""
    P, rows = planes.shape[:2]
    data = FXS.limbs_of(f, np.ascontiguousarray(planes.transpose(1, 0, 2)).reshape(rows * P, N)) if kind == "in" else None
    return mat(A, name, f, rows * P, N, pitch, align, phase, kind, data)


def planes_read(w, f, P, rows, N):
    """the window's elements as [P][rows][N] integers"""
    return FXS.ints_of(f, el(w, f)).reshape(rows, P, N).transpose(1, 0, 2)


def cases(f):
    for k, N in enumerate(NS):
        for rows in ROWS:
            tight = [(16, 8 * (k % 2), N)] if O.LIMBS[f] == 1 else [(128, 16, N)]      # inputs at a pitch of N: outputs at N + 1 and N + 3
            for j, (align, phase, pitch) in enumerate(placements(f, N, k + rows) + tight):
                yield k, N, rows, j, align, phase, pitch


def run_first(env, f):
    scl, cmp, port = env
    p = FXS.prime(f)
    for k, N, rows, j, align, phase, pitch in cases(f):
        w, B, m = ((5, 9), (2, 6), (1, 4), (8, 12))[(k + j) % 4] + ((1, 3, 4)[(k + j) % 3],)
        lt_only = w <= 2 and (k + rows) % 2 == 0
        P = 1 if lt_only else 2 * ((w + 1) // 2)
        note = f"first_mask {fname(f)} N={N} rows={rows} (w, B)=({w}, {B}) m={m} lt_only={lt_only} pitch={pitch} phase={phase}"
        bits, r2 = FXS.uniform(p, (w, rows, N), 8000 + 10 * k + rows), FXS.uniform(p, (P, rows, N), 8100 + 10 * k + rows)
        c = FXS.uniform(p, (N,), 8200 + 10 * k + rows) % (1 << (B + 1))
        c[N // 2] = 1 << (B + 1)                                                  # a flagged column
        lam = FXS.limbs_of(f, np.array(FXS.lagrange_at_zero(p, m), dtype=object))
        A = R.Arena()
        ws = mat(A, "csh", f, m, N, pitch, align, phase, "in", FXS.limbs_of(f, FXS.a_share(p, c, m - 1, m, 8300 + k)))
        wb = planes_window(A, "bits", f, bits, N, pitch, align, phase)
        wr = planes_window(A, "r2", f, r2, N, pitch, align, phase)
        wd = planes_window(A, "d", f, r2, N, pitch + 1 + 2 * (j % 2), align, phase, "out")
        wc = mat(A, "cmod", f, 1, N, N, align, phase)
        wst = A.window("status", N, 16, (3 * k + 7 * j + rows) % 16, kind="out")
        dp = pitch + 1 + 2 * (j % 2)
        rc = cmp.lib.scl_cmp_first_mask(f, wd.ptr, dp, P * dp, wc.ptr, wst.ptr, ws.ptr, pitch, lam.ctypes.data, m, wb.ptr, pitch, w * pitch, wr.ptr, pitch,
                                        P * pitch, w, B, rows, N, CS.LT_ONLY if lt_only else 0, None)
        settle(cmp.lib.scl_cmp_last_error, A, rc, note)
        cmod, status = CS.a_open_col(c.copy(), w, B)
        assert (FXS.ints_of(f, el(wc, f)).reshape(-1) == cmod).all() and wst.read().reshape(-1).tolist() == status.tolist() and status[N // 2] == 1, note
        assert (planes_read(wd, f, P, rows, N) == CS.a_first(p, cmod, bits, r2, w, lt_only)).all(), note


def run_level(env, f):
    scl, cmp, port = env
    p = FXS.prime(f)
    for k, N, rows, j, align, phase, pitch in cases(f):
        cnt = (2, 3, 7, 8)[(k + j) % 4]
        lt_only = cnt == 2 and (k + rows) % 2 == 0
        P = 1 if lt_only else 2 * ((cnt + 1) // 2)
        note = f"level_mask {fname(f)} N={N} rows={rows} cnt={cnt} lt_only={lt_only} pitch={pitch} phase={phase}"
        nodes, r2 = FXS.uniform(p, (2 * cnt, rows, N), 8400 + 10 * k + rows), FXS.uniform(p, (P, rows, N), 8500 + 10 * k + rows)
        A = R.Arena()
        wn = planes_window(A, "nodes", f, nodes, N, pitch, align, phase)
        wr = planes_window(A, "r2", f, r2, N, pitch, align, phase)
        dp = pitch + 1 + 2 * (j % 2)
        wd = planes_window(A, "d", f, r2, N, dp, align, phase, "out")
        rc = cmp.lib.scl_cmp_level_mask(f, wd.ptr, dp, P * dp, wn.ptr, pitch, 2 * cnt * pitch, wr.ptr, pitch, P * pitch, cnt, rows, N,
                                        CS.LT_ONLY if lt_only else 0, None)
        settle(cmp.lib.scl_cmp_last_error, A, rc, note)
        assert (planes_read(wd, f, P, rows, N) == CS.a_level(p, nodes, r2, lt_only)).all(), note


def run_finish(env, f):
    scl, cmp, port = env
    p = FXS.prime(f)
    for k, N, rows, j, align, phase, pitch in cases(f):
        w, what = (5, 2, 1, 8)[(k + j) % 4], (k + j + rows) % 3
        note = f"finish {fname(f)} N={N} rows={rows} w={w} what={what} pitch={pitch} phase={phase}"
        lt, rlow, x = (FXS.uniform(p, (rows, N), 8600 + 100 * i + 10 * k + rows) for i in range(3))
        cmod = FXS.uniform(p, (N,), 8900 + 10 * k + rows) % (1 << w)
        status = np.zeros(N, dtype=np.uint8)
        status[N // 2], cmod[N // 2] = 1, 0
        A = R.Arena()
        wt = mat(A, "lt", f, rows, N, pitch, align, phase, "in", FXS.limbs_of(f, lt))
        wl = mat(A, "rlow", f, rows, N, pitch + 1, align, phase, "in", FXS.limbs_of(f, rlow))
        wx = mat(A, "x", f, rows, N, pitch, align, phase, "in", FXS.limbs_of(f, x))
        wc = mat(A, "cmod", f, 1, N, N, align, phase, "in", FXS.limbs_of(f, cmod[None, :]))
        wst = A.window("status", N, 16, (3 * k + 7 * j + rows) % 16, kind="in")
        wst.load(status)
        wy = mat(A, "out", f, rows, N, pitch + 3, align, phase)
        rc = cmp.lib.scl_cmp_finish(f, wy.ptr, pitch + 3, wt.ptr, pitch, wc.ptr, wst.ptr, wl.ptr, pitch + 1, None if what == CS.MOD else wx.ptr, pitch, w, what,
                                    rows, N, None)
        settle(cmp.lib.scl_cmp_last_error, A, rc, note)
        assert (FXS.ints_of(f, el(wy, f)) == CS.a_finish(p, lt, cmod, status, rlow, x, w, what)).all(), note


TABLE = {"scl_cmp_first_mask": run_first, "scl_cmp_level_mask": run_level, "scl_cmp_finish": run_finish}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("cmp")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(CS.CMP)
    assert len(names) == 3 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_cmp_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
