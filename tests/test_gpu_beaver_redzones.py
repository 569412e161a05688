"""Red-zone tests for the protocol extension: neither scl_mpc_* entry point writes outside its output windows.

tests/test_gpu_redzones.py pins WHERE every entry point of include/scl_hip.h writes; this file does the same for
include/scl_hip_mpc.h, through the raw C ABI with pointers into a tests/redzone.py arena.  Operands are `in` windows (a changed
input byte is caught), outputs `out` windows, the in-place operand of the finish an `inout` window.  Every output window has
rows in {1, 3} (the mask's output twice as many) at a pitch larger than N, so the gaps between rows are flanks too.  One-limb
windows start 0 and 8 bytes past a 16-byte boundary with even and odd pitches (phase 0 with an even pitch is the two-per-lane
body with its one-element tail at odd N; everything else the one-per-lane form); wider ones 0, 16 and 48 bytes past a 128-byte
line.  N in {1, 2, 3, 64, 257}: one element, one pair, a pair and a tail, a wavefront, a block and one.  Each case asserts the
return code, arena.check() and the values (the oracle's: beaver_reference of tests/gpu_support.py, shared with tests/test_gpu_beaver.py).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that
takes a `_dev` pointer has none."""
import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from abi_support import MPC, device_entry_points
from gpu_support import beaver_reference as reference
from gpu_support import el, fname, gpu_env, mat, placements, settle

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD, O.Z2K(62), O.Z2K(128)]
NS = [1, 2, 3, 64, 257]
ROWS = [1, 3]


def run_mask(env, f):
    scl, mpc, port = env
    r = reference(port, f)
    for k, N in enumerate(NS):
        for rows in ROWS:
            for align, phase, pitch in placements(f, N, k + rows):
                note = f"beaver_mask {fname(f)} N={N} rows={rows} pitch={pitch} phase={phase}"
                A = R.Arena()
                wx, wy, wa, wb = [mat(A, nm, f, rows, N, pitch, align, phase, "in", r[nm][:rows, :N]) for nm in ("x", "y", "a", "b")]
                wo = mat(A, "de", f, 2 * rows, N, pitch, align, phase, "out")
                rc = mpc.lib.scl_mpc_beaver_mask(f, wo.ptr, pitch, wx.ptr, wy.ptr, wa.ptr, wb.ptr, pitch, rows, N, None)
                settle(mpc.lib.scl_mpc_last_error, A, rc, note)
                got = el(wo, f)
                assert np.array_equal(got[:rows], r["mask_e"][:rows, :N]) and np.array_equal(got[rows:], r["mask_d"][:rows, :N]), note


def run_finish(env, f):
    scl, mpc, port = env
    r = reference(port, f)
    for k, N in enumerate(NS):
        for rows in ROWS:
            for i, (align, phase, pitch) in enumerate(placements(f, N, k + rows)):
                ed_rows = (0, 1, rows)[(k + i) % 3]
                inplace = (None, "a", "b", "c")[(k + rows + i) % 4]
                note = f"beaver_finish {fname(f)} N={N} rows={rows} pitch={pitch} phase={phase} ed_rows={ed_rows} in place: {inplace}"
                A = R.Arena()
                we, wd = [mat(A, nm, f, 1, N, N, align, phase, "in", r[nm][None, :N]) for nm in ("e", "d")]
                ops = {nm: mat(A, nm, f, rows, N, pitch, align, phase, "inout" if nm == inplace else "in", r[nm][:rows, :N])
                       for nm in ("a", "b", "c")}
                wz = ops[inplace] if inplace else mat(A, "z", f, rows, N, pitch, align, phase, "out")
                rc = mpc.lib.scl_mpc_beaver_finish(f, wz.ptr, pitch, we.ptr, wd.ptr, ops["a"].ptr, ops["b"].ptr, ops["c"].ptr, pitch, rows,
                                                   ed_rows, N, None)
                settle(mpc.lib.scl_mpc_last_error, A, rc, note)
                want = np.concatenate([r["z1"][:ed_rows, :N], r["z0"][ed_rows:rows, :N]])
                assert np.array_equal(el(wz, f), want), note


TABLE = {"scl_mpc_beaver_mask": run_mask, "scl_mpc_beaver_finish": run_finish}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("mpc")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(MPC)
    assert len(names) >= 2 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_mpc_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
