"""Red-zone tests for the honest-majority extension: no scl_hm_* call writes outside its output windows.

tests/test_gpu_redzones.py pins WHERE every entry point of include/scl_hip.h writes, tests/test_gpu_beaver_redzones.py and
tests/test_gpu_prep_redzones.py do the same for the other two extension headers; this file does it for include/scl_hip_hm.h,
through the raw C ABI with pointers into a tests/redzone.py arena.  Share matrices are rows at a pitch larger than N, so the gaps
between rows are flanks too; the two-pass scratch is a window of exactly scl_hm_double_scratch_bytes, so its tail is a flank; the
batches of scl_hm_apply are windows of their own, so everything between two batches is a flank.  Operands are `in` windows, the
in-place forms `inout`.  One-limb windows start 0 and 8 bytes past a 16-byte boundary with even and odd pitches (phase 0 with an
even pitch is the two-per-lane body with the odd last element); wider ones 0, 16 and 48 bytes past a 128-byte line.
N in {1, 2, 3, 64, 257}.  Each case asserts the return code, arena.check() and the values (the model's).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that takes
a `_dev` pointer has none."""
import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from abi_support import HM, device_entry_points
from gpu_support import HM_SEED as SEED
from gpu_support import hm_reference as reference
from gpu_support import el, esz, fname, gpu_env, limbs, mat, placements, pool, settle
from port_models import model_apply, model_finish, model_him, model_mask, model_open

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 64, 257]


def run_double(env, f):
    """(4,1) as the field takes it (fused or two passes), then forced through two passes, and (9,4): the scratch is an `out` window
    of exactly the size the library names"""
    scl, hm, port = env
    for k, N in enumerate(NS):
        for n, t, flags in ((4, 1, 0), (4, 1, 1), (9, 4, 0)):
            want = reference(port, f, n, t)
            for align, phase, pitch in placements(f, N, k + n)[:: (2 if flags else 1)]:
                note = f"double_share_prg {fname(f)} N={N} ({n},{t}) flags={flags} pitch={pitch} phase={phase}"
                A = R.Arena()
                wl, wh = [mat(A, nm, f, n, N, pitch, align, phase) for nm in ("lo", "hi")]
                need = hm.lib.scl_hm_double_scratch_bytes(f, N, n, t, flags)
                assert (need == 0) == (f in (O.M61, O.M127, O.GF2_128) and t <= 3 and not flags), note
                ws = A.window("scratch", need, 16, 0, kind="out") if need else None
                rc = hm.lib.scl_hm_double_share_prg(f, wl.ptr, wh.ptr, pitch, N, t, n, SEED, len(SEED), 0, ws.ptr if ws else None, flags, None)
                settle(hm.lib.scl_hm_last_error, A, rc, note)
                for w, m, nm in zip((wl, wh), want, ("lo", "hi")):
                    assert np.array_equal(el(w, f), m[:, :N]), f"{note}: {nm}"


def run_apply(env, f):
    """(3,4) and (9,10) -- the thin kernel -- and (9,17) -- the general one, more than one group of rows --, batch 1 and 2; each batch of `in` and of `out` is a window of
    its own, the batch strides are the distances between them; M at a leading dimension of n + 1"""
    scl, hm, port = env
    L = limbs(f)
    for k, N in enumerate(NS):
        for m, n in ((3, 4), (9, 10), (9, 17)):
            M = model_him(port, f, m, n)
            xs = [pool(port, f, n * N, b"rz-apply-%d" % b).reshape(n, N, L) for b in range(2)]
            for batch in (1, 2):
                for align, phase, pitch in placements(f, N, k + m)[:: batch]:
                    note = f"apply {fname(f)} N={N} ({m},{n}) batch={batch} pitch={pitch} phase={phase}"
                    A = R.Arena()
                    wi = [mat(A, "in%d" % b, f, n, N, pitch, align, phase, "in", xs[b]) for b in range(batch)]
                    wm = mat(A, "M", f, m, n, n + 1, align if L > 1 else 8, 0, "in", M)
                    wo = [mat(A, "out%d" % b, f, m, N, pitch, align, phase) for b in range(batch)]
                    ibs = (wi[1].ptr - wi[0].ptr) // esz(f) if batch > 1 else 0
                    obs = (wo[1].ptr - wo[0].ptr) // esz(f) if batch > 1 else 0
                    assert batch == 1 or ((wi[1].ptr - wi[0].ptr) % esz(f) == 0 and (wo[1].ptr - wo[0].ptr) % esz(f) == 0)
                    rc = hm.lib.scl_hm_apply(f, wo[0].ptr, pitch, obs, wi[0].ptr, pitch, ibs, wm.ptr, n + 1, m, n, batch, N, None)
                    settle(hm.lib.scl_hm_last_error, A, rc, note)
                    for b in range(batch):
                        assert np.array_equal(el(wo[b], f), model_apply(port, f, M, xs[b])), f"{note}: batch {b}"


def run_mask(env, f):
    scl, hm, port = env
    L = limbs(f)
    for k, N in enumerate(NS):
        for rows in (1, 3):
            x, y, r2 = [pool(port, f, rows * N, b"rz-mask-" + t).reshape(rows, N, L) for t in (b"x", b"y", b"r")]
            want = model_mask(port, f, x, y, r2)
            for align, phase, pitch in placements(f, N, k + rows):
                for in_place in (False, True):
                    note = f"mul_mask {fname(f)} N={N} rows={rows} pitch={pitch} phase={phase} in_place={in_place}"
                    A = R.Arena()
                    wx, wy = [mat(A, nm, f, rows, N, pitch, align, phase, "in", a) for nm, a in (("x", x), ("y", y))]
                    wr = mat(A, "r2", f, rows, N, pitch, align, phase, "inout" if in_place else "in", r2)
                    wd = wr if in_place else mat(A, "d", f, rows, N, pitch + 2, align, phase)
                    rc = hm.lib.scl_hm_mul_mask(f, wd.ptr, pitch if in_place else pitch + 2, wx.ptr, wy.ptr, wr.ptr, pitch, rows, N, None)
                    settle(hm.lib.scl_hm_last_error, A, rc, note)
                    assert np.array_equal(el(wd, f), want), note


def run_finish(env, f):
    scl, hm, port = env
    L = limbs(f)
    for k, N in enumerate(NS):
        for rows, m in ((1, 1), (3, 4), (3, 64)):
            dsh = pool(port, f, m * N, b"rz-finish-d").reshape(m, N, L)
            r = pool(port, f, rows * N, b"rz-finish-r").reshape(rows, N, L)
            lam = port.from_int(f, 1)[None] if m == 1 else scl.lagrange_basis(f, m)
            lam = np.ascontiguousarray(lam, dtype=np.uint64)
            want = model_finish(port, f, model_open(port, f, dsh, lam), r)
            for align, phase, pitch in placements(f, N, k + rows)[:: (2 if m == 64 else 1)]:
                for in_place in (False, True):
                    note = f"mul_finish {fname(f)} N={N} rows={rows} m={m} pitch={pitch} phase={phase} in_place={in_place}"
                    A = R.Arena()
                    wd = mat(A, "dsh", f, m, N, pitch, align, phase, "in", dsh)
                    wr = mat(A, "r", f, rows, N, pitch, align, phase, "inout" if in_place else "in", r)
                    wz = wr if in_place else mat(A, "z", f, rows, N, pitch + 2, align, phase)
                    rc = hm.lib.scl_hm_mul_finish(f, wz.ptr, pitch if in_place else pitch + 2, wd.ptr, pitch, lam.ctypes.data, m, wr.ptr, pitch,
                                                  rows, N, None)
                    settle(hm.lib.scl_hm_last_error, A, rc, note)
                    assert np.array_equal(el(wz, f), want), note


TABLE = {"scl_hm_double_share_prg": run_double, "scl_hm_apply": run_apply, "scl_hm_mul_mask": run_mask, "scl_hm_mul_finish": run_finish}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("hm")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(HM)
    assert len(names) == 4 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_hm_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
