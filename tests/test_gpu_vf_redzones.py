"""Red-zone tests for the batch-verification extension: no scl_vf_* call writes outside its output windows.

tests/test_gpu_ip_redzones.py pins where the entry points of include/scl_hip_ip.h write; this file does it for
include/scl_hip_vf.h, through the raw C ABI with pointers into a tests/redzone.py arena.  `out` is rows x reps elements at a pitch
larger than reps, so the gaps between its rows are flanks: exactly rows x reps elements per row stride are written.  The scratch
is an `out` window of exactly scl_vf_scratch_bytes bytes: nothing beyond it is written.  x, y and the coefficient rows are `in`
windows at a pitch larger than N: unchanged.  One-limb windows start 0 and 8 bytes past a 16-byte boundary with even and odd
pitches; wider ones 0, 16 and 48 bytes past a 128-byte line.  N in {1, 2, 3, 64, 257}, rows 1 and R + 1, reps 1, 2 and 4, plain
and product.  Each case asserts the return code, arena.check() and the values (the model's).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that takes
a `_dev` pointer has none."""
import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from abi_support import VF, device_entry_points
from gpu_support import el, fname, gpu_env, limbs, mat, placements, pool, settle
from port_models import model_coins, model_combine

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 64, 257]
SEED, C0 = b"vf redzone coin", 3


def run(env, f, prg):
    scl, vf, port = env
    L = limbs(f)
    for k, N in enumerate(NS):
        for reps in (1, 2, 4):
            rows_R = vf.launch_shape(f, reps, prg)[0] + 1
            rho = model_coins(port, f, SEED, C0, N, reps)
            for rows in (1, rows_R):
                x = pool(port, f, rows * N, b"rz-vf-x").reshape(rows, N, L)
                y = pool(port, f, rows * N + 5, b"rz-vf-y")[5:].reshape(rows, N, L)
                want = {False: model_combine(port, f, x, rho), True: model_combine(port, f, x, rho, y)}
                for align, phase, pitch in placements(f, N, k + rows)[:: (1 if reps == 2 else 2)]:
                    for prod in (False, True):
                        note = f"{'combine_prg' if prg else 'combine'} {fname(f)} N={N} reps={reps} rows={rows} pitch={pitch} phase={phase} {'product' if prod else 'plain'}"
                        A = R.Arena()
                        wx = mat(A, "x", f, rows, N, pitch, align, phase, "in", x)
                        wy = mat(A, "y", f, rows, N, pitch, align, phase, "in", y)
                        wo = mat(A, "out", f, rows, reps, reps + 3, align, phase)
                        need = vf.scratch_bytes(f, rows, reps, N, vf.PRG if prg else 0)
                        ws = A.window("scratch", need, 16, 0, kind="out")
                        if prg:
                            rc = vf.lib.scl_vf_combine_prg(f, wo.ptr, reps + 3, wx.ptr, wy.ptr if prod else None, pitch, rows, N, reps, SEED, len(SEED), C0,
                                                           ws.ptr, need, None)
                        else:
                            wr = mat(A, "rho", f, reps, N, pitch, align, phase, "in", rho)
                            rc = vf.lib.scl_vf_combine(f, wo.ptr, reps + 3, wx.ptr, wy.ptr if prod else None, pitch, wr.ptr, pitch, rows, N, reps, ws.ptr,
                                                       need, None)
                        settle(vf.lib.scl_vf_last_error, A, rc, note)
                        assert np.array_equal(el(wo, f), want[prod]), note


TABLE = {"scl_vf_combine_prg": lambda env, f: run(env, f, True), "scl_vf_combine": lambda env, f: run(env, f, False)}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("vf")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(VF)
    assert len(names) == 2 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_vf_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
