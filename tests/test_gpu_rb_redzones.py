"""Red-zone tests for the random-bit extension: no scl_rb_* call writes outside its output windows.

tests/test_gpu_vf_redzones.py pins where the entry points of include/scl_hip_vf.h write; this file does it for
include/scl_hip_rb.h, through the raw C ABI with pointers into a tests/redzone.py arena.  The root vector and the status bytes
are `out` windows of exactly N elements and N bytes; b is rows x N elements at a pitch larger than N, so the gaps between its
rows are flanks: exactly N elements per row stride are written.  a, u and r are `in` windows: unchanged.  One-limb windows start
0 and 8 bytes past a 16-byte boundary with even and odd pitches (one and two columns per lane); wider ones 0, 16 and 48 bytes
past a 128-byte line; the status window starts at every byte phase in turn.  N in {1, 2, 3, 64, 65, 257}, rows 1, 3 and 10 (and
17 over Mersenne61, past the preloaded rows).  Each case asserts the return code, arena.check() and the values (the model's).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that takes
a `_dev` pointer has none."""
import numpy as np
import pytest

import oracle_lib as O
import rb_support as RBS
import redzone as R
from abi_support import device_entry_points
from gpu_support import el, esz, fname, gpu_env, mat, placements, settle

FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 64, 65, 257]


def operands(f, N, rows, tag):
    """a: seeded, a zero in the middle; u: squares, one zero and one non-residue from N = 3 on; r: seeded -> integers"""
    p = RBS.prime(f)
    a = RBS.seeded(p, N, 7000 + tag)
    u = [v * v % p for v in RBS.seeded(p, N, 7100 + tag)]
    if N >= 3:
        z = 2
        while RBS.is_residue(p, z):
            z += 1
        a[N // 2], u[N // 2], u[N - 1] = 0, 0, z * u[N - 1] % p
    return p, a, u, [RBS.seeded(p, N, 7200 + tag + i) for i in range(rows)]


def run_sqrt(env, f):
    scl, rb, port = env
    for k, N in enumerate(NS):
        p, a, _, _ = operands(f, N, 1, k)
        for j, (align, phase, _) in enumerate(placements(f, N, k)):
            flags = (k + j) % 4
            note = f"sqrt {fname(f)} N={N} phase={phase} flags={flags}"
            A = R.Arena()
            wa = mat(A, "a", f, 1, N, N, align, phase, "in", RBS.to_limbs(f, a))
            wo = mat(A, "out", f, 1, N, N, align, phase)
            ws = A.window("status", N, 16, (k + 5 * j) % 16, kind="out")
            rc = rb.lib.scl_rb_sqrt(f, wo.ptr, ws.ptr, wa.ptr, N, flags, None)
            settle(rb.lib.scl_rb_last_error, A, rc, note)
            want = [RBS.model_sqrt(p, v, flags) for v in a]
            assert RBS.from_limbs(f, el(wo, f)) == [v for v, _ in want] and ws.read().reshape(-1).tolist() == [s for _, s in want], note


def run_bits(env, f):
    scl, rb, port = env
    for k, N in enumerate(NS):
        for rows in (1, 3, 10) + ((17,) if f == O.M61 else ()):
            p, _, u, r = operands(f, N, rows, 10 * k + rows)
            want, wstatus = RBS.model_bits(p, u, r)
            for j, (align, phase, pitch) in enumerate(placements(f, N, k + rows)):
                note = f"bits_finish {fname(f)} N={N} rows={rows} pitch={pitch} phase={phase}"
                A = R.Arena()
                wu = mat(A, "u", f, 1, N, N, align, phase, "in", RBS.to_limbs(f, u))
                wr = mat(A, "r", f, rows, N, pitch, align, phase, "in", np.stack([RBS.to_limbs(f, row) for row in r]))
                wb = mat(A, "b", f, rows, N, pitch + 2, align, phase)
                ws = A.window("status", N, 16, (3 * k + 7 * j + rows) % 16, kind="out")
                rc = rb.lib.scl_rb_bits_finish(f, wb.ptr, pitch + 2, ws.ptr, wu.ptr, wr.ptr, pitch, rows, N, None)
                settle(rb.lib.scl_rb_last_error, A, rc, note)
                assert RBS.from_limbs(f, el(wb, f)) == [v for row in want for v in row] and ws.read().reshape(-1).tolist() == wstatus, note


TABLE = {"scl_rb_sqrt": run_sqrt, "scl_rb_bits_finish": run_bits}
CASES = [(entry, f) for entry in TABLE for f in FIELDS]


@pytest.fixture(scope="module")
def env():
    return gpu_env("rb")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(RBS.RB)
    assert len(names) == 2 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_rb_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
