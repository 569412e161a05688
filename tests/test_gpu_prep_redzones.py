"""Red-zone tests for the preprocessing extension: neither scl_prep_* deal call writes outside its output windows.

tests/test_gpu_redzones.py pins WHERE every entry point of include/scl_hip.h writes and tests/test_gpu_beaver_redzones.py does
the same for include/scl_hip_mpc.h; this file does it for include/scl_hip_prep.h, through the raw C ABI with pointers into a
tests/redzone.py arena.  The calls read nothing from the device, so every window is an `out` window: the three share matrices --
n rows at a pitch larger than N, so the gaps between rows are flanks too -- and, on the two-pass path, the scratch, a window of
exactly scl_prep_triples_scratch_bytes.  One-limb windows start 0 and 8 bytes past a 16-byte boundary with even and odd pitches
(phase 0 with an even pitch is the two-per-lane body with its tail launch at odd N; everything else the one-per-lane form); wider
ones 0, 16 and 48 bytes past a 128-byte line.  N in {1, 2, 3, 64, 257}.  Each case asserts the return code, arena.check() and the
values (the model's: triples_reference of tests/gpu_support.py, shared with tests/test_gpu_triples.py).

TABLE has one row per entry point; test_every_device_entry_point_has_a_row reads the header and fails when a prototype that
takes a `_dev` pointer has none."""
import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from abi_support import PREP, device_entry_points
from gpu_support import TRIPLES_SEED as SEED
from gpu_support import triples_reference as reference
from gpu_support import el, fname, gpu_env, mat, placements, settle

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(62), O.Z2K(128)]
NS = [1, 2, 3, 64, 257]


def run_additive(env, f):
    scl, prep, port = env
    for k, N in enumerate(NS):
        for n in (2, 3):
            want = reference(port, f, n)
            for align, phase, pitch in placements(f, N, k + n):
                note = f"triples_additive_prg {fname(f)} N={N} n={n} pitch={pitch} phase={phase}"
                A = R.Arena()
                wa, wb, wc = [mat(A, nm, f, n, N, pitch, align, phase) for nm in "abc"]
                rc = prep.lib.scl_prep_triples_additive_prg(f, wa.ptr, wb.ptr, wc.ptr, pitch, N, n, SEED, len(SEED), 0, None)
                settle(prep.lib.scl_prep_last_error, A, rc, note)
                for w, m, nm in zip((wa, wb, wc), want, "abc"):
                    assert np.array_equal(el(w, f), m[:, :N]), f"{note}: {nm}"


def run_shamir(env, f):
    """(4,1) as the field takes it (fused or two passes), then forced through two passes, and (20,9): the scratch is an `out`
    window of exactly the size the library names"""
    if O.is_ring(f):
        return
    scl, prep, port = env
    for k, N in enumerate(NS):
        for n, t, flags in ((4, 1, 0), (4, 1, 1), (20, 9, 0)):
            want = reference(port, f, n, t)
            for align, phase, pitch in placements(f, N, k + n)[:: (2 if flags else 1)]:
                note = f"triples_shamir_prg {fname(f)} N={N} ({n},{t}) flags={flags} pitch={pitch} phase={phase}"
                A = R.Arena()
                wa, wb, wc = [mat(A, nm, f, n, N, pitch, align, phase) for nm in "abc"]
                need = prep.lib.scl_prep_triples_scratch_bytes(f, N, n, t, flags)
                assert (need == 0) == (f in (O.M61, O.M127, O.GF2_128) and t <= 7 and not flags), note
                ws = A.window("scratch", need, 16, 0, kind="out") if need else None
                rc = prep.lib.scl_prep_triples_shamir_prg(f, wa.ptr, wb.ptr, wc.ptr, pitch, N, t, n, SEED, len(SEED), 0,
                                                          ws.ptr if ws else None, flags, None)
                settle(prep.lib.scl_prep_last_error, A, rc, note)
                for w, m, nm in zip((wa, wb, wc), want, "abc"):
                    assert np.array_equal(el(w, f), m[:, :N]), f"{note}: {nm}"


TABLE = {"scl_prep_triples_additive_prg": run_additive, "scl_prep_triples_shamir_prg": run_shamir}
CASES = [(entry, f) for entry in TABLE for f in FIELDS + (RINGS if entry.endswith("additive_prg") else [])]


@pytest.fixture(scope="module")
def env():
    return gpu_env("prep")


def test_every_device_entry_point_has_a_row():
    """(reads the header and the table: needs no GPU)"""
    names = device_entry_points(PREP)
    assert len(names) == 2 and sorted(TABLE) == names, sorted(set(TABLE) ^ set(names))
    assert all(any(e == n for e, _ in CASES) for n in names)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,f", CASES, ids=[f"{e[len('scl_prep_'):]}-{fname(f)}" for e, f in CASES])
def test_no_write_outside_the_output_windows(env, entry, f):
    TABLE[entry](env, f)
