"""The red-zone arena of tests/redzone.py checked on the CPU (device="cpu": no GPU needed), and the completeness check of
tests/test_gpu_redzones.py: every entry point that include/scl_hip.h declares is either a row of that file's TABLE or a key of
its EXEMPT dict -- and only the entries that write no device memory through a caller's pointer may be exempt."""
import inspect
import os
import re

import numpy as np
import pytest

import redzone as R
from abi_support import ENGINE, declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arena_with_windows():
    """an `in` vector, an `out` matrix of 5 rows of 24 bytes 40 apart at 8 past a 16-byte boundary, an `inout` status array at
    phase 3"""
    a = R.Arena("cpu", capacity=1 << 20)
    src = a.window("src", 64, align=128, phase=48, kind="in")
    dst = a.window("dst", 24, align=16, phase=8, rows=5, pitch_bytes=40, kind="out")
    st = a.window("status", 7, align=16, phase=3, kind="inout")
    src.load(np.arange(8, dtype=np.uint64))
    return a, src, dst, st


# ---------------------------------------------------------------------------------------------- the fill pattern
def test_pattern_words_are_never_zero_all_ones_or_equal_to_a_neighbour():
    n = R.MAX_CAPACITY                                   # the largest arena there is (Arena refuses a larger one)
    assert n >= R.DEFAULT_CAPACITY
    w = R.pattern(n).view(np.uint64)
    assert w.size == n // 8
    assert not (w == 0).any() and not (w == np.uint64(2 ** 64 - 1)).any()
    assert not (w[1:] == w[:-1]).any()
    # position-dependent: no word repeats anywhere, so a copy from elsewhere in the arena shows as well
    assert np.unique(w).size == w.size
    # and no byte is a value the library writes into a status / verdict array, or a cleared / all-ones byte
    b = R.pattern(n)
    assert not np.isin(b, [0, 1, 2, 255]).any()
    # a prefix of a longer fill is the shorter fill (position, not length, decides a byte)
    assert np.array_equal(R.pattern(1000), b[:1000])
    assert np.array_equal(R.pattern(1003)[:1000], b[:1000])


def test_a_fresh_arena_is_the_pattern_and_the_flanks_are_inside_it():
    a, src, dst, st = arena_with_windows()
    assert a.data.numel() == a.capacity and a.data.dtype.is_floating_point is False
    for w in (src, dst, st):
        span = w.end - w.start
        assert w.start >= max(R.MIN_FLANK, span) and w.end + max(R.MIN_FLANK, span) <= a.capacity
        assert w.ptr == a.base + w.start
    assert (src.ptr - 48) % 128 == 0 and (dst.ptr - 8) % 16 == 0 and (st.ptr - 3) % 16 == 0
    # flanks: at least the window, never under 64 KiB, and no two windows share one
    assert dst.start - src.end >= R.MIN_FLANK and st.start - dst.end >= R.MIN_FLANK
    big = a.window("big", 100_000, kind="out")
    assert big.start - st.end >= 100_000 and a.capacity - big.end >= 100_000
    with pytest.raises(MemoryError):
        a.window("too-big", 600_000)
    with pytest.raises(AssertionError):
        R.Arena("cpu", capacity=R.MAX_CAPACITY + 8)


def test_a_large_window_keeps_its_after_flank_when_a_small_one_follows():
    """the flank AFTER a window is as long as that window, whatever comes next: the window-table scratch of ec_mul (192 KiB at
    n = 65) followed by a few bytes of verdicts"""
    a = R.Arena("cpu", capacity=2 << 20)
    first = a.window("first", 16, kind="in")
    big = a.window("big", 200_000, align=128, phase=48, kind="inout")
    small = a.window("small", 8, align=16, phase=3, kind="out")
    pitched = a.window("pitched", 100, rows=1000, pitch_bytes=120, kind="out")      # span 119 980
    last = a.window("last", 1, kind="out")
    assert big.start - first.end >= 200_000
    assert small.start - big.end >= 200_000
    assert pitched.start - small.end >= 119_980 and last.start - pitched.end >= 119_980
    assert a.capacity - last.end >= R.MIN_FLANK
    for w, nxt in ((first, big), (small, pitched)):
        assert nxt.start - w.end >= R.MIN_FLANK


# ---------------------------------------------------------------------------------------------- check()
def test_clean_round_trip_passes():
    a, src, dst, st = arena_with_windows()
    a.check()
    dst.view.fill_(0)                                    # the whole output, every row
    st.view.fill_(1)
    a.check()
    assert np.array_equal(src.read(np.uint64)[0], np.arange(8, dtype=np.uint64))
    assert dst.read().shape == (5, 24) and not dst.read().any()


def test_a_write_inside_an_out_window_is_not_reported():
    a, src, dst, st = arena_with_windows()
    dst.view[0, 0] = 0
    dst.view[4, 23] = 0xEE
    st.view[0, 6] = 2
    assert a.strays() == (0, [])
    a.check()


def plant(a, pos, value=None):
    """flip one arena byte (to a value that differs from what is there)"""
    old = int(a.data[pos])
    a.data[pos] = (old ^ 0xFF) if value is None else value
    assert int(a.data[pos]) != old


@pytest.mark.parametrize("where,side,offset,row", [
    ("just-before", "before", -1, 0),
    ("just-after", "after", +1, 4),
    ("gap-last-byte", "gap", +16, 2),          # pitch 40 - 24 bytes of row = 16 gap bytes; the last one of row 2's gap
    ("gap-first-byte", "gap", +1, 0),
    ("far-flank-before", "before", -R.MIN_FLANK, 0),
    ("far-flank-after", "after", +R.MIN_FLANK, 4),
])
def test_one_planted_byte_is_caught_and_attributed(where, side, offset, row):
    a, src, dst, st = arena_with_windows()
    # the flank between dst and status is shared ground: plant on dst's side of its midpoint except for the far cases, where
    # the byte belongs to the nearer window by construction below
    pos = {"just-before": dst.start - 1, "just-after": dst.end,
           "gap-last-byte": dst.start + 2 * 40 + 39, "gap-first-byte": dst.start + 24,
           "far-flank-before": dst.start - R.MIN_FLANK, "far-flank-after": dst.end + R.MIN_FLANK - 1}[where]
    if where.startswith("far"):
        # the far end of dst's own flank: make dst the only window so that the attribution is unambiguous
        a = R.Arena("cpu", capacity=1 << 20)
        dst = a.window("dst", 24, align=16, phase=8, rows=5, pitch_bytes=40, kind="out")
        pos = dst.start - R.MIN_FLANK if where == "far-flank-before" else dst.end + R.MIN_FLANK - 1
    plant(a, pos)
    with pytest.raises(R.RedZoneError) as ei:
        a.check()
    e = ei.value
    assert e.count == 1 and len(e.strays) == 1
    s = e.strays[0]
    assert (s["window"], s["side"], s["offset"], s["count"]) == ("dst", side, offset, 1), s
    if side == "gap":
        assert s["row"] == row
    msg = str(e)
    assert "'dst'" in msg and f"{offset:+d}" in msg and "1 byte(s)" in msg
    assert {"before": "before window", "after": "after window", "gap": f"gap after row {row}"}[side] in msg


def test_a_byte_changed_inside_an_in_window_is_caught():
    a, src, dst, st = arena_with_windows()
    plant(a, src.start + 8 * 3 + 2)                      # byte 2 of element 3
    with pytest.raises(R.RedZoneError) as ei:
        a.check()
    s = ei.value.strays[0]
    assert (s["window"], s["side"], s["offset"], s["row"], s["count"]) == ("src", "inside", 26, 0, 1)
    assert "inside row 0 of window 'src'" in str(ei.value)


def test_an_in_window_that_was_never_loaded_must_keep_the_pattern():
    a = R.Arena("cpu", capacity=1 << 20)
    w = a.window("table", 32, kind="in")
    a.check()
    w.view[0, 31] = 0
    with pytest.raises(R.RedZoneError):
        a.check()


def test_storing_the_pattern_of_the_neighbouring_word_is_caught():
    """what a constant fill would let through: a kernel that copies the flank word before the window over the one after it, or
    stores the 'untouched' constant itself"""
    a, src, dst, st = arena_with_windows()
    before = a.data[dst.start - 8: dst.start].clone()
    a.data[dst.end: dst.end + 8] = before
    with pytest.raises(R.RedZoneError) as ei:
        a.check()
    assert ei.value.strays[0]["side"] == "after" and ei.value.strays[0]["offset"] == 1


def test_several_strays_are_counted_and_grouped_by_window_and_side():
    a, src, dst, st = arena_with_windows()
    for k in range(8):                                   # one 8-byte element past the end of the output
        plant(a, dst.end + k)
    plant(a, st.start - 1)
    with pytest.raises(R.RedZoneError) as ei:
        a.check()
    e = ei.value
    assert e.count == 9
    by = {(s["window"], s["side"]): s for s in e.strays}
    assert by[("dst", "after")]["count"] == 8 and by[("dst", "after")]["offset"] == 1 and by[("dst", "after")]["far"] == 8
    assert by[("status", "before")]["count"] == 1 and by[("status", "before")]["offset"] == -1


# ---------------------------------------------------------------------------------------------- completeness
# The only entries that may be exempt: those that write no device memory through a caller's pointer.  Kept HERE, apart from the
# EXEMPT dict of tests/test_gpu_redzones.py, so that moving an entry point from the table to the exemptions takes a change in two
# files that says why.
MAY_BE_EXEMPT = {
    # queries and sizes (host values only)
    "scl_hip_abi_version", "scl_hip_last_error", "scl_hip_status_message", "scl_hip_limbs", "scl_hip_field_name",
    "scl_hip_wire_size", "scl_hip_wire_size_matrix", "scl_hip_frame_size", "scl_hip_merkle_depth", "scl_hip_merkle_level_size",
    "scl_hip_merkle_tree_bytes", "scl_hip_ec_base_table_bytes", "scl_hip_ec_mul_scratch_bytes",
    # results to the host, host-side tables and settings
    "scl_hip_lagrange_basis", "scl_hip_sum", "scl_hip_dot", "scl_hip_equals", "scl_hip_set_tuning", "scl_hip_ec_generator",
    "scl_hip_mont128_set_prime", "scl_hip_mont128_get_prime", "scl_hip_mont128_relatch",
    # device, stream and timer management
    "scl_hip_device_count", "scl_hip_set_device", "scl_hip_thread_cleanup", "scl_hip_stream_create", "scl_hip_stream_destroy",
    "scl_hip_stream_sync", "scl_hip_timer_create", "scl_hip_timer_destroy", "scl_hip_timer_start", "scl_hip_timer_stop",
    "scl_hip_timer_elapsed_ms",
    # the runtime's own allocation and copies
    "scl_hip_malloc", "scl_hip_free", "scl_hip_memcpy_h2d", "scl_hip_memcpy_d2h", "scl_hip_memset",
}
MAY_BE_EXEMPT_PREFIXES = ("scl_hip_comm_", "scl_hip_open_")     # need RCCL ranks: tests/open_world_check.py


def test_every_entry_point_is_a_table_row_or_exempt_with_a_reason():
    import test_gpu_redzones as G
    names = declared_symbols(ENGINE)
    assert len(names) >= 98
    table, exempt = set(G.TABLE), set(G.EXEMPT)
    assert not table & exempt, sorted(table & exempt)
    unknown = (table | exempt) - set(names)
    assert not unknown, f"not declared in include/scl_hip.h: {sorted(unknown)}"
    missing = [n for n in names if n not in table and n not in exempt]
    assert not missing, f"neither a row of TABLE nor a key of EXEMPT in tests/test_gpu_redzones.py: {missing}"
    not_allowed = [n for n in exempt if n not in MAY_BE_EXEMPT and not n.startswith(MAY_BE_EXEMPT_PREFIXES)]
    assert not not_allowed, f"these write device memory through a caller's pointer and cannot be exempt: {not_allowed}"
    for n, reason in G.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 10 and "\n" not in reason, n


def test_every_table_row_has_cases_that_call_its_entry_point():
    """a row is a generator of cases and a runner; the runner's source calls lib.<entry point> itself (not a Python wrapper that
    allocates the output), and the row yields at least one case -- so a name cannot sit in the table without a test behind it"""
    import test_gpu_redzones as G
    for name, row in G.TABLE.items():
        cases = list(row.cases())
        assert cases, name
        src = inspect.getsource(row.run)
        assert re.search(r"\blib\." + name + r"\b", src) or re.search(r"['\"]" + name + r"['\"]", src), name
    ids = [c.id for c in G.ALL_CASES]
    assert len(ids) == len(set(ids))
    assert {c.entry for c in G.ALL_CASES} == set(G.TABLE)


def test_every_knob_value_of_the_table_comes_from_fuzz_abi_or_is_accounted_for():
    """the knob values are those tests/fuzz_abi.py documents in KNOBS; one that is not carries its source in EXTRA_KNOB_VALUES"""
    import test_gpu_redzones as G
    used = {(k, v) for c in G.ALL_CASES for k, v in c.knobs.items()}
    stray = sorted(kv for kv in used if kv[1] not in G.KNOBS.get(kv[0], []) and kv not in G.EXTRA_KNOB_VALUES)
    assert not stray, stray
    assert set(G.EXTRA_KNOB_VALUES) <= used and all(len(why) >= 20 for why in G.EXTRA_KNOB_VALUES.values())
    assert all(k in G.KNOB_DEFAULTS for k, _ in used)
    # every knob the table is asked to use is used
    for key in ("mfma", "force_table", "force_scalar", "transpose_tile", "inv_batch", "inv_two_level", "gf_tiles", "matmul_lds_min",
                "gemm_slab_mib", "max_blocks", "aes_blocks"):
        assert any(k == key for k, _ in used), key
