"""Red-zone tests: no entry point writes outside its output windows.

The value tests pin WHAT every kernel computes; this file pins WHERE it writes.  Every entry point of include/scl_hip.h that
writes device memory through a caller's pointer is called through the raw C ABI (scl.lib.scl_hip_*) with pointers into a
tests/redzone.py arena: operands are `in` windows, outputs `out` windows, in-place operands and caller-supplied scratch `inout`
windows of exactly the documented size.  Each case asserts (a) arena.check(): no byte outside the output windows changed and no
input changed, (b) the output windows hold the right result, (c) the return code is SCL_OK or the documented one.

References for (b): tests/oracle_lib.py's Port for every field, ring, sharing, matrix, layout, wire and PRG entry point; hashlib
and the Merkle model of tests/test_merkle_host.py for the hash family.  For the secp256k1 family (ec_*, Feldman, Pedersen, ECDSA)
the reference is THE SAME ENTRY POINT called through its ordinary wrapper on plain allocations: tests/test_gpu_feldman.py,
tests/test_gpu_pedersen.py and tests/test_gpu_ecdsa.py already pin that call to the big-integer model and the fixtures, and the
Python model is too slow to repeat here.  This is the one place where a test compares the library with itself, and the reason is
that placement, not the value, is the property under test (the kernels are deterministic: byte equality is expected).
GF(2^128) has no usable default nodes in the oracle (its x++ walk alternates 1, 0 in characteristic 2): its sharings are checked
through the oracle's poly_eval at the bit patterns 1..n, and recover_detect / recover_correct leave it out as tests/fuzz_abi.py
does.

Shapes are the smallest at which a tail exists: N in {1, 2, 3, 255, 256, 257} (BLOCK = 256) plus one element past every tile
that is wider than a block, each cited where it is used; the tuning knobs reach each kernel family at these sizes.  Placement:
one-limb windows start 0 and 8 bytes past a 16-byte boundary (the second is the one-element-per-lane fallback of vec_width) with
even and odd pitches; wider fields 0, 16 and 48 bytes past a 128-byte line; wire buffers 0 and 4 past a 16-byte boundary; status
and verdict bytes 0, 1 and 3 past a boundary.  TABLE has one row per entry point; tests/test_redzone_model.py checks that every
declared entry point is a row here or a key of EXEMPT.
"""
import ast
import ctypes as C
import functools
import os
import hashlib

import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from merkle_model import model_levels, model_path, model_tree_bytes, sha

import torch


def _fuzz_abi_tables():
    """KNOBS and KNOB_DEFAULTS of tests/fuzz_abi.py, read from its source: importing it would load the built library, and the
    table below has to be readable (tests/test_redzone_model.py) in a tree that has not been built"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_abi.py")) as fh:
        tree = ast.parse(fh.read())
    found = {n.targets[0].id: ast.literal_eval(n.value) for n in tree.body
             if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and n.targets[0].id in ("KNOBS", "KNOB_DEFAULTS")}
    return found["KNOBS"], found["KNOB_DEFAULTS"]


KNOBS, KNOB_DEFAULTS = _fuzz_abi_tables()
# knob values a row uses beyond fuzz_abi's KNOBS, each with where it comes from (tests/test_redzone_model.py allows no others)
EXTRA_KNOB_VALUES = {
    ("force_table", 3): "documented in include/scl_hip.h (GF(2^128) reconstruct on the shared-shift nibble tables) and taken at "
                        "recover_block's GF(2^128) branch; fuzz_abi leaves it out because it only matters to one field's reconstruct",
}
FIELDS6 = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]     # fuzz_abi's FIELDS

pytestmark = pytest.mark.gpu

OK, ERR_ZERO_INVERSE, ERR_ERROR_DETECTED, ERR_NOT_INVERTIBLE_2K = 0, 2, 6, 11
M61, M127, MONT128, GF, SCALAR, FIELD = O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD
RINGS = [O.Z2K(62), O.Z2K(128)]
FIELDS8 = list(FIELDS6) + RINGS
FIELDS3 = [M61, M127, SCALAR]             # one limb, one 16-byte field, one 32-byte field
NOGF = [f for f in FIELDS6 if f != GF]
BATCH = [1, 2, 3, 255, 256, 257]          # 1, 2, odd, and BLOCK = 256 (kernels.hpp) with one either side
EC_N = [1, 63, 64, 65]                    # EBLOCK = 64 (ec_unit.hip:24, ecdsa_unit.hip:24) with one either side
PT = 96                                   # bytes of a point: 12 limbs

EXEMPT = {
    "scl_hip_abi_version": "query: returns a host integer",
    "scl_hip_last_error": "query: returns a host string",
    "scl_hip_status_message": "query: returns a host string",
    "scl_hip_limbs": "query: returns a host integer",
    "scl_hip_field_name": "query: returns a host string",
    "scl_hip_wire_size": "size computation on the host",
    "scl_hip_wire_size_matrix": "size computation on the host",
    "scl_hip_frame_size": "size computation on the host",
    "scl_hip_merkle_depth": "shape computation on the host",
    "scl_hip_merkle_level_size": "shape computation on the host",
    "scl_hip_merkle_tree_bytes": "size computation on the host",
    "scl_hip_ec_base_table_bytes": "size computation on the host",
    "scl_hip_ec_mul_scratch_bytes": "size computation on the host",
    "scl_hip_lagrange_basis": "host table in, host table out: no device memory",
    "scl_hip_sum": "reads device memory, result to a host pointer",
    "scl_hip_dot": "reads device memory, result to a host pointer",
    "scl_hip_equals": "reads device memory, result to a host pointer",
    "scl_hip_set_tuning": "per-thread host setting",
    "scl_hip_ec_generator": "writes a host array",
    "scl_hip_mont128_set_prime": "per-thread host setting",
    "scl_hip_mont128_get_prime": "writes a host array",
    "scl_hip_mont128_relatch": "per-thread host setting",
    "scl_hip_device_count": "device management",
    "scl_hip_set_device": "device management",
    "scl_hip_thread_cleanup": "frees the library's own per-thread buffers",
    "scl_hip_stream_create": "stream management",
    "scl_hip_stream_destroy": "stream management",
    "scl_hip_stream_sync": "stream management",
    "scl_hip_timer_create": "timer management",
    "scl_hip_timer_destroy": "timer management",
    "scl_hip_timer_start": "timer management",
    "scl_hip_timer_stop": "timer management",
    "scl_hip_timer_elapsed_ms": "timer management, result to a host pointer",
    "scl_hip_malloc": "the runtime's allocation, no kernel of the library",
    "scl_hip_free": "the runtime's allocation, no kernel of the library",
    "scl_hip_memcpy_h2d": "the runtime's copy, no kernel of the library",
    "scl_hip_memcpy_d2h": "the runtime's copy, no kernel of the library",
    "scl_hip_memset": "the runtime's fill, no kernel of the library",
    "scl_hip_comm_unique_id": "needs RCCL: tests/open_world_check.py",
    "scl_hip_comm_init_rank": "needs RCCL ranks: tests/open_world_check.py",
    "scl_hip_comm_adopt": "needs an RCCL communicator: tests/open_world_check.py",
    "scl_hip_comm_info": "needs an RCCL communicator: tests/open_world_check.py",
    "scl_hip_comm_destroy": "needs an RCCL communicator: tests/open_world_check.py",
    "scl_hip_open_row_order": "host table of the open step: tests/open_world_check.py",
    "scl_hip_open_all_gather": "needs RCCL ranks: tests/open_world_check.py",
    "scl_hip_open_partial_gather": "needs RCCL ranks: tests/open_world_check.py",
    "scl_hip_open_reduce_scatter": "needs RCCL ranks: tests/open_world_check.py",
}


# ---------------------------------------------------------------------------------------------- the table's machinery
class Case:
    def __init__(self, entry, label, params, knobs):
        self.entry, self.params, self.knobs = entry, params, knobs
        self.id = entry[len("scl_hip_"):] + "-" + label


class Row:
    """one entry point: run(env, **params) is the runner, cases() its (label, params, knobs) list as Case objects"""

    def __init__(self, entry, run, specs):
        self.entry, self.run, self.specs = entry, run, specs

    def cases(self):
        return [Case(self.entry, label, params, knobs) for label, params, knobs in self.specs]


TABLE = {}


def row(entry, specs):
    def deco(fn):
        assert entry not in TABLE
        TABLE[entry] = Row(entry, fn, list(specs))
        return fn
    return deco


class Env:
    def __init__(self, scl, port):
        self.scl, self.lib, self.port = scl, scl.lib, port


def fname(f):
    return {M61: "m61", M127: "m127", MONT128: "mont128", GF: "gf128", SCALAR: "secp_scalar", FIELD: "secp_field"}.get(
        f, "z2k%d" % (f - 0x100))


def knob_label(knobs):
    return "".join("-%s=%d" % kv for kv in knobs.items())


def limbs(f):
    return O.LIMBS[f]


def esz(f):
    return 8 * limbs(f)


def place(f, pi):
    """(align, phase) of placement index pi: one-limb windows 0 / 8 past a 16-byte boundary, wider 0 / 16 / 48 past a line"""
    return (16, (0, 8)[pi % 2]) if limbs(f) == 1 else (128, (0, 16, 48)[pi % 3])


def pitch1(N, parity):
    p = N + 2
    return p if p % 2 == parity else p + 1


def placements(f, Ns=BATCH):
    """(N, placement index, row pitch in elements).  One limb: both phases at every N, the pitch even and odd in turn, so that
    phase 0 with an even pitch (the two-per-lane body of split_vec with its one-per-lane tail) meets N = 1, 3 and 257.  Wider
    fields: two of the three phases at every N in rotation -- every phase meets the odd N -- at a pitch of N + 3."""
    out = []
    if limbs(f) == 1:
        for k, N in enumerate(Ns):
            for pi in (0, 1):
                out.append((N, pi, pitch1(N, (k + pi) % 2)))
        out.append((Ns[-1], 0, pitch1(Ns[-1], 0)))
    else:
        for k, N in enumerate(Ns):
            for pi in (k % 3, (k + 1) % 3):
                out.append((N, pi, N + 3))
    return out


def vec(A, name, f, n, pi, kind, data=None):
    al, ph = place(f, pi)
    w = A.window(name, n * esz(f), al, ph, kind=kind)
    return w.load(data) if data is not None else w


def mat(A, name, f, rows, cols, pitch, pi, kind, data=None):
    al, ph = place(f, pi)
    w = A.window(name, cols * esz(f), al, ph, rows=rows, pitch_bytes=pitch * esz(f), kind=kind)
    return w.load(data) if data is not None else w


def raw(A, name, nbytes, align, phase, kind, data=None, rows=1, pitch=None):
    w = A.window(name, nbytes, align, phase, rows=rows, pitch_bytes=pitch, kind=kind)
    return w.load(data) if data is not None else w


def el(w, f):
    """a window's elements [rows][cols][limbs] (a vector: [n][limbs])"""
    a = w.read(np.uint64).reshape(w.rows, -1, limbs(f))
    return a[0] if w.rows == 1 else a


def settle(env, A, rc, want_rc, note):
    """(c) the return code, then (a) the red zones"""
    assert rc == want_rc, f"{note}: status {rc} ({env.lib.scl_hip_last_error().decode()}), expected {want_rc}"
    try:
        A.check()
    except R.RedZoneError as e:
        raise R.RedZoneError(f"{note}\n{e}", e.strays, e.count) from None


def same(got, want, note):
    assert np.array_equal(np.asarray(got), np.asarray(want)), f"{note}: wrong result"


def rnd(env, f, n, tag):
    """n uniform elements from the oracle's own read of PRG bytes"""
    if O.is_ring(f):
        bs = O.byte_size(f)
        return env.port.from_bytes(f, env.port.prg(b"rz-" + tag, [max(n, 1) * bs]))[:n]
    return env.port.vector_random(f, b"rz-" + tag, n)


def soa(aos):
    return np.ascontiguousarray(np.transpose(aos, (1, 0, 2)))


def one(env, f):
    return env.port.from_int(f, 1)


# ---------------------------------------------------------------------------------------------- element-wise
_EW = {}


def ew_ref(env, f, op):
    """operands and the oracle's result for 257 elements, computed once per (field, op): every shape takes a prefix"""
    if (f, op) not in _EW:
        a, b = rnd(env, f, 257, b"ew-a"), rnd(env, f, 257, b"ew-b")
        tgt = b if op == O.DIV else a
        if op in (O.INV, O.DIV):
            if O.is_ring(f):
                tgt[:, 0] |= np.uint64(1)                     # a ring inverts odd values
            else:
                tgt[(tgt == 0).all(axis=1)] = one(env, f)
        want = env.port.ew(f, op, a, b if op in (O.ADD, O.SUB, O.MUL, O.DIV) else None)
        _EW[(f, op)] = (a, b, want)
    return _EW[(f, op)]


OPNAME = {O.ADD: "add", O.SUB: "sub", O.MUL: "mul", O.NEG: "neg", O.INV: "inv", O.DIV: "div"}


def _ew(env, call, f, op, inplace, with_status=False, plant=False):
    binary = op in (O.ADD, O.SUB, O.MUL, O.DIV)
    a0, b0, want0 = ew_ref(env, f, op)
    for N, pi, _ in placements(f):
        note = f"{fname(f)} {OPNAME[op]} N={N} placement {place(f, pi)} inplace={inplace} plant={plant}"
        a, b, want = a0[:N].copy(), b0[:N].copy(), want0[:N].copy()
        want_flag = 0
        if plant:                                            # a zero (even, in a ring) operand in the LAST slot: the tail's
            (b if op == O.DIV else a)[N - 1] = 0
            want[N - 1] = 0
            want_flag = 1
        A = R.Arena()
        wa = vec(A, "a", f, N, pi, "inout" if inplace else "in", a)
        wb = vec(A, "b", f, N, pi, "in", b) if binary else None
        wd = wa if inplace else vec(A, "dst", f, N, pi, "out")
        args = [f, op, wd.ptr, wa.ptr, wb.ptr if wb else None, N]
        if with_status:
            # one 32-bit word, 4-byte aligned (scl_hip.h): 0, 4 and 12 bytes past a 16-byte boundary
            ws = raw(A, "status", 4, 16, (0, 4, 12)[(N + pi) % 3], "inout", np.zeros(1, dtype=np.uint32))
            args.append(ws.ptr)
        rc = call(*args, None)
        bad_rc = ERR_NOT_INVERTIBLE_2K if O.is_ring(f) else ERR_ZERO_INVERSE
        settle(env, A, rc, bad_rc if plant and not with_status else OK, note)
        same(el(wd, f), want, note)
        if with_status:
            assert int(ws.read(np.uint32)[0, 0]) == want_flag, note


def ew_specs(with_status):
    out = []
    for f in FIELDS8:
        for op in (O.ADD, O.MUL, O.NEG, O.INV, O.DIV):
            for inplace in (False, True):
                out.append((f"{fname(f)}-{OPNAME[op]}{'-inplace' if inplace else ''}", dict(f=f, op=op, inplace=inplace), {}))
        out.append((f"{fname(f)}-inv-zero-in-the-last-slot", dict(f=f, op=O.INV, inplace=False, plant=True), {}))
    # the inversion kernels behind "inv_batch" (chain lengths, -1: one Fermat chain per element) and "inv_two_level"
    for f in (M61, M127, MONT128, GF, SCALAR):
        for v in (-1, 8, 16, 32, 64, 128):
            out.append((f"{fname(f)}-div-inplace-inv_batch={v}", dict(f=f, op=O.DIV, inplace=True), {"inv_batch": v}))
    for f in (M127, MONT128):
        for v in (-1, 4, 8):
            out.append((f"{fname(f)}-inv-inv_batch=64-inv_two_level={v}", dict(f=f, op=O.INV, inplace=False),
                        {"inv_batch": 64, "inv_two_level": v}))
    for f in FIELDS3 + [GF]:
        out.append((f"{fname(f)}-mul-force_scalar=1", dict(f=f, op=O.MUL, inplace=False), {"force_scalar": 1}))
        for mb in (1, 7, 300):
            out.append((f"{fname(f)}-add-max_blocks={mb}", dict(f=f, op=O.ADD, inplace=False), {"max_blocks": mb}))
    if with_status:
        out = [(label, dict(p, with_status=True), k) for label, p, k in out]
    return out


@row("scl_hip_ew", ew_specs(False))
def run_ew(env, **kw):
    _ew(env, env.lib.scl_hip_ew, **kw)


@row("scl_hip_ew_status", ew_specs(True))
def run_ew_status(env, **kw):
    _ew(env, env.lib.scl_hip_ew_status, **kw)


@row("scl_hip_scalar_mul", [(f"{fname(f)}{'-inplace' if ip else ''}{knob_label(k)}", dict(f=f, inplace=ip), k)
                            for f in FIELDS8 for ip in (False, True) for k in ({},)] +
     [(f"{fname(f)}{knob_label(k)}", dict(f=f, inplace=False), k) for f in (M61, GF) for k in ({"force_scalar": 1}, {"inv_batch": -1})])
def run_scalar_mul(env, f, inplace):
    s = rnd(env, f, 1, b"sm-s")
    a0 = rnd(env, f, 257, b"sm-a")
    want0 = env.port.scalar_mul(f, a0, s[0])
    for N, pi, _ in placements(f):
        note = f"{fname(f)} scalar_mul N={N} placement {place(f, pi)} inplace={inplace}"
        A = R.Arena()
        wa = vec(A, "a", f, N, pi, "inout" if inplace else "in", a0[:N])
        wd = wa if inplace else vec(A, "dst", f, N, pi, "out")
        rc = env.lib.scl_hip_scalar_mul(f, wd.ptr, wa.ptr, s.ctypes.data, N, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f), want0[:N], note)


# ---------------------------------------------------------------------------------------------- randomness
@row("scl_hip_prg_blocks", [("blocks" + knob_label(k), {}, k) for k in ({}, {"aes_blocks": 1}, {"aes_blocks": 64}, {"max_blocks": 1})])
def run_prg_blocks(env):
    seed = b"rz-prg-seed"
    for k, nb in enumerate(BATCH + [5]):                     # (four blocks per lane: 5 = one lane and a quarter)
        for ph in ((0, 16, 48)[k % 3], (0, 16, 48)[(k + 1) % 3]):   # the destination must be 16-byte aligned
            note = f"prg_blocks nblocks={nb} phase {ph}"
            A = R.Arena()
            wd = raw(A, "dst", 16 * nb, 128, ph, "out")
            rc = env.lib.scl_hip_prg_blocks(wd.ptr, nb, seed, len(seed), 2 ** 32 - 3, None)
            settle(env, A, rc, OK, note)
            assert wd.read().tobytes() == env.port.prg_blocks(seed, 2 ** 32 - 3, nb), note


@row("scl_hip_from_bytes", [(fname(f) + knob_label(k), dict(f=f), k) for f in FIELDS8 for k in ({},)] +
     [(fname(f) + "-max_blocks=1", dict(f=f), {"max_blocks": 1}) for f in FIELDS3])
def run_from_bytes(env, f):
    bs = O.byte_size(f)
    src0 = env.port.prg(b"rz-fb", [257 * bs])
    want0 = env.port.from_bytes(f, src0)
    for N, pi, _ in placements(f):
        note = f"{fname(f)} from_bytes N={N} placement {place(f, pi)}"
        A = R.Arena()
        ws = raw(A, "src", N * bs, 16, (0, 1, 3)[(N + pi) % 3], "in", np.frombuffer(src0[:N * bs], dtype=np.uint8))
        wd = vec(A, "dst", f, N, pi, "out")
        rc = env.lib.scl_hip_from_bytes(f, wd.ptr, ws.ptr, N, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f), want0[:N], note)


@row("scl_hip_vector_random", [(fname(f) + knob_label(k), dict(f=f), k) for f in FIELDS8 for k in ({},)] +
     [(fname(f) + knob_label(k), dict(f=f), k) for f in FIELDS3 for k in ({"aes_blocks": 1}, {"max_blocks": 1})])
def run_vector_random(env, f):
    seed, bs = b"rz-vr", O.byte_size(f)
    for N, pi, _ in placements(f):
        for c0 in (0, 7):
            note = f"{fname(f)} vector_random N={N} counter0={c0} placement {place(f, pi)}"
            A = R.Arena()
            wd = vec(A, "dst", f, N, pi, "out")
            rc = env.lib.scl_hip_vector_random(f, wd.ptr, N, seed, len(seed), c0, None)
            settle(env, A, rc, OK, note)
            # Vector::random (vector.h:507-519): one draw of ceil(N byteSize / 16) blocks from counter0, T::read per element
            want = env.port.from_bytes(f, env.port.prg_blocks(seed, c0, (N * bs + 15) // 16))[:N]
            same(el(wd, f), want, note)


# ---------------------------------------------------------------------------------------------- Shamir sharing
def gf_nodes(n):
    return O.from_ints(list(range(1, n + 1)), 2)


def share_want(env, f, secrets, coeffs, n):
    """[n][N][L] shares of secrets [N][L] with coefficients [N][t][L] at the default nodes"""
    if f == GF:     # the library's GF(2^128) nodes are the bit patterns 1..n
        nodes = gf_nodes(n)
        return soa(np.stack([env.port.poly_eval(f, np.concatenate([secrets[s:s + 1], coeffs[s]]), nodes) for s in range(secrets.shape[0])]))
    return soa(env.port.shamir_share_coeffs(f, secrets, coeffs, n))


# (n, t) across the dispatch of scl_hip_shamir_share (its with_field body in capi.hip): (10, 3) the small-node kernels; t = 4 | 5 and 16 | 17
# either side of the register-specialised Horner range 5..16 (k_share with 4 / 16 / 48 coefficients in registers; 32-byte elements take
# the chunked kernel past 16, share_chunked)
SHARE_SHAPES = [(10, 3), (10, 4), (10, 5), (20, 16), (20, 17)]
# Mersenne61 on the matrix cores ("mfma" 1).  One element past each kernel's column tile: k_share_mfma_m61_p16 and _pipe take 32
# secrets per trip (launch_share_mfma: nblocks = (N + 31) / 32) -> 33; k_share_mfma_m61<KS, MT> takes 2 * (4 / MT) * 32 columns
# (launch_share_mfma) -> 129 for two row tiles (33..64 parties), 257 for one (already in BATCH)
MFMA_SHARE = [((128, 42), [33]), ((100, 40), [33]), ((128, 63), [33]), ((100, 20), [33]), ((40, 13), [129]), ((10, 3), [])]


def share_specs():
    out = [(f"{fname(f)}-n{n}-t{t}", dict(f=f, n=n, t=t), {}) for f in FIELDS6 for n, t in SHARE_SHAPES]
    for f in FIELDS3 + [GF]:
        for k in ({"force_table": 1}, {"force_table": 2}, {"max_blocks": 1}):
            for n, t in ((10, 3), (10, 5)):
                out.append((f"{fname(f)}-n{n}-t{t}{knob_label(k)}", dict(f=f, n=n, t=t), k))
    out.append(("m61-n10-t3-force_scalar=1", dict(f=M61, n=10, t=3), {"force_scalar": 1}))
    out.append(("gf128-n10-t5-gf_tiles=0", dict(f=GF, n=10, t=5), {"gf_tiles": 0}))
    out.append(("m61-n10-t3-share_waves=0", dict(f=M61, n=10, t=3), {"share_waves": 0}))
    for f in (M127, MONT128, SCALAR):
        out.append((f"{fname(f)}-n10-t3-share_waves128=0", dict(f=f, n=10, t=3), {"share_waves128": 0}))
    for (n, t), extra in MFMA_SHARE:
        out.append((f"m61-n{n}-t{t}-mfma=1", dict(f=M61, n=n, t=t, extra=tuple(extra)), {"mfma": 1}))
    out.append(("m61-n40-t13-mfma=-1", dict(f=M61, n=40, t=13), {"mfma": -1}))
    return out


@row("scl_hip_shamir_share", share_specs())
def run_shamir_share(env, f, n, t, extra=()):
    L = limbs(f)
    NM = max(BATCH + list(extra))
    sec0, co0 = rnd(env, f, NM, b"sh-s"), rnd(env, f, NM * t, b"sh-c").reshape(NM, t, L)
    want0 = share_want(env, f, sec0, co0, n)                  # [n][NM][L]: every shape takes a prefix of the secrets
    for N, pi, pitch in placements(f, BATCH + list(extra)):
        note = f"{fname(f)} shamir_share ({n},{t}) N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = vec(A, "secrets", f, N, pi, "in", sec0[:N])
        wc = mat(A, "coeffs", f, t, N, pitch + 2, pi, "in", soa(co0[:N]))
        wd = mat(A, "shares", f, n, N, pitch, pi, "out")
        rc = env.lib.scl_hip_shamir_share(f, wd.ptr, pitch, ws.ptr, wc.ptr, pitch + 2, N, t, n, None, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f).reshape(n, N, L), want0[:, :N], note)


def prg_coeffs(env, f, seed, N, t, c0=0):
    """the coefficients c_1..c_t shamirSecretShare draws for secret s: Vector::random(t + 1) from blocks [c0 + s B, ..)"""
    B = ((t + 1) * esz(f) + 15) // 16
    return np.stack([env.port.from_bytes(f, env.port.prg_blocks(seed, c0 + s * B, B))[1:t + 1] for s in range(N)])


@row("scl_hip_shamir_share_prg",
     [(f"{fname(f)}-n{n}-t{t}", dict(f=f, n=n, t=t), {}) for f in FIELDS6 for n, t in ((10, 3), (10, 5), (20, 17))] +
     [(f"{fname(f)}-n10-t3{knob_label(k)}", dict(f=f, n=10, t=3), k) for f in FIELDS3
      for k in ({"prg_two_pass": 1}, {"prg_two_pass": -1}, {"aes_blocks": 1}, {"force_table": 1})] +
     [("m61-n128-t42-mfma=1", dict(f=M61, n=128, t=42, extra=(33,)), {"mfma": 1})])
def run_shamir_share_prg(env, f, n, t, extra=()):
    L, seed = limbs(f), b"rz-share-prg"
    NM = max(BATCH + list(extra))
    sec0 = rnd(env, f, NM, b"sp-s")
    if f == GF:
        want0 = share_want(env, f, sec0, prg_coeffs(env, f, seed, NM, t), n)
    else:
        want0 = soa(env.port.shamir_share(f, seed, sec0, t, n))
    for N, pi, pitch in placements(f, BATCH + list(extra)):
        note = f"{fname(f)} shamir_share_prg ({n},{t}) N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = vec(A, "secrets", f, N, pi, "in", sec0[:N])
        wd = mat(A, "shares", f, n, N, pitch, pi, "out")
        rc = env.lib.scl_hip_shamir_share_prg(f, wd.ptr, pitch, ws.ptr, N, t, n, seed, len(seed), 0, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f).reshape(n, N, L), want0[:, :N], note)


@row("scl_hip_shamir_share_prg_packed",
     [(f"{fname(f)}-n{n}-t{t}-w{w}", dict(f=f, n=n, t=t, W=w), {}) for f in NOGF for n, t, w in ((10, 3, 2), (5, 5, 3))] +
     [(f"{fname(f)}-n10-t3-w2{knob_label(k)}", dict(f=f, n=10, t=3, W=2), k) for f in FIELDS3 for k in ({"prg_two_pass": 1}, {"prg_two_pass": -1})])
def run_shamir_share_prg_packed(env, f, n, t, W):
    L, seed = limbs(f), b"rz-packed"
    sec0 = rnd(env, f, 257 * W, b"pk-s").reshape(257, W, L)
    want0 = np.asarray(env.port.shamir_share_packed(f, seed, sec0, t, n))       # [N][n][W][L]
    for N, pi, pitch in placements(f):
        note = f"{fname(f)} shamir_share_prg_packed ({n},{t}) W={W} N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = mat(A, "secrets", f, W, N, pitch + 2, pi, "in", np.ascontiguousarray(sec0[:N].transpose(1, 0, 2)))
        wd = mat(A, "shares", f, W * n, N, pitch, pi, "out")
        rc = env.lib.scl_hip_shamir_share_prg_packed(f, wd.ptr, pitch, ws.ptr, pitch + 2, N, t, n, W, seed, len(seed), 0, None)
        settle(env, A, rc, OK, note)
        got = el(wd, f).reshape(W, n, N, L).transpose(2, 1, 0, 3)
        same(got, want0[:N], note)


# ---------------------------------------------------------------------------------------------- reconstruction
@row("scl_hip_shamir_recover",
     [(f"{fname(f)}-m{m}", dict(f=f, m=m), {}) for f in FIELDS6 for m in (4, 10, 40)] +
     [(f"{fname(f)}-m10{knob_label(k)}", dict(f=f, m=10), k) for f in FIELDS3
      for k in ({"force_table": 1}, {"max_blocks": 1}, {"stream_waves": 0})] +
     # ("force_table" 3 is not among fuzz_abi's KNOBS: see EXTRA_KNOB_VALUES)
     [("gf128-m10-force_table=3", dict(f=GF, m=10), {"force_table": 3}), ("gf128-m40-force_table=1", dict(f=GF, m=40), {"force_table": 1}),
      ("m61-m10-force_scalar=1", dict(f=M61, m=10), {"force_scalar": 1})])
def run_shamir_recover(env, f, m):
    L = limbs(f)
    sh0 = rnd(env, f, 257 * m, b"rc-sh").reshape(257, m, L)   # reconstruction is linear: any rows do
    lam = env.scl.lagrange_basis(f, m)
    want0 = env.port.shamir_recover_lambda(f, sh0, lam)
    for N, pi, pitch in placements(f):
        note = f"{fname(f)} shamir_recover m={m} N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = mat(A, "shares", f, m, N, pitch, pi, "in", soa(sh0[:N]))
        wd = vec(A, "out", f, N, pi, "out")
        rc = env.lib.scl_hip_shamir_recover(f, wd.ptr, ws.ptr, pitch, lam.ctypes.data, m, N, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f), want0[:N], note)


# recover_detect (scl_hip_shamir_recover_detect), t = d, m = 2t + 1: nchk = t - 1 check rows and the value row, rows = t
# (its nchk and rows).  Vector-ALU kernel: rows <= 4 take four rows per pass, more take eight (RBsel; 32-byte elements two) -> t = 3, 5 and 9 (two row blocks).  Matrix
# cores under "mfma" 1 (detect_mfma): rows * (d + 1) = 10 * 11 = 110 below 512, 23 * 24 = 552 above it (one row tile: 256 columns
# per workgroup, 257 is in BATCH), and t = 40 with two k-steps and two row tiles: 128 columns (launch_share_mfma) -> 129
DETECT = [(3, {}, ()), (5, {}, ()), (9, {}, ())]
DETECT_MFMA = [(10, {"mfma": 1}, ()), (23, {"mfma": 1}, ()), (40, {"mfma": 1}, (129,))]


@row("scl_hip_shamir_recover_detect",
     [(f"{fname(f)}-t{t}", dict(f=f, t=t, extra=x), k) for f in NOGF for t, k, x in DETECT] +
     [(f"m61-t{t}{knob_label(k)}", dict(f=M61, t=t, extra=x), k) for t, k, x in DETECT_MFMA] +
     [("m61-t9-mfma=-1", dict(f=M61, t=9, extra=()), {"mfma": -1}), ("m61-t3-force_scalar=1", dict(f=M61, t=3, extra=()), {"force_scalar": 1})])
def run_shamir_recover_detect(env, f, t, extra):
    L, n = limbs(f), 2 * t + 1
    NM = max(BATCH + list(extra))
    sec0 = rnd(env, f, NM, b"dt-s")
    sh0 = np.asarray(env.port.shamir_share(f, b"rz-detect", sec0, t, n)).reshape(NM, n, L)
    for idx, (N, pi, pitch) in enumerate(placements(f, BATCH + list(extra))):
        for planted in (False, True):
            note = f"{fname(f)} recover_detect t={t} N={N} placement {place(f, pi)} pitch {pitch} planted={planted}"
            sh = sh0[:N].copy()
            if planted:                                       # an error in the first and in the LAST secret (the tail's)
                for s in {0, N - 1}:
                    j = (s + idx) % (2 * t)                   # (share 2t is neither interpolated nor checked, shamir.h:129)
                    sh[s, j] = env.port.ew(f, O.ADD, sh[s, j:j + 1], one(env, f).reshape(1, L))[0]
            want_val, want_st = env.port.shamir_recover_d(f, sh, t)
            bad_s = np.asarray(want_st).astype(bool)
            assert bad_s.any() == planted
            A = R.Arena()
            ws = mat(A, "shares", f, n, N, pitch, pi, "in", soa(sh))
            wd = vec(A, "out", f, N, pi, "out")
            wst = raw(A, "status", N, 16, (0, 1, 3)[(idx + planted) % 3], "out")
            nbad = C.c_size_t(99)
            rc = env.lib.scl_hip_shamir_recover_detect(f, wd.ptr, wst.ptr, ws.ptr, pitch, n, N, t, t, None, None, C.byref(nbad), None)
            settle(env, A, rc, ERR_ERROR_DETECTED if planted else OK, note)
            assert nbad.value == int(bad_s.sum()), note
            same(wst.read()[0].astype(bool), bad_s, note)
            assert set(np.unique(wst.read())) <= {0, 1}, note
            got = el(wd, f)
            same(got[~bad_s], want_val[~bad_s], note)
            assert not got[bad_s].any(), note                 # out[s] = 0 where an error was detected (scl_hip.h)


# Berlekamp-Welch (scl_hip_shamir_recover_correct): one shape in each storage regime of k_bw_solve.  n = 7: one wavefront; n = 67: the systems
# in the workgroup's LDS for 8- and 16-byte elements (n <= 136 / 95: in_lds) and ALREADY in the device-memory slice for
# 32-byte elements (n <= 66); n = 148 over Mersenne61: the device-memory slice.  Secret s is clean, correctable (t errors) or
# uncorrectable (t + 1 errors) by s mod 3, so the queued path writes f, err, nerr and status.
@row("scl_hip_shamir_recover_correct",
     [(f"{fname(f)}-n{n}", dict(f=f, n=n, Ns=Ns), {}) for f, n, Ns in
      [(M61, 7, (1, 2, 3, 257)), (M61, 67, (5,)), (M61, 148, (5,)), (M127, 7, (3, 257)), (M127, 67, (5,)),
       (MONT128, 7, (3,)), (SCALAR, 7, (3, 257)), (SCALAR, 67, (4,)), (FIELD, 7, (3,))]])
def run_shamir_recover_correct(env, f, n, Ns):
    L, t = limbs(f), (n - 1) // 3
    for idx, (N, pi, pitch) in enumerate(placements(f, list(Ns))):
        note = f"{fname(f)} recover_correct n={n} N={N} placement {place(f, pi)} pitch {pitch}"
        sec = rnd(env, f, N, b"bw-s")
        sh = np.asarray(env.port.shamir_share(f, b"rz-bw", sec, t, n)).reshape(N, n, L).copy()
        for s in range(N):
            for j in range({0: 0, 1: t, 2: t + 1}[s % 3]):
                p = (3 * j + s) % n if 3 * (t + 1) <= n + 2 else j
                sh[s, p] = env.port.ew(f, O.ADD, sh[s, p:p + 1], env.port.from_int(f, 7 + j).reshape(1, L))[0]
        fo, eo, st, ne = env.port.shamir_recover_c(f, sh)
        st = np.asarray(st).astype(bool)
        if N >= 3:
            assert st.any() and not st.all(), note            # the three classes are really there
        A = R.Arena()
        fs, es = pitch, pitch + 2                             # pitches above N, f's and err's different
        ws = mat(A, "shares", f, n, N, pitch + 4, pi, "in", soa(sh))
        wf = mat(A, "f", f, n, N, fs, pi, "out")
        we = mat(A, "err", f, t + 1, N, es, pi, "out")
        wst = raw(A, "status", N, 16, (0, 1, 3)[idx % 3], "out")
        wne = raw(A, "nerr", 4 * N, 16, (0, 4, 12)[idx % 3], "out")
        q, fl = C.c_size_t(99), C.c_size_t(99)
        rc = env.lib.scl_hip_shamir_recover_correct(f, wf.ptr, fs, we.ptr, es, wst.ptr, wne.ptr, ws.ptr, pitch + 4, n, N, None,
                                                    C.byref(q), C.byref(fl), None)
        settle(env, A, rc, OK, note)
        same(wst.read()[0].astype(bool), st, note)
        assert fl.value == int(st.sum()) and q.value >= fl.value and q.value == sum(1 for s in range(N) if s % 3), note
        gf_, ge, gn = el(wf, f).reshape(n, N, L).transpose(1, 0, 2), el(we, f).reshape(t + 1, N, L).transpose(1, 0, 2), wne.read(np.uint32)[0]
        same(gf_[~st], np.asarray(fo)[~st], note)
        same(ge[~st], np.asarray(eo)[~st], note)
        same(gn[~st], np.asarray(ne)[~st], note)
        assert not gf_[st].any() and not ge[st].any() and not gn[st].any(), note   # f, E and nerr zeroed (scl_hip.h)


# ---------------------------------------------------------------------------------------------- additive sharing
def add_specs(knobs=({},)):
    return [(f"{fname(f)}-n{n}{knob_label(k)}", dict(f=f, n=n), k) for f in FIELDS8 for n in (1, 2, 5) for k in knobs] + \
           [(f"{fname(f)}-n5{knob_label(k)}", dict(f=f, n=5), k) for f in FIELDS3 for k in ({"force_scalar": 1}, {"max_blocks": 1})]


@row("scl_hip_additive_share", add_specs())
def run_additive_share(env, f, n):
    L = limbs(f)
    sec0, rnd0 = rnd(env, f, 257, b"ad-s"), rnd(env, f, 257 * max(n - 1, 1), b"ad-r").reshape(max(n - 1, 1), 257, L)[:n - 1]
    last = sec0.copy()
    for i in range(n - 1):                                    # additive.h:41-53: the last share is secret - sum of the others
        last = env.port.ew(f, O.SUB, last, rnd0[i])
    for N, pi, pitch in placements(f):
        note = f"{fname(f)} additive_share n={n} N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = vec(A, "secrets", f, N, pi, "in", sec0[:N])
        wr = mat(A, "rnd", f, n - 1, N, pitch + 2, pi, "in", np.ascontiguousarray(rnd0[:, :N])) if n > 1 else None
        wd = mat(A, "shares", f, n, N, pitch, pi, "out")
        rc = env.lib.scl_hip_additive_share(f, wd.ptr, pitch, ws.ptr, wr.ptr if wr else None, pitch + 2, N, n, None)
        settle(env, A, rc, OK, note)
        got = el(wd, f).reshape(n, N, L)
        same(got[:n - 1], rnd0[:, :N], note)
        same(got[n - 1], last[:N], note)


@row("scl_hip_additive_share_prg", add_specs() + [(f"{fname(f)}-n5-aes_blocks=1", dict(f=f, n=5), {"aes_blocks": 1}) for f in FIELDS3])
def run_additive_share_prg(env, f, n):
    L, seed = limbs(f), b"rz-additive"
    sec0 = rnd(env, f, 257, b"ap-s")
    want0 = soa(np.asarray(env.port.additive_share(f, seed, sec0, n)).reshape(257, n, L))
    for N, pi, pitch in placements(f):
        note = f"{fname(f)} additive_share_prg n={n} N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = vec(A, "secrets", f, N, pi, "in", sec0[:N])
        wd = mat(A, "shares", f, n, N, pitch, pi, "out")
        rc = env.lib.scl_hip_additive_share_prg(f, wd.ptr, pitch, ws.ptr, N, n, seed, len(seed), 0, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f).reshape(n, N, L), want0[:, :N], note)


@row("scl_hip_additive_recover", add_specs())
def run_additive_recover(env, f, n):
    L = limbs(f)
    sh0 = rnd(env, f, 257 * n, b"ar-sh").reshape(257, n, L)
    want0 = env.port.additive_recover(f, sh0)
    for N, pi, pitch in placements(f):
        note = f"{fname(f)} additive_recover n={n} N={N} placement {place(f, pi)} pitch {pitch}"
        A = R.Arena()
        ws = mat(A, "shares", f, n, N, pitch, pi, "in", soa(sh0[:N]))
        wd = vec(A, "out", f, N, pi, "out")
        rc = env.lib.scl_hip_additive_recover(f, wd.ptr, ws.ptr, pitch, n, N, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f), want0[:N], note)


# ---------------------------------------------------------------------------------------------- matrices
@row("scl_hip_vandermonde", [(fname(f), dict(f=f), {}) for f in FIELDS6])
def run_vandermonde(env, f):
    for idx, (n, m) in enumerate([(1, 1), (3, 2), (10, 4), (257, 3), (2, 257)]):
        for pi in (idx, idx + 1):
            note = f"{fname(f)} vandermonde {n} x {m} placement {place(f, pi)}"
            xs = rnd(env, f, n, b"vd-x") if (f == GF or idx % 2) else None
            A = R.Arena()
            wd = vec(A, "V", f, n * m, pi, "out")
            rc = env.lib.scl_hip_vandermonde(f, wd.ptr, n, m, xs.ctypes.data if xs is not None else None, None)
            settle(env, A, rc, OK, note)
            same(el(wd, f).reshape(n, m, limbs(f)), env.port.vandermonde(f, n, m, xs), note)


def tiled_edge(f):
    """one row, one k-step and one column past a tile of k_matmul_tiled: MatmulShape (kernels.hpp:3280-3288) has TM = 16 RM,
    TN = 16 RN, TK = 16 (8 for 32-byte elements); RM x RN = 2 x 1 for 32-byte elements, 2 x 2 for Mont128, 4 x 4 otherwise"""
    if limbs(f) == 4:
        return 33, 9, 17
    return (33, 17, 33) if f == MONT128 else (65, 17, 65)


def matmul_specs():
    out = []
    for f in FIELDS8:
        M, K, N = tiled_edge(f)
        shapes = [(1, 1, 1), (3, 2, 1), (257, 3, 1),             # one column: k_matvec, a wavefront per row (scl_hip_matmul, N == 1)
                  (2, 3, 3), (3, 5, 255), (M, K, N),
                  (5, 513, 5)]                                   # K >= 512 and few tiles: slices of K to a temporary (scl_hip_matmul, split)
        out.append((fname(f), dict(f=f, shapes=shapes), {"mfma": -1} if f == M61 else {}))
        if f == M61:    # what the shape picks by itself: the tiled kernel, the general matrix-core kernel, one matrix-core tile
            out.append(("m61-auto", dict(f=f, shapes=[(65, 17, 65), (33, 65, 33), (100, 43, 300)]), {}))
        # "matmul_lds_min" 1024: k_matmul_thin for K <= 16 (8 for 32-byte elements) and k_matmul beyond, a thread per (pack of)
        # column(s) from 1024 columns (scl_hip_matmul, k_matmul_thin); 1025 has the odd tail of split_vec
        out.append((fname(f) + "-matmul_lds_min=1024", dict(f=f, shapes=[(3, 5, 1025), (3, 17, 1025), (3, 5, 1024)]),
                    dict({"matmul_lds_min": 1024}, **({"mfma": -1} if f == M61 else {}))))
    for f in (M61, M127):
        out.append((fname(f) + "-matmul_lds_min=4096", dict(f=f, shapes=[(3, 5, 4097), (3, 17, 4097)]),
                    dict({"matmul_lds_min": 4096}, **({"mfma": -1} if f == M61 else {}))))
    # Mersenne61 on the matrix cores.  "mfma" 2: row blocks of 128 and k-chunks of 64 on the sharing kernels, the later chunks
    # ADDING into C (matmul_mfma_blocks) -> 129 rows, 65 inner; columns one past the 32 / 128 / 256 of a trip (launch_share_mfma)
    out.append(("m61-mfma=2", dict(f=M61, shapes=[(3, 2, 3), (33, 17, 257), (40, 33, 129), (129, 65, 33), (100, 130, 33)]), {"mfma": 2}))
    # the general kernel (gemm_mfma.hpp): tiles of 32 x 32 x 32, a workgroup takes 2 x 2 tiles (gemm_mfma_slab) -> 33 and 65 in
    # every dimension; K = 1000 is 32 k-tiles, from where few workgroups split K into slices (gemm_mfma_slab, needs ldc == N)
    out.append(("m61-mfma=1-gemm", dict(f=M61, shapes=[(33, 65, 33), (65, 65, 65), (33, 97, 65), (34, 1000, 35)], dense=(34, 1000, 35)), {"mfma": 1}))
    # "gemm_slab_mib" 1: 65536 16-byte units per factor and launch; K = 1025 is 33 k-tiles of 512 units, so 3 tiles = 96 rows /
    # columns per slab (matmul_gemm_mfma) -> 97 takes a second slab of one row and one column
    for v in (1, 4):
        out.append((f"m61-mfma=1-gemm_slab_mib={v}", dict(f=M61, shapes=[(97, 1025, 97)]), {"mfma": 1, "gemm_slab_mib": v}))
    return out


@row("scl_hip_matmul", matmul_specs())
def run_matmul(env, f, shapes, dense=None):
    L = limbs(f)
    for idx, (M, K, N) in enumerate(shapes):
        Am, Bm = rnd(env, f, M * K, b"mm-a").reshape(M, K, L), rnd(env, f, K * N, b"mm-b").reshape(K, N, L)
        want = np.asarray(env.port.matmul(f, Am, Bm)).reshape(M, N, L)
        for pi in (idx, idx + 1):
            odd = (idx + pi) % 2
            ldc = N if (M, K, N) == dense else pitch1(N, odd) if L == 1 else N + 3
            lda, ldb = K + 1 + odd, ldc + 2
            note = f"{fname(f)} matmul {M} x {K} x {N} placement {place(f, pi)} ldc {ldc} lda {lda} ldb {ldb}"
            A = R.Arena(capacity=16 << 20)
            wa = mat(A, "A", f, M, K, lda, pi, "in", Am)
            wb = mat(A, "B", f, K, N, ldb, pi, "in", Bm)
            wc = mat(A, "C", f, M, N, ldc, pi, "out")
            rc = env.lib.scl_hip_matmul(f, wc.ptr, ldc, wa.ptr, lda, wb.ptr, ldb, M, K, N, None)
            settle(env, A, rc, OK, note)
            same(el(wc, f).reshape(M, N, L), want, note)


# ---------------------------------------------------------------------------------------------- the layout bridge
def transpose_edges(f, n, knobs):
    """one secret past a tile of the layout kernels (transpose_impl in capi.hip): k_transpose16 takes the largest power
    of two within min(40 KiB / (n L 8), "transpose_tile" or 512), at least 64 (t16); k_transpose (odd strides,
    8-byte alignment, "force_scalar") takes 32 KiB / (n L 8) capped at 1024, a multiple of 64 from 64 up (tile)"""
    per = n * limbs(f) * 8
    t16 = min(40 * 1024 // per, knobs.get("transpose_tile", 0) or 512)
    t16 = max([p for p in (64, 128, 256, 512) if p <= t16], default=0)
    tile = min(1024, 32 * 1024 // per)
    if tile >= 64:
        tile &= ~63
    return sorted({e + 1 for e in (t16, tile) if e})


def layout_specs():
    out = []
    for f in FIELDS8:
        for n in (1, 3, 10):
            out.append((f"{fname(f)}-n{n}", dict(f=f, n=n, knobs={}), {}))
        for k in ({"transpose_tile": 64}, {"transpose_tile": 128}, {"transpose_tile": 256}, {"force_scalar": 1}):
            out.append((f"{fname(f)}-n10{knob_label(k)}", dict(f=f, n=10, knobs=k), k))
    return out


def _layout(env, call, to_soa, f, n, knobs):
    L = limbs(f)
    Ns = BATCH + [e for e in transpose_edges(f, n, knobs) if e not in BATCH]
    aos0 = rnd(env, f, max(Ns) * n, b"ly").reshape(max(Ns), n, L)
    for N, pi, pitch in placements(f, Ns):
        note = f"{fname(f)} {'aos_to_soa' if to_soa else 'soa_to_aos'} n={n} N={N} placement {place(f, pi)} stride {pitch}"
        A = R.Arena()
        if to_soa:
            ws = vec(A, "aos", f, N * n, pi, "in", aos0[:N])
            wd = mat(A, "soa", f, n, N, pitch, pi, "out")
            rc = call(f, wd.ptr, pitch, ws.ptr, N, n, None)
            want = soa(aos0[:N])
        else:
            ws = mat(A, "soa", f, n, N, pitch, pi, "in", soa(aos0[:N]))
            wd = vec(A, "aos", f, N * n, pi, "out")
            rc = call(f, wd.ptr, ws.ptr, pitch, N, n, None)
            want = aos0[:N]
        settle(env, A, rc, OK, note)
        same(el(wd, f).reshape(want.shape), want, note)


@row("scl_hip_aos_to_soa", layout_specs())
def run_aos_to_soa(env, **kw):
    _layout(env, env.lib.scl_hip_aos_to_soa, True, **kw)


@row("scl_hip_soa_to_aos", layout_specs())
def run_soa_to_aos(env, **kw):
    _layout(env, env.lib.scl_hip_soa_to_aos, False, **kw)


# ---------------------------------------------------------------------------------------------- wire and frame images
WIRE_SPECS = [(fname(f) + knob_label(k), dict(f=f), k) for f in FIELDS3 for k in ({}, {"max_blocks": 1})]
MATS = [(1, 1), (3, 2), (2, 255), (257, 1), (5, 65)]


def wire_phase(k):
    return (0, 4)[k % 2]          # wire buffers are 4-byte aligned (scl_hip.h): 0 and 4 bytes past a 16-byte boundary


def _wire_pack(env, call, framed, f):
    for idx, (N, pi, _) in enumerate(placements(f)):
        note = f"{fname(f)} {'frame' if framed else 'wire'}_pack N={N} placement {place(f, pi)} wire phase {wire_phase(idx)}"
        a = rnd(env, f, N, b"wp")
        want = env.port.frame(f, a) if framed else env.port.wire_vector(f, a)
        A = R.Arena()
        ws = vec(A, "src", f, N, pi, "in", a)
        wd = raw(A, "image", len(want), 16, wire_phase(idx), "out")
        rc = call(f, wd.ptr, ws.ptr, N, None)
        settle(env, A, rc, OK, note)
        assert wd.read().tobytes() == want, note


def _wire_unpack(env, call, framed, f):
    for idx, (N, pi, _) in enumerate(placements(f)):
        note = f"{fname(f)} {'frame' if framed else 'wire'}_unpack N={N} placement {place(f, pi)} wire phase {wire_phase(idx)}"
        a = rnd(env, f, N, b"wu")
        img = env.port.frame(f, a) if framed else env.port.wire_vector(f, a)
        A = R.Arena()
        ws = raw(A, "image", len(img), 16, wire_phase(idx), "in", np.frombuffer(img, dtype=np.uint8))
        wd = vec(A, "dst", f, N, pi, "out")                   # capacity = the count: not one element more
        got_n = C.c_size_t(0)
        rc = call(f, wd.ptr, N, ws.ptr, len(img), C.byref(got_n), None)
        settle(env, A, rc, OK, note)
        assert got_n.value == N, note
        same(el(wd, f), a, note)


def _wire_pack_matrix(env, call, framed, f):
    L = limbs(f)
    for idx, (rows, cols) in enumerate(MATS):
        for pi in (idx, idx + 1):
            ld = pitch1(cols, (idx + pi) % 2) if L == 1 else cols + 3
            note = f"{fname(f)} {'frame' if framed else 'wire'}_pack_matrix {rows} x {cols} ld {ld} placement {place(f, pi)}"
            a = rnd(env, f, rows * cols, b"wm").reshape(rows, cols, L)
            want = env.port.frame(f, a, as_matrix=True) if framed else env.port.wire_matrix(f, a)
            A = R.Arena()
            ws = mat(A, "src", f, rows, cols, ld, pi, "in", a)
            wd = raw(A, "image", len(want), 16, wire_phase(idx + pi), "out")
            rc = call(f, wd.ptr, ws.ptr, ld, rows, cols, None)
            settle(env, A, rc, OK, note)
            assert wd.read().tobytes() == want, note


@row("scl_hip_wire_pack", WIRE_SPECS)
def run_wire_pack(env, f):
    _wire_pack(env, env.lib.scl_hip_wire_pack, False, f)


@row("scl_hip_frame_pack", WIRE_SPECS)
def run_frame_pack(env, f):
    _wire_pack(env, env.lib.scl_hip_frame_pack, True, f)


@row("scl_hip_wire_unpack", WIRE_SPECS)
def run_wire_unpack(env, f):
    _wire_unpack(env, env.lib.scl_hip_wire_unpack, False, f)


@row("scl_hip_frame_unpack", WIRE_SPECS)
def run_frame_unpack(env, f):
    _wire_unpack(env, env.lib.scl_hip_frame_unpack, True, f)


@row("scl_hip_wire_pack_matrix", WIRE_SPECS)
def run_wire_pack_matrix(env, f):
    _wire_pack_matrix(env, env.lib.scl_hip_wire_pack_matrix, False, f)


@row("scl_hip_frame_pack_matrix", WIRE_SPECS)
def run_frame_pack_matrix(env, f):
    _wire_pack_matrix(env, env.lib.scl_hip_frame_pack_matrix, True, f)


@row("scl_hip_wire_unpack_matrix", WIRE_SPECS)
def run_wire_unpack_matrix(env, f):
    L = limbs(f)
    for idx, (rows, cols) in enumerate(MATS):
        for pi in (idx, idx + 1):
            ld = pitch1(cols, (idx + pi) % 2) if L == 1 else cols + 3
            note = f"{fname(f)} wire_unpack_matrix {rows} x {cols} ld {ld} placement {place(f, pi)}"
            a = rnd(env, f, rows * cols, b"wx").reshape(rows, cols, L)
            img = env.port.wire_matrix(f, a)
            A = R.Arena()
            ws = raw(A, "image", len(img), 16, wire_phase(idx + pi), "in", np.frombuffer(img, dtype=np.uint8))
            wd = mat(A, "dst", f, rows, cols, ld, pi, "out")  # capacity_rows = rows: not one row more
            r, c = C.c_size_t(0), C.c_size_t(0)
            rc = env.lib.scl_hip_wire_unpack_matrix(f, wd.ptr, ld, rows, ws.ptr, len(img), C.byref(r), C.byref(c), None)
            settle(env, A, rc, OK, note)
            assert (r.value, c.value) == (rows, cols), note
            same(el(wd, f).reshape(rows, cols, L), a, note)


@row("scl_hip_stream_copy", [("copy" + knob_label(k), {}, k) for k in ({}, {"max_blocks": 1})])
def run_stream_copy(env):
    for k, n16 in enumerate(BATCH):                           # 16 bytes per lane, BLOCK lanes
        for ph in ((0, 16, 48)[k % 3], (0, 16, 48)[(k + 1) % 3]):
            note = f"stream_copy {16 * n16} bytes phase {ph}"
            data = np.frombuffer(env.port.prg(b"rz-copy", [16 * n16]), dtype=np.uint8)
            A = R.Arena()
            ws = raw(A, "src", 16 * n16, 128, ph, "in", data)
            wd = raw(A, "dst", 16 * n16, 128, (ph + 16) % 64, "out")
            rc = env.lib.scl_hip_stream_copy(wd.ptr, ws.ptr, 16 * n16, None)
            settle(env, A, rc, OK, note)
            same(wd.read()[0], data, note)


# ---------------------------------------------------------------------------------------------- SHA-256 and Merkle
def digests_of(env, count, tag):
    b = env.port.prg(b"rz-dg-" + tag, [32 * count])
    return [b[32 * i:32 * i + 32] for i in range(count)]


def dig_phase(k):
    return (0, 16, 48)[k % 3]     # digest buffers are 16-byte aligned (scl_hip.h)


@row("scl_hip_sha256", [("len%d-%s" % (ln, "dense" if dense else "odd-stride"), dict(ln=ln, dense=dense), {})
                        for ln in (0, 55, 56, 64, 119) for dense in (True, False)])
def run_sha256(env, ln, dense):
    stride = ln if dense else (ln + 3) | 1
    for k, count in enumerate([1, 2, 3, 65, 257]):
        for ph in (dig_phase(k), dig_phase(k + 1)):
            note = f"sha256 len {ln} stride {stride} count {count} digest phase {ph}"
            span = (count - 1) * stride + ln
            msgs = np.frombuffer(env.port.prg(b"rz-sha", [max(span, 1)]), dtype=np.uint8)[:span]
            A = R.Arena()
            wm = raw(A, "msgs", max(span, 1), 16, (0, 1, 3)[k % 3], "in", msgs if span else None)
            wd = raw(A, "digests", 32 * count, 128, ph, "out")
            rc = env.lib.scl_hip_sha256(wd.ptr, wm.ptr, ln, stride, count, None)
            settle(env, A, rc, OK, note)
            want = b"".join(hashlib.sha256(msgs[i * stride:i * stride + ln].tobytes()).digest() for i in range(count))
            assert wd.read().tobytes() == want, note


@row("scl_hip_merkle_leaves", [(fname(f), dict(f=f), {}) for f in FIELDS3])
def run_merkle_leaves(env, f):
    L = limbs(f)
    for idx, (rows, cols) in enumerate([(1, 1), (3, 5), (2, 257), (5, 64), (1, 255)]):
        for pi in (idx, idx + 1):
            stride = pitch1(cols, (idx + pi) % 2) if L == 1 else cols + 3
            note = f"{fname(f)} merkle_leaves {rows} x {cols} stride {stride} placement {place(f, pi)}"
            a = rnd(env, f, rows * cols, b"ml").reshape(rows, cols, L)
            A = R.Arena()
            ws = mat(A, "a", f, rows, cols, stride, pi, "in", a)
            wd = raw(A, "digests", 32 * rows * cols, 128, dig_phase(idx + pi), "out")
            rc = env.lib.scl_hip_merkle_leaves(f, wd.ptr, ws.ptr, stride, rows, cols, None)
            settle(env, A, rc, OK, note)
            image = env.port.wire_vector(f, a.reshape(-1, L))[4:]      # the bytes wire_pack puts behind its count
            want = b"".join(sha(image[i * esz(f):(i + 1) * esz(f)]) for i in range(rows * cols))
            assert wd.read().tobytes() == want, note


MERKLE = [(L_, T) for L_ in (1, 2, 3, 5, 64, 65) for T in (1, 3)]      # odd level sizes at 3, 5 and 65 (33, 17, 9, 5, 3)


@row("scl_hip_merkle_build", [("L%d-T%d%s" % (L_, T, "-inplace" if ip else ""), dict(L_=L_, T=T, inplace=ip), {})
                              for L_, T in MERKLE for ip in (False, True)])
def run_merkle_build(env, L_, T, inplace):
    dg = digests_of(env, L_ * T, b"build")
    want = model_tree_bytes(dg, L_, T)
    nbytes = env.lib.scl_hip_merkle_tree_bytes(L_, T)
    assert nbytes == len(want)
    for k in range(3):
        note = f"merkle_build L={L_} T={T} inplace={inplace} phase {dig_phase(k)}"
        A = R.Arena()
        leaves = np.frombuffer(b"".join(dg), dtype=np.uint8)
        # the tree is exactly scl_hip_merkle_tree_bytes(L, T): a kernel that keeps one digest more than the header promises fails
        wt = raw(A, "tree", nbytes, 128, dig_phase(k), "inout" if inplace else "out")
        if inplace:
            wt.view[0, :leaves.size].copy_(torch.from_numpy(leaves.copy()).to(wt.view.device))
            wl = wt
        else:
            wl = raw(A, "leaves", leaves.size, 128, dig_phase(k + 1), "in", leaves)
        rc = env.lib.scl_hip_merkle_build(wt.ptr, wl.ptr, L_, T, None)
        settle(env, A, rc, OK, note)
        assert wt.read().tobytes() == want, note


@row("scl_hip_merkle_root", [("L%d-T%d" % (L_, T), dict(L_=L_, T=T), {}) for L_, T in MERKLE])
def run_merkle_root(env, L_, T):
    dg = digests_of(env, L_ * T, b"root")
    want = b"".join(model_levels([dg[j * T + t] for j in range(L_)])[-1][0] for t in range(T))
    for k in range(3):
        note = f"merkle_root L={L_} T={T} phase {dig_phase(k)}"
        A = R.Arena()
        wl = raw(A, "leaves", 32 * L_ * T, 128, dig_phase(k + 1), "in", np.frombuffer(b"".join(dg), dtype=np.uint8))
        wr = raw(A, "roots", 32 * T, 128, dig_phase(k), "out")
        rc = env.lib.scl_hip_merkle_root(wr.ptr, wl.ptr, L_, T, None)
        settle(env, A, rc, OK, note)
        assert wr.read().tobytes() == want, note


def merkle_queries(L_, T, mode):
    """(leaf, tree) per query: every leaf of every tree in the regular pattern, or a scattered list through index arrays"""
    if mode == "regular":
        return [(q // T, q % T) for q in range(L_ * T)]
    return [((7 * q + 3) % L_, (5 * q + 1) % T) for q in range(L_ * T + 2)]


@row("scl_hip_merkle_paths", [("L%d-T%d-%s" % (L_, T, mode), dict(L_=L_, T=T, mode=mode), {})
                              for L_, T in MERKLE for mode in ("regular", "indexed")])
def run_merkle_paths(env, L_, T, mode):
    dg = digests_of(env, L_ * T, b"paths")
    per_tree = [model_levels([dg[j * T + t] for j in range(L_)]) for t in range(T)]
    tree = model_tree_bytes(dg, L_, T)
    qs = merkle_queries(L_, T, mode)
    k, depth = len(qs), len(per_tree[0]) - 1
    paths = [model_path(per_tree[t], leaf) for leaf, t in qs]
    want = b"".join(paths[q][l] for l in range(depth) for q in range(k))
    for ph in range(3):
        note = f"merkle_paths L={L_} T={T} {mode} phase {dig_phase(ph)}"
        A = R.Arena()
        wt = raw(A, "tree", len(tree), 128, dig_phase(ph + 1), "in", np.frombuffer(tree, dtype=np.uint8))
        wp = raw(A, "path", 32 * depth * k, 128, dig_phase(ph), "out")
        li = ti = None
        if mode == "indexed":
            li = raw(A, "leaf_index", 8 * k, 16, 8 * (ph % 2), "in", np.array([q[0] for q in qs], dtype=np.uint64))
            ti = raw(A, "tree_index", 8 * k, 16, 8 * ((ph + 1) % 2), "in", np.array([q[1] for q in qs], dtype=np.uint64))
        rc = env.lib.scl_hip_merkle_paths(wp.ptr, wt.ptr, L_, T, li.ptr if li else None, ti.ptr if ti else None, 0, k, None)
        settle(env, A, rc, OK, note)
        assert wp.read().tobytes() == want, note


@row("scl_hip_merkle_verify", [("L%d-T%d-%s" % (L_, T, mode), dict(L_=L_, T=T, mode=mode), {})
                               for L_, T in MERKLE for mode in ("regular", "indexed")])
def run_merkle_verify(env, L_, T, mode):
    dg = digests_of(env, L_ * T, b"verify")
    per_tree = [model_levels([dg[j * T + t] for j in range(L_)]) for t in range(T)]
    depth = len(per_tree[0]) - 1
    roots = b"".join(per_tree[t][-1][0] for t in range(T))
    # regular: one party's leaf in every tree (leaf index from the host, root q mod T); indexed: scattered (leaf, tree) pairs
    qs = [(L_ - 1, t) for t in range(T)] if mode == "regular" else merkle_queries(L_, T, mode)
    k = len(qs)
    paths = [model_path(per_tree[t], leaf) for leaf, t in qs]
    leafs = [dg[leaf * T + t] for leaf, t in qs]
    tampered = {k - 1}                                        # the LAST query's proof does not verify: its byte is 0
    flat = bytearray(b"".join(paths[q][l] for l in range(depth) for q in range(k)))
    lf = bytearray(b"".join(leafs))
    lf[32 * (k - 1) + 5] ^= 0x10
    want = np.array([0 if q in tampered else 1 for q in range(k)], dtype=np.uint8)
    for ph in range(3):
        note = f"merkle_verify L={L_} T={T} {mode} verdict phase {(0, 1, 3)[ph]}"
        A = R.Arena()
        wl = raw(A, "leaves", 32 * k, 128, dig_phase(ph), "in", np.frombuffer(bytes(lf), dtype=np.uint8))
        wp = raw(A, "path", max(len(flat), 32), 128, dig_phase(ph + 1), "in", np.frombuffer(bytes(flat), dtype=np.uint8) if flat else None)
        wr = raw(A, "roots", 32 * T, 128, dig_phase(ph + 2), "in", np.frombuffer(roots, dtype=np.uint8))
        wo = raw(A, "ok", k, 16, (0, 1, 3)[ph], "out")
        li = ri = None
        if mode == "indexed":
            li = raw(A, "leaf_index", 8 * k, 16, 8 * (ph % 2), "in", np.array([q[0] for q in qs], dtype=np.uint64))
            ri = raw(A, "root_index", 8 * k, 16, 8 * ((ph + 1) % 2), "in", np.array([q[1] for q in qs], dtype=np.uint64))
        rc = env.lib.scl_hip_merkle_verify(wo.ptr, wl.ptr, li.ptr if li else None, L_ - 1, wp.ptr, depth, wr.ptr,
                                           ri.ptr if ri else None, T, k, None)
        settle(env, A, rc, OK, note)
        same(wo.read()[0], want, note)


# ---------------------------------------------------------------------------------------------- secp256k1: points
# The reference of every row below is the same entry point through its wrapper on plain allocations (see the docstring).
def host(t):
    return t.detach().cpu().numpy()


def scalars(env, n, tag):
    return env.scl.vector_random(SCALAR, n, b"rz-ec-" + tag)


@functools.lru_cache(maxsize=None)
def _tables(scl):
    g = scl.ec_base_table()
    h_pt = scl.to_host(scl.ec_mul_base(g, scl.vector_random(SCALAR, 1, b"rz-ec-h")))[0]
    return g, scl.ec_base_table(h_pt), h_pt


def points(env, n, tag):
    """n points with Z != 1: sums of two multiples of the generator"""
    g = _tables(env.scl)[0]
    p = env.scl.ec_mul_base(g, scalars(env, n, tag + b"-1"))
    return env.scl.ec_ew(O.ADD, p, env.scl.ec_mul_base(g, scalars(env, n, tag + b"-2")))


def table_win(A, name, t, ph):
    return raw(A, name, t.numel(), 128, ph, "in", host(t))


def ec_phase(k):
    return (0, 16, 48)[k % 3]     # point and scalar arrays are 16-byte aligned (scl_hip.h)


def byte_phase(k):
    return (0, 1, 3)[k % 3]


def ec_shapes(Ns=EC_N):
    """(n, phase index): two of the three phases at every n, all three at the odd ones between them"""
    return [(n, k + j) for k, n in enumerate(Ns) for j in (0, 1)]


EC_DBL = 6


@row("scl_hip_ec_ew", [(name + ("-inplace" if ip else ""), dict(op=op, inplace=ip), {})
                       for name, op in (("add", O.ADD), ("sub", O.SUB), ("neg", O.NEG), ("dbl", EC_DBL)) for ip in (False, True)])
def run_ec_ew(env, op, inplace):
    binary = op in (O.ADD, O.SUB)
    for n, k in ec_shapes():
        note = f"ec_ew op {op} n={n} phase {ec_phase(k)} inplace={inplace}"
        a, b = points(env, n, b"ew-a"), points(env, n, b"ew-b")
        want = host(env.scl.ec_ew(op, a, b if binary else None))
        A = R.Arena()
        wa = raw(A, "a", PT * n, 128, ec_phase(k), "inout" if inplace else "in", host(a))
        wb = raw(A, "b", PT * n, 128, ec_phase(k + 1), "in", host(b)) if binary else None
        wd = wa if inplace else raw(A, "dst", PT * n, 128, ec_phase(k + 2), "out")
        rc = env.lib.scl_hip_ec_ew(op, wd.ptr, wa.ptr, wb.ptr if wb else None, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 12), want, note)


@row("scl_hip_ec_equal", [("equal", {}, {})])
def run_ec_equal(env):
    for n, k in ec_shapes():
        note = f"ec_equal n={n} phase {ec_phase(k)} verdict phase {byte_phase(k)}"
        a = points(env, n, b"eq-a")
        b = env.scl.ec_ew(O.ADD, a, env.scl.ec_ew(O.NEG, points(env, n, b"eq-z")))
        b = env.scl.ec_ew(O.ADD, b, points(env, n, b"eq-z"))        # the same points under other coordinates
        b[n - 1] = points(env, 1, b"eq-other")[0]                   # the last pair differs
        want = host(env.scl.ec_equal(a, b))
        assert want.tolist() == [1] * (n - 1) + [0]
        A = R.Arena()
        wa = raw(A, "a", PT * n, 128, ec_phase(k), "in", host(a))
        wb = raw(A, "b", PT * n, 128, ec_phase(k + 1), "in", host(b))
        wd = raw(A, "eq", n, 16, byte_phase(k), "out")
        rc = env.lib.scl_hip_ec_equal(wd.ptr, wa.ptr, wb.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read()[0], want, note)


@row("scl_hip_ec_base_table", [("table", {}, {})])
def run_ec_base_table(env):
    g, h, h_pt = _tables(env.scl)
    nbytes = env.lib.scl_hip_ec_base_table_bytes()
    for k, (base, want) in enumerate([(env.scl.ec_generator(), g), (h_pt, h), (h_pt, h)]):
        note = f"ec_base_table phase {ec_phase(k)}"
        A = R.Arena()
        wt = raw(A, "table", nbytes, 128, ec_phase(k), "out")        # exactly scl_hip_ec_base_table_bytes()
        base = np.ascontiguousarray(base, dtype=np.uint64)
        rc = env.lib.scl_hip_ec_base_table(wt.ptr, base.ctypes.data, None)
        settle(env, A, rc, OK, note)
        same(wt.read()[0], host(want), note)


@row("scl_hip_ec_mul_base", [("mul_base", {}, {})])
def run_ec_mul_base(env):
    g = _tables(env.scl)[0]
    for n, k in ec_shapes():
        note = f"ec_mul_base n={n} phase {ec_phase(k)}"
        s = scalars(env, n, b"mb")
        want = host(env.scl.ec_mul_base(g, s))
        A = R.Arena()
        wg = table_win(A, "gtable", g, ec_phase(k + 1))
        ws = raw(A, "scalars", 32 * n, 128, ec_phase(k + 2), "in", host(s))
        wd = raw(A, "dst", PT * n, 128, ec_phase(k), "out")
        rc = env.lib.scl_hip_ec_mul_base(wd.ptr, wg.ptr, ws.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 12), want, note)


def pitched_points(env, A, name, pts, rows, cols, stride, ph):
    """[rows][cols][12] points as a window of rows `stride` points apart; also the same view on a plain allocation"""
    w = raw(A, name, PT * cols, 128, ph, "in", host(pts), rows=rows, pitch=PT * stride)
    wide = env.scl.ec_empty(rows, stride)
    wide[:, :cols] = pts
    return w, wide[:, :cols]


# m = 257 rows: LC_ROWS = 256 scalars are recoded per launch (ec_unit.hip:90, 174-177), the second launch ADDS its row into dst
@row("scl_hip_ec_lincomb", [("m%d" % m, dict(m=m, Ns=Ns), {}) for m, Ns in ((1, EC_N), (3, EC_N), (257, [2]))])
def run_ec_lincomb(env, m, Ns):
    for n, k in ec_shapes(Ns):
        stride = n + 3
        note = f"ec_lincomb m={m} n={n} row_stride {stride} phase {ec_phase(k)}"
        pts = points(env, m * n, b"lc").reshape(m, n, 12)
        s = scalars(env, m, b"lc-s")
        A = R.Arena()
        wp, plain = pitched_points(env, A, "points", pts, m, n, stride, ec_phase(k + 1))
        want = host(env.scl.ec_lincomb(plain, s))
        ws = raw(A, "scalars", 32 * m, 128, ec_phase(k + 2), "in", host(s))
        wd = raw(A, "dst", PT * n, 128, ec_phase(k), "out")
        rc = env.lib.scl_hip_ec_lincomb(wd.ptr, wp.ptr, stride, m, ws.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 12), want, note)


@row("scl_hip_ec_wire_pack", [("wire_pack", {}, {})])
def run_ec_wire_pack(env):
    for n, k in ec_shapes():
        note = f"ec_wire_pack n={n} phase {ec_phase(k)} image phase {byte_phase(k)}"
        pts = points(env, n, b"wp")
        pts[n - 1] = torch.tensor([0] * 4 + [1] + [0] * 7, dtype=torch.int64)     # some Y, Z = 0: infinity, 0x06 and zeros
        want = host(env.scl.ec_wire_pack(pts))
        A = R.Arena()
        wp = raw(A, "points", PT * n, 128, ec_phase(k), "in", host(pts))
        wd = raw(A, "images", 65 * n, 16, byte_phase(k), "out")     # 65 bytes per image: no alignment to speak of
        rc = env.lib.scl_hip_ec_wire_pack(wd.ptr, wp.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read().reshape(n, 65), want, note)


@row("scl_hip_ec_wire_unpack", [("wire_unpack", {}, {})])
def run_ec_wire_unpack(env):
    for n, k in ec_shapes():
        note = f"ec_wire_unpack n={n} phase {ec_phase(k)} image phase {byte_phase(k + 1)} status phase {byte_phase(k)}"
        img = env.scl.ec_wire_pack(points(env, n, b"wu"))
        img[n - 1, 0] = 0x01                                  # a compressed image in the last slot: status 1, infinity written
        want_p, want_s = env.scl.ec_wire_unpack(img)
        assert host(want_s).tolist() == [0] * (n - 1) + [1]
        A = R.Arena()
        wi = raw(A, "images", 65 * n, 16, byte_phase(k + 1), "in", host(img))
        wd = raw(A, "points", PT * n, 128, ec_phase(k), "out")
        wst = raw(A, "status", n, 16, byte_phase(k), "out")
        rc = env.lib.scl_hip_ec_wire_unpack(wd.ptr, wst.ptr, wi.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 12), host(want_p), note)
        same(wst.read()[0], host(want_s), note)


@row("scl_hip_ec_mul_two_base", [("mul_two_base", {}, {})])
def run_ec_mul_two_base(env):
    g, h, _ = _tables(env.scl)
    for n, k in ec_shapes():
        note = f"ec_mul_two_base n={n} phase {ec_phase(k)}"
        a, b = scalars(env, n, b"tb-a"), scalars(env, n, b"tb-b")
        want = host(env.scl.ec_mul_two_base(g, h, a, b))
        A = R.Arena()
        wg, wh = table_win(A, "gtable", g, ec_phase(k + 1)), table_win(A, "htable", h, ec_phase(k + 2))
        wa = raw(A, "a", 32 * n, 128, ec_phase(k + 1), "in", host(a))
        wb = raw(A, "b", 32 * n, 128, ec_phase(k + 2), "in", host(b))
        wd = raw(A, "dst", PT * n, 128, ec_phase(k), "out")
        rc = env.lib.scl_hip_ec_mul_two_base(wd.ptr, wg.ptr, wh.ptr, wa.ptr, wb.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 12), want, note)


# p = 257: the rows of M are recoded 256 scalars per launch as in ec_lincomb, the second launch adds into dst
@row("scl_hip_ec_matmul", [("rows%d-p%d" % (r, p), dict(rows=r, p=p, Ns=Ns), {})
                           for r, p, Ns in ((1, 1, EC_N), (3, 2, EC_N), (2, 257, [1]))])
def run_ec_matmul(env, rows, p, Ns):
    for cols, k in ec_shapes(Ns):
        dstride, rstride = cols + 3, cols + 5
        note = f"ec_matmul {rows} x {p} x {cols} dst_stride {dstride} row_stride {rstride} phase {ec_phase(k)}"
        pts = points(env, p * cols, b"mm").reshape(p, cols, 12)
        Mx = scalars(env, rows * p, b"mm-s").reshape(rows, p, 4)
        A = R.Arena()
        wp, plain = pitched_points(env, A, "points", pts, p, cols, rstride, ec_phase(k + 1))
        want = host(env.scl.ec_matmul(Mx, plain))
        wm = raw(A, "M", 32 * rows * p, 128, ec_phase(k + 2), "in", host(Mx))
        wd = raw(A, "dst", PT * cols, 128, ec_phase(k), "out", rows=rows, pitch=PT * dstride)
        rc = env.lib.scl_hip_ec_matmul(wd.ptr, dstride, wm.ptr, rows, p, wp.ptr, rstride, cols, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(rows, cols, 12), want, note)


@row("scl_hip_ec_mul", [("mul" + ("-inplace" if ip else ""), dict(inplace=ip), {}) for ip in (False, True)])
def run_ec_mul(env, inplace):
    for n, k in ec_shapes():
        note = f"ec_mul n={n} phase {ec_phase(k)} inplace={inplace}"
        pts, s = points(env, n, b"ml"), scalars(env, n, b"ml-s")
        want = host(env.scl.ec_mul(pts, s))
        A = R.Arena()
        wp = raw(A, "points", PT * n, 128, ec_phase(k + 1), "inout" if inplace else "in", host(pts))
        ws = raw(A, "scalars", 32 * n, 128, ec_phase(k + 2), "in", host(s))
        # the window-table scratch at exactly scl_hip_ec_mul_scratch_bytes(n): one slot more than promised fails
        wsc = raw(A, "scratch", env.lib.scl_hip_ec_mul_scratch_bytes(n), 128, ec_phase(k), "inout")
        wd = wp if inplace else raw(A, "dst", PT * n, 128, ec_phase(k), "out")
        rc = env.lib.scl_hip_ec_mul(wd.ptr, wp.ptr, ws.ptr, wsc.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 12), want, note)


# ---------------------------------------------------------------------------------------------- Feldman and Pedersen
@row("scl_hip_feldman_commit", [("t%d" % t, dict(t=t), {}) for t in (0, 1, 3)])
def run_feldman_commit(env, t):
    g = _tables(env.scl)[0]
    for N, k in ec_shapes():
        cstride, sstride = N + 3, N + 5
        note = f"feldman_commit t={t} N={N} commit_stride {cstride} share_stride {sstride} phase {ec_phase(k)}"
        sec, sh = scalars(env, N, b"fc-s"), scalars(env, max(t, 1) * N, b"fc-sh").reshape(max(t, 1), N, 4)[:t]
        want = host(env.scl.feldman_commit(g, sec, sh.contiguous(), t))
        A = R.Arena()
        wg = table_win(A, "gtable", g, ec_phase(k + 1))
        wsec = raw(A, "secrets", 32 * N, 128, ec_phase(k + 2), "in", host(sec))
        wsh = raw(A, "shares", 32 * N, 128, ec_phase(k + 1), "in", host(sh), rows=t, pitch=32 * sstride) if t else None
        wd = raw(A, "commit", PT * N, 128, ec_phase(k), "out", rows=t + 1, pitch=PT * cstride)
        rc = env.lib.scl_hip_feldman_commit(wd.ptr, cstride, wg.ptr, wsec.ptr, wsh.ptr if wsh else None, sstride, t, N, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(t + 1, N, 12), want, note)


def _sharing(env, N, t, n, tag):
    """a PRG sharing of N secrets over SECP256K1_SCALAR: (secrets [N][4], shares [n][N][4])"""
    sec = scalars(env, N, tag)
    return sec, env.scl.shamir_share_prg(SCALAR, sec, t, n, b"rz-vss-" + tag)


@row("scl_hip_feldman_verify", [("t%d" % t, dict(t=t), {}) for t in (1, 3)])
def run_feldman_verify(env, t):
    scl, g = env.scl, _tables(env.scl)[0]
    party = 2
    lam = scl.feldman_lambda(t, party + 1)
    for N, k in ec_shapes():
        cstride = N + 3
        note = f"feldman_verify t={t} N={N} commit_stride {cstride} phase {ec_phase(k)} verdict phase {byte_phase(k)}"
        sec, sh = _sharing(env, N, t, t + 2, b"fv")
        com = scl.feldman_commit(g, sec, sh, t)
        share = sh[party].clone()
        share[N - 1] = sec[N - 1]                             # the last share is wrong (the secret itself, not f(3))
        want = host(scl.feldman_verify(g, share, com, lam))
        assert want.tolist() == [1] * (N - 1) + [0]
        A = R.Arena()
        wg = table_win(A, "gtable", g, ec_phase(k + 1))
        wsh = raw(A, "share", 32 * N, 128, ec_phase(k + 2), "in", host(share))
        wc = raw(A, "commit", PT * N, 128, ec_phase(k + 1), "in", host(com), rows=t + 1, pitch=PT * cstride)
        wl = raw(A, "lambda", 32 * (t + 1), 128, ec_phase(k + 2), "in", host(lam))
        wsc = raw(A, "scratch", 2 * N * PT, 128, ec_phase(k), "inout")      # 2 N points (scl_hip.h), not one more
        wo = raw(A, "ok", N, 16, byte_phase(k), "out")
        rc = env.lib.scl_hip_feldman_verify(wo.ptr, wsh.ptr, wc.ptr, cstride, t, wl.ptr, wg.ptr, wsc.ptr, N, None)
        settle(env, A, rc, OK, note)
        same(wo.read()[0], want, note)


def _pedersen_sharing(env, N, t, n, tag):
    """({secret, blinding} [2][N][4], shares [2][n][N][4]) in shamir_share_prg_packed's layout"""
    sec = scalars(env, 2 * N, tag).reshape(2, N, 4)
    return sec, env.scl.shamir_share_prg_packed(SCALAR, sec, t, n, b"rz-ped-" + tag)


@row("scl_hip_pedersen_commit", [("t%d" % t, dict(t=t), {}) for t in (0, 1, 3)])
def run_pedersen_commit(env, t):
    g, h, _ = _tables(env.scl)
    n = t + 2
    for N, k in ec_shapes():
        cstride, secstride, sstride = N + 3, N + 2, N + 5
        note = f"pedersen_commit t={t} N={N} strides {cstride}/{secstride}/{sstride} phase {ec_phase(k)}"
        sec, sh = _pedersen_sharing(env, N, t, n, b"pc")
        want = host(env.scl.pedersen_commit(g, h, sec, sh, t))
        A = R.Arena()
        wg, wh = table_win(A, "gtable", g, ec_phase(k + 1)), table_win(A, "htable", h, ec_phase(k + 2))
        wsec = raw(A, "secrets", 32 * N, 128, ec_phase(k + 2), "in", host(sec), rows=2, pitch=32 * secstride)
        wsh = raw(A, "shares", 32 * N, 128, ec_phase(k + 1), "in", host(sh), rows=2 * n, pitch=32 * sstride)
        wd = raw(A, "commit", PT * N, 128, ec_phase(k), "out", rows=t + 1, pitch=PT * cstride)
        rc = env.lib.scl_hip_pedersen_commit(wd.ptr, cstride, wg.ptr, wh.ptr, wsec.ptr, secstride, wsh.ptr, sstride, t, n, N, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(t + 1, N, 12), want, note)


@row("scl_hip_pedersen_verify", [("t%d" % t, dict(t=t), {}) for t in (1, 3)])
def run_pedersen_verify(env, t):
    scl = env.scl
    g, h, _ = _tables(scl)
    party = 2
    lam = scl.feldman_lambda(t, party + 1)
    for N, k in ec_shapes():
        cstride = N + 3
        note = f"pedersen_verify t={t} N={N} commit_stride {cstride} phase {ec_phase(k)} verdict phase {byte_phase(k)}"
        sec, sh = _pedersen_sharing(env, N, t, t + 2, b"pv")
        com = scl.pedersen_commit(g, h, sec, sh, t)
        share, rand = sh[0, party].clone(), sh[1, party].clone()
        rand[N - 1] = sec[1, N - 1]                           # the last opening is wrong
        want = host(scl.pedersen_verify(g, h, share, rand, com, lam))
        assert want.tolist() == [1] * (N - 1) + [0]
        A = R.Arena()
        wg, wh = table_win(A, "gtable", g, ec_phase(k + 1)), table_win(A, "htable", h, ec_phase(k + 2))
        wsh = raw(A, "share", 32 * N, 128, ec_phase(k + 2), "in", host(share))
        wr = raw(A, "rand", 32 * N, 128, ec_phase(k), "in", host(rand))
        wc = raw(A, "commit", PT * N, 128, ec_phase(k + 1), "in", host(com), rows=t + 1, pitch=PT * cstride)
        wl = raw(A, "lambda", 32 * (t + 1), 128, ec_phase(k + 2), "in", host(lam))
        wsc = raw(A, "scratch", 2 * N * PT, 128, ec_phase(k), "inout")      # 2 N points (scl_hip.h), not one more
        wo = raw(A, "ok", N, 16, byte_phase(k), "out")
        rc = env.lib.scl_hip_pedersen_verify(wo.ptr, wsh.ptr, wr.ptr, wc.ptr, cstride, t, wl.ptr, wg.ptr, wh.ptr, wsc.ptr, N, None)
        settle(env, A, rc, OK, note)
        same(wo.read()[0], want, note)


# ---------------------------------------------------------------------------------------------- ECDSA
def digest_rows(env, n, tag):
    return torch.from_numpy(np.frombuffer(env.port.prg(b"rz-ecdsa-" + tag, [32 * n]), dtype=np.uint8).copy().reshape(n, 32)).cuda()


@row("scl_hip_ecdsa_conversion", [("conversion", {}, {})])
def run_ecdsa_conversion(env):
    for n, k in ec_shapes():
        note = f"ecdsa_conversion n={n} phase {ec_phase(k)}"
        pts = points(env, n, b"cv")
        want = host(env.scl.ecdsa_conversion(pts))
        A = R.Arena()
        wp = raw(A, "points", PT * n, 128, ec_phase(k + 1), "in", host(pts))
        wd = raw(A, "scalars", 32 * n, 128, ec_phase(k), "out")
        rc = env.lib.scl_hip_ecdsa_conversion(wd.ptr, wp.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 4), want, note)


def _signed(env, n, per_key, tag):
    """(sk [1 | n][4], pk [1 | n][12], nonces, digests, signatures) through the wrappers"""
    scl, g = env.scl, _tables(env.scl)[0]
    sk = scalars(env, n if per_key else 1, tag + b"-sk")
    pk = scl.ec_mul_base(g, sk)
    nonces, dg = scalars(env, n, tag + b"-k"), digest_rows(env, n, tag)
    return sk, pk, nonces, dg, scl.ecdsa_sign(g, sk, nonces, dg)


@row("scl_hip_ecdsa_sign", [("one-key", dict(per_key=False), {}), ("key-per-signature", dict(per_key=True), {})])
def run_ecdsa_sign(env, per_key):
    g = _tables(env.scl)[0]
    for n, k in ec_shapes():
        note = f"ecdsa_sign n={n} per_key={per_key} phase {ec_phase(k)}"
        sk, pk, nonces, dg, _ = _signed(env, n, per_key, b"sg")
        nonces[n - 1] = 0                                     # a zero nonce in the last lane: (0, 0) and the status word raised
        st = env.scl.ew_status_buffer()
        want = host(env.scl.ecdsa_sign(g, sk, nonces, dg, status=st))
        assert int(st.item()) == 1 and not want[n - 1].any()
        A = R.Arena()
        wg = table_win(A, "gtable", g, ec_phase(k + 1))
        wsk = raw(A, "sk", 32 * sk.shape[0], 128, ec_phase(k + 2), "in", host(sk))
        wk = raw(A, "nonces", 32 * n, 128, ec_phase(k + 1), "in", host(nonces))
        wdg = raw(A, "digests", 32 * n, 16, byte_phase(k), "in", host(dg))
        wst = raw(A, "status", 4, 16, (0, 4, 12)[k % 3], "inout", np.zeros(1, dtype=np.uint32))
        wd = raw(A, "sig", 64 * n, 128, ec_phase(k), "out")
        rc = env.lib.scl_hip_ecdsa_sign(wd.ptr, wg.ptr, wsk.ptr, 1 if per_key else 0, wk.ptr, wdg.ptr, wst.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wd.read(np.int64).reshape(n, 8), want, note)
        assert int(wst.read(np.uint32)[0, 0]) == 1, note


@row("scl_hip_ecdsa_verify", [("one-key", dict(per_key=False), {}), ("key-per-signature", dict(per_key=True), {})])
def run_ecdsa_verify(env, per_key):
    g = _tables(env.scl)[0]
    for n, k in ec_shapes():
        note = f"ecdsa_verify n={n} per_key={per_key} phase {ec_phase(k)} verdict phase {byte_phase(k)}"
        sk, pk, nonces, dg, sig = _signed(env, n, per_key, b"vf")
        sig[n - 1, 4:] = 0                                    # s == 0 in the last lane: verdict 2
        if n > 1:
            dg[0, 0] ^= 1                                     # another digest in the first: rejected
        want = host(env.scl.ecdsa_verify(g, pk, sig, dg))
        assert want.tolist() == ([0] + [1] * (n - 2) + [2] if n > 1 else [2])
        A = R.Arena()
        wg = table_win(A, "gtable", g, ec_phase(k + 1))
        wpk = raw(A, "pk", PT * pk.shape[0], 128, ec_phase(k + 2), "in", host(pk))
        wsig = raw(A, "sig", 64 * n, 128, ec_phase(k + 1), "in", host(sig))
        wdg = raw(A, "digests", 32 * n, 16, byte_phase(k + 1), "in", host(dg))
        wsc = raw(A, "scratch", env.lib.scl_hip_ec_mul_scratch_bytes(n), 128, ec_phase(k), "inout")   # exactly the documented size
        wo = raw(A, "verdict", n, 16, byte_phase(k), "out")
        rc = env.lib.scl_hip_ecdsa_verify(wo.ptr, wsig.ptr, wdg.ptr, wpk.ptr, 1 if per_key else 0, wg.ptr, wsc.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wo.read()[0], want, note)


@row("scl_hip_ecdsa_verify_base", [("one-signer", {}, {})])
def run_ecdsa_verify_base(env):
    scl, g = env.scl, _tables(env.scl)[0]
    for n, k in ec_shapes():
        note = f"ecdsa_verify_base n={n} phase {ec_phase(k)} verdict phase {byte_phase(k)}"
        sk, pk, nonces, dg, sig = _signed(env, n, False, b"vb")
        q = scl.ec_base_table(scl.to_host(pk)[0])
        sig[n - 1, 4:] = 0
        want = host(scl.ecdsa_verify_base(g, q, sig, dg))
        assert want.tolist() == [1] * (n - 1) + [2]
        A = R.Arena()
        wg, wq = table_win(A, "gtable", g, ec_phase(k + 1)), table_win(A, "qtable", q, ec_phase(k + 2))
        wsig = raw(A, "sig", 64 * n, 128, ec_phase(k + 1), "in", host(sig))
        wdg = raw(A, "digests", 32 * n, 16, byte_phase(k + 1), "in", host(dg))
        wo = raw(A, "verdict", n, 16, byte_phase(k), "out")
        rc = env.lib.scl_hip_ecdsa_verify_base(wo.ptr, wsig.ptr, wdg.ptr, wq.ptr, wg.ptr, n, None)
        settle(env, A, rc, OK, note)
        same(wo.read()[0], want, note)


# ---------------------------------------------------------------------------------------------- the test
ALL_CASES = [c for r in TABLE.values() for c in r.cases()]


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    import scl_amd
    port = O.Port()
    scl_amd.set_mont128_prime((1 << 128) - 159)
    port.mont128_set_prime((1 << 128) - 159)
    return Env(scl_amd, port)


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_no_write_outside_the_output_windows(env, case):
    """one row of TABLE at one (field, variant, knob): every shape and placement of the row through the raw C ABI"""
    try:
        for key, value in case.knobs.items():
            env.scl.set_tuning(key, value)
        TABLE[case.entry].run(env, **case.params)
    finally:
        for key in case.knobs:
            env.scl.set_tuning(key, KNOB_DEFAULTS[key])
