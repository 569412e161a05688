"""Aliasing tests: which operands of an entry point may share memory, and that every other overlap is refused.

The value tests pin WHAT every kernel computes and tests/test_gpu_redzones.py WHERE it writes; this file pins what happens when an
output buffer lies on an input.  include/scl_hip.h (Conventions) has the rule: an output may COINCIDE with an input -- the same
pointer and, for matrices, the same stride -- only where the entry point says so; any other overlap of an output with an input,
of two outputs, or of caller scratch with anything is SCL_ERR_BAD_ARG with both operands named in scl_hip_last_error(), before
anything is launched or written.  Overlap is judged on bounding spans (include/scl_hip/detail/span.hpp; its interval arithmetic
has a host test of its own, tests/cxx/span_overlap_check.cc).

ALIASING below is the contract as data: for every entry point that is a row of test_gpu_redzones.TABLE, a decision -- "permit"
or "refuse" -- for every (written *_dev parameter, other *_dev parameter) pair, with the words by which the header states it.
tests/test_aliasing_model.py (CPU) checks the table against the prototypes and the header's comments, so an entry point cannot be
added without deciding.  An alias is permitted only where every kernel the launcher can select reads the aliased operand at the
positions the same lane later writes, and before it writes them; refusing is the default.

Two kinds of test, both through the raw C ABI into a tests/redzone.py arena with the placement helpers of test_gpu_redzones:
* permitted aliases: every one the header lists, for every field and ring the entry point takes, at BATCH = 1, 2, 3, 255, 256, 257
  (EC_N = 1, 63, 64, 65 for points), both one-limb phases, and on the kernel paths the knobs of fuzz_abi.KNOBS reach -- for INV /
  DIV the chain lengths "inv_batch" -1 | 8 | 128 and the two-level form "inv_two_level" 4 | 8 at one tile and one tile plus one
  element.  Expected values: oracle_lib.Port for the field, ring and sharing calls; for the secp256k1 family the same entry point
  out of place (as test_gpu_redzones argues) with the two end lanes against the big-integer model of tests/secp256k1_model.py.
  The aliased window is `inout`, so arena.check() still holds everything else to its pattern.
* refusals: for every refused pair the exact alias, the output one element into the input and, where the input has rows, the
  output one row into it -- and for every PERMITTED pair the two near misses.  Each returns SCL_ERR_BAD_ARG, names both operands,
  and leaves the arena untouched with every window declared `in`: nothing was written.  (The operands hold the arena's pattern:
  a refusal reads none of them.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
import redzone as R
import test_gpu_redzones as G
from test_gpu_redzones import (BATCH, EC_N, FIELDS3, FIELDS6, FIELDS8, GF, KNOB_DEFAULTS, M61, M127, MONT128, OPNAME, PT, el, esz, fname,
                               host, knob_label, limbs, mat, place, placements, points, raw, rnd, same, scalars, settle, vec,
                               ec_phase, ec_shapes)

pytestmark = pytest.mark.gpu

OK, ERR_BAD_ARG = 0, 3
EC_DBL = G.EC_DBL


# ---------------------------------------------------------------------------------------------- the contract as data
def decide(outs, ins=(), permit=(), whole=()):
    """{(written operand, other operand): (decision, the header's words)} for every pair of one entry point.  `permit`: the pairs
    that may coincide; `whole`: written operands the header bars from "any other operand" in one phrase"""
    table = {}
    for o in outs:
        for x in list(outs) + list(ins):
            if x == o:
                continue
            if (o, x) in permit:
                table[(o, x)] = ("permit", f"{o} may be {x}")
            elif o in whole:
                table[(o, x)] = ("refuse", f"{o} must not overlap any other operand")
            elif x in whole:
                table[(o, x)] = ("refuse", f"{x} must not overlap any other operand")
            else:
                table[(o, x)] = ("refuse", f"{o} must not overlap {x}")
    return table


def sole(name):
    return f"{name} is the only device operand"


_EW_OK = {("dst_dev", "a_dev"), ("dst_dev", "b_dev")}
ALIASING = {
    "scl_hip_ew": decide(["dst_dev"], ["a_dev", "b_dev"], permit=_EW_OK),
    "scl_hip_ew_status": decide(["dst_dev", "status_dev"], ["a_dev", "b_dev"], permit=_EW_OK, whole=["status_dev"]),
    "scl_hip_scalar_mul": decide(["dst_dev"], ["a_dev"], permit={("dst_dev", "a_dev")}),
    "scl_hip_prg_blocks": decide(["dst_dev"]),
    "scl_hip_from_bytes": decide(["dst_dev"], ["src_dev"], permit={("dst_dev", "src_dev")}),     # (full-width elements only)
    "scl_hip_vector_random": decide(["dst_dev"]),
    "scl_hip_shamir_share": decide(["shares_dev"], ["secrets_dev", "coeffs_dev"], whole=["shares_dev"]),
    "scl_hip_shamir_share_prg": decide(["shares_dev"], ["secrets_dev"]),
    "scl_hip_shamir_share_prg_packed": decide(["shares_dev"], ["secrets_dev"]),
    "scl_hip_shamir_recover": decide(["out_dev"], ["shares_dev"]),
    "scl_hip_shamir_recover_detect": decide(["out_dev", "status_dev"], ["shares_dev"], whole=["out_dev", "status_dev"]),
    "scl_hip_shamir_recover_correct": decide(["f_dev", "e_dev", "status_dev", "nerr_dev"], ["shares_dev"],
                                             whole=["f_dev", "e_dev", "status_dev", "nerr_dev"]),
    "scl_hip_additive_share": decide(["shares_dev"], ["secrets_dev", "rnd_dev"], permit={("shares_dev", "rnd_dev")}),
    "scl_hip_additive_share_prg": decide(["shares_dev"], ["secrets_dev"]),
    "scl_hip_additive_recover": decide(["out_dev"], ["shares_dev"]),
    "scl_hip_vandermonde": decide(["V_dev"]),
    "scl_hip_matmul": decide(["C_dev"], ["A_dev", "B_dev"], whole=["C_dev"]),
    "scl_hip_aos_to_soa": decide(["soa_dev"], ["aos_dev"]),
    "scl_hip_soa_to_aos": decide(["aos_dev"], ["soa_dev"]),
    "scl_hip_wire_pack": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_frame_pack": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_wire_unpack": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_frame_unpack": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_wire_pack_matrix": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_frame_pack_matrix": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_wire_unpack_matrix": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_stream_copy": decide(["dst_dev"], ["src_dev"]),
    "scl_hip_sha256": decide(["digests_dev"], ["msgs_dev"]),
    "scl_hip_merkle_leaves": decide(["digests_dev"], ["a_dev"]),
    "scl_hip_merkle_build": decide(["tree_dev"], ["leaf_digests_dev"], permit={("tree_dev", "leaf_digests_dev")}),
    "scl_hip_merkle_root": decide(["roots_dev"], ["leaf_digests_dev"]),
    "scl_hip_merkle_paths": decide(["path_dev"], ["tree_dev", "leaf_index_dev", "tree_index_dev"], whole=["path_dev"]),
    "scl_hip_merkle_verify": decide(["ok_dev"], ["leaf_digests_dev", "leaf_index_dev", "path_dev", "roots_dev", "root_index_dev"],
                                    whole=["ok_dev"]),
    "scl_hip_ec_ew": decide(["dst_dev"], ["a_dev", "b_dev"], permit=_EW_OK),
    "scl_hip_ec_equal": decide(["eq_dev"], ["a_dev", "b_dev"], whole=["eq_dev"]),
    "scl_hip_ec_base_table": decide(["table_dev"]),
    "scl_hip_ec_mul_base": decide(["dst_dev"], ["table_dev", "scalars_dev"], whole=["dst_dev"]),
    "scl_hip_ec_lincomb": decide(["dst_dev"], ["points_dev", "scalars_dev"], whole=["dst_dev"]),
    "scl_hip_ec_wire_pack": decide(["dst_dev"], ["points_dev"]),
    "scl_hip_ec_wire_unpack": decide(["points_dev", "status_dev"], ["src_dev"], whole=["points_dev", "status_dev"]),
    "scl_hip_feldman_commit": decide(["commit_dev"], ["gtable_dev", "secrets_dev", "shares_dev"], whole=["commit_dev"]),
    "scl_hip_feldman_verify": decide(["ok_dev", "scratch_points_dev"], ["share_dev", "commit_dev", "lambda_dev", "gtable_dev"],
                                     whole=["ok_dev", "scratch_points_dev"]),
    "scl_hip_ec_mul_two_base": decide(["dst_dev"], ["gtable_dev", "htable_dev", "a_dev", "b_dev"], whole=["dst_dev"]),
    "scl_hip_ec_matmul": decide(["dst_dev"], ["M_dev", "points_dev"], whole=["dst_dev"]),
    "scl_hip_pedersen_commit": decide(["commit_dev"], ["gtable_dev", "htable_dev", "secrets_dev", "shares_dev"], whole=["commit_dev"]),
    "scl_hip_pedersen_verify": decide(["ok_dev", "scratch_points_dev"],
                                      ["share_dev", "rand_dev", "commit_dev", "lambda_dev", "gtable_dev", "htable_dev"],
                                      whole=["ok_dev", "scratch_points_dev"]),
    "scl_hip_ec_mul": decide(["dst_dev", "scratch_dev"], ["points_dev", "scalars_dev"], permit={("dst_dev", "points_dev")},
                             whole=["scratch_dev"]),
    "scl_hip_ecdsa_conversion": decide(["scalars_dev"], ["points_dev"]),
    "scl_hip_ecdsa_sign": decide(["sig_dev", "status_dev"], ["gtable_dev", "sk_dev", "nonces_dev", "digests_dev"],
                                 whole=["sig_dev", "status_dev"]),
    "scl_hip_ecdsa_verify": decide(["verdict_dev", "scratch_dev"], ["sig_dev", "digests_dev", "pk_dev", "gtable_dev"],
                                   whole=["verdict_dev", "scratch_dev"]),
    "scl_hip_ecdsa_verify_base": decide(["verdict_dev"], ["sig_dev", "digests_dev", "qtable_dev", "gtable_dev"], whole=["verdict_dev"]),
}
# entry points with one device operand: what the header says in place of a rule
SOLE = {"scl_hip_prg_blocks": sole("dst_dev"), "scl_hip_vector_random": sole("dst_dev"), "scl_hip_vandermonde": sole("V_dev"),
        "scl_hip_ec_base_table": sole("table_dev")}


# ---------------------------------------------------------------------------------------------- refusals
class Op:
    """one device operand of a refusal case: rows x nbytes bytes `pitch` apart, `step` bytes per element, `al` its alignment"""

    def __init__(self, nbytes, step, al, rows=1, pitch=None):
        self.nbytes, self.step, self.al, self.rows, self.pitch = nbytes, step, al, rows, pitch if pitch is not None else nbytes

    @property
    def span(self):
        return (self.rows - 1) * self.pitch + self.nbytes


N, PITCH = 6, 8        # elements per row and the row pitch in elements: every pitch in bytes is a multiple of 16


def fv(f, n):
    e = esz(f)
    return Op(n * e, e, 8 if limbs(f) == 1 else 16)


def fm(f, rows, cols=N, pitch=PITCH):
    e = esz(f)
    return Op(cols * e, e, 8 if limbs(f) == 1 else 16, rows, pitch * e)


def bv(n, e, al=None):
    return Op(n * e, e, al if al is not None else (16 if e % 16 == 0 else 4 if e == 4 else 8 if e == 8 else 1))


def pv(n):
    return Op(n * PT, PT, 16)


def pm(rows, cols, pitch=PITCH):
    return Op(cols * PT, PT, 16, rows, pitch * PT)


SEED = b"alias-seed"
KEEP = []              # host arrays a call's pointer arguments refer to


def hostv(f, n):
    a = np.ones(max(n, 1) * limbs(f), dtype=np.uint64)
    KEEP.append(a)
    return a.ctypes.data


def spec(entry, f, lib):
    """(operands by header name, call(pointers by name) -> status) of one valid call of `entry`"""
    name = entry[len("scl_hip_"):]
    fn = getattr(lib, entry)
    e = esz(f) if f is not None else 0
    tb = lib.scl_hip_ec_base_table_bytes()
    table = Op(tb, 16, 16)
    sz = C.c_size_t
    cnt, cnt2 = sz(0), sz(0)
    if name in ("ew", "ew_status"):
        ops = dict(dst_dev=fv(f, N), a_dev=fv(f, N), b_dev=fv(f, N))
        if name == "ew":
            return ops, lambda p: fn(f, O.ADD, p["dst_dev"], p["a_dev"], p["b_dev"], N, None)
        ops["status_dev"] = bv(1, 4)
        return ops, lambda p: fn(f, O.ADD, p["dst_dev"], p["a_dev"], p["b_dev"], N, p["status_dev"], None)
    if name == "scalar_mul":
        return dict(dst_dev=fv(f, N), a_dev=fv(f, N)), lambda p: fn(f, p["dst_dev"], p["a_dev"], hostv(f, 1), N, None)
    if name == "from_bytes":
        bs = O.byte_size(f)
        return dict(dst_dev=fv(f, N), src_dev=Op(N * bs, bs, 1)), lambda p: fn(f, p["dst_dev"], p["src_dev"], N, None)
    if name == "shamir_share":
        return (dict(shares_dev=fm(f, 3), secrets_dev=fv(f, N), coeffs_dev=fm(f, 2)),
                lambda p: fn(f, p["shares_dev"], PITCH, p["secrets_dev"], p["coeffs_dev"], PITCH, N, 2, 3, None, None))
    if name == "shamir_share_prg":
        return (dict(shares_dev=fm(f, 3), secrets_dev=fv(f, N)),
                lambda p: fn(f, p["shares_dev"], PITCH, p["secrets_dev"], N, 2, 3, SEED, len(SEED), 0, None))
    if name == "shamir_share_prg_packed":
        return (dict(shares_dev=fm(f, 6), secrets_dev=fm(f, 2)),
                lambda p: fn(f, p["shares_dev"], PITCH, p["secrets_dev"], PITCH, N, 2, 3, 2, SEED, len(SEED), 0, None))
    if name == "shamir_recover":
        return (dict(out_dev=fv(f, N), shares_dev=fm(f, 3)),
                lambda p: fn(f, p["out_dev"], p["shares_dev"], PITCH, hostv(f, 3), 3, N, None))
    if name == "shamir_recover_detect":
        return (dict(out_dev=fv(f, N), status_dev=bv(N, 1), shares_dev=fm(f, 5)),
                lambda p: fn(f, p["out_dev"], p["status_dev"], p["shares_dev"], PITCH, 5, N, 2, 2, None, None, C.byref(cnt), None))
    if name == "shamir_recover_correct":
        return (dict(f_dev=fm(f, 7), e_dev=fm(f, 3), status_dev=bv(N, 1), nerr_dev=bv(N, 4), shares_dev=fm(f, 7)),
                lambda p: fn(f, p["f_dev"], PITCH, p["e_dev"], PITCH, p["status_dev"], p["nerr_dev"], p["shares_dev"], PITCH, 7, N, None,
                             C.byref(cnt), C.byref(cnt2), None))
    if name == "additive_share":
        return (dict(shares_dev=fm(f, 3), secrets_dev=fv(f, N), rnd_dev=fm(f, 2)),
                lambda p: fn(f, p["shares_dev"], PITCH, p["secrets_dev"], p["rnd_dev"], PITCH, N, 3, None))
    if name == "additive_share_prg":
        return (dict(shares_dev=fm(f, 3), secrets_dev=fv(f, N)),
                lambda p: fn(f, p["shares_dev"], PITCH, p["secrets_dev"], N, 3, SEED, len(SEED), 0, None))
    if name == "additive_recover":
        return dict(out_dev=fv(f, N), shares_dev=fm(f, 3)), lambda p: fn(f, p["out_dev"], p["shares_dev"], PITCH, 3, N, None)
    if name == "matmul":
        return (dict(C_dev=fm(f, 4), A_dev=fm(f, 4, 4), B_dev=fm(f, 4)),
                lambda p: fn(f, p["C_dev"], PITCH, p["A_dev"], PITCH, p["B_dev"], PITCH, 4, 4, N, None))
    if name == "aos_to_soa":
        return dict(soa_dev=fm(f, 3), aos_dev=fv(f, 3 * N)), lambda p: fn(f, p["soa_dev"], PITCH, p["aos_dev"], N, 3, None)
    if name == "soa_to_aos":
        return dict(aos_dev=fv(f, 3 * N), soa_dev=fm(f, 3)), lambda p: fn(f, p["aos_dev"], p["soa_dev"], PITCH, N, 3, None)
    if name in ("wire_pack", "frame_pack"):
        head = 4 if name == "wire_pack" else 8
        return dict(dst_dev=Op(head + N * e, 4, 4), src_dev=fv(f, N)), lambda p: fn(f, p["dst_dev"], p["src_dev"], N, None)
    if name in ("wire_pack_matrix", "frame_pack_matrix"):
        head = 12 if name == "wire_pack_matrix" else 16
        return (dict(dst_dev=Op(head + 3 * 4 * e, 4, 4), src_dev=fm(f, 3, 4)),
                lambda p: fn(f, p["dst_dev"], p["src_dev"], PITCH, 3, 4, None))
    if name in ("wire_unpack", "frame_unpack"):
        nb = (4 if name == "wire_unpack" else 8) + N * e
        return (dict(dst_dev=fv(f, N), src_dev=Op(nb, 4, 4)),
                lambda p: fn(f, p["dst_dev"], N, p["src_dev"], nb, C.byref(cnt), None))
    if name == "wire_unpack_matrix":
        nb = 12 + 3 * 4 * e
        return (dict(dst_dev=fm(f, 3, PITCH), src_dev=Op(nb, 4, 4)),      # the destination is capacity_rows rows of ld elements
                lambda p: fn(f, p["dst_dev"], PITCH, 3, p["src_dev"], nb, C.byref(cnt), C.byref(cnt2), None))
    if name == "stream_copy":
        return dict(dst_dev=bv(6, 16), src_dev=bv(6, 16)), lambda p: fn(p["dst_dev"], p["src_dev"], 96, None)
    if name == "sha256":
        return (dict(digests_dev=bv(4, 32), msgs_dev=Op(10, 1, 1, 4, 16)),
                lambda p: fn(p["digests_dev"], p["msgs_dev"], 10, 16, 4, None))
    if name == "merkle_leaves":
        return (dict(digests_dev=bv(12, 32), a_dev=fm(f, 3, 4)),
                lambda p: fn(f, p["digests_dev"], p["a_dev"], PITCH, 3, 4, None))
    if name == "merkle_build":
        return (dict(tree_dev=Op(lib.scl_hip_merkle_tree_bytes(4, 2), 32, 16), leaf_digests_dev=bv(8, 32)),
                lambda p: fn(p["tree_dev"], p["leaf_digests_dev"], 4, 2, None))
    if name == "merkle_root":
        return dict(roots_dev=bv(2, 32), leaf_digests_dev=bv(8, 32)), lambda p: fn(p["roots_dev"], p["leaf_digests_dev"], 4, 2, None)
    if name == "merkle_paths":
        return (dict(path_dev=bv(6, 32), tree_dev=Op(lib.scl_hip_merkle_tree_bytes(4, 2), 32, 16), leaf_index_dev=bv(3, 8),
                     tree_index_dev=bv(3, 8)),
                lambda p: fn(p["path_dev"], p["tree_dev"], 4, 2, p["leaf_index_dev"], p["tree_index_dev"], 0, 3, None))
    if name == "merkle_verify":
        return (dict(ok_dev=bv(3, 1), leaf_digests_dev=bv(3, 32), leaf_index_dev=bv(3, 8), path_dev=bv(6, 32), roots_dev=bv(2, 32),
                     root_index_dev=bv(3, 8)),
                lambda p: fn(p["ok_dev"], p["leaf_digests_dev"], p["leaf_index_dev"], 0, p["path_dev"], 2, p["roots_dev"],
                             p["root_index_dev"], 2, 3, None))
    n = 3
    if name == "ec_ew":
        return dict(dst_dev=pv(n), a_dev=pv(n), b_dev=pv(n)), lambda p: fn(O.ADD, p["dst_dev"], p["a_dev"], p["b_dev"], n, None)
    if name == "ec_equal":
        return dict(eq_dev=bv(n, 1), a_dev=pv(n), b_dev=pv(n)), lambda p: fn(p["eq_dev"], p["a_dev"], p["b_dev"], n, None)
    if name == "ec_mul_base":
        return (dict(dst_dev=pv(n), table_dev=table, scalars_dev=bv(n, 32)),
                lambda p: fn(p["dst_dev"], p["table_dev"], p["scalars_dev"], n, None))
    if name == "ec_lincomb":
        return (dict(dst_dev=pv(n), points_dev=pm(2, n), scalars_dev=bv(2, 32)),
                lambda p: fn(p["dst_dev"], p["points_dev"], PITCH, 2, p["scalars_dev"], n, None))
    if name == "ec_wire_pack":
        return dict(dst_dev=Op(65 * n, 65, 1), points_dev=pv(n)), lambda p: fn(p["dst_dev"], p["points_dev"], n, None)
    if name == "ec_wire_unpack":
        return (dict(points_dev=pv(n), status_dev=bv(n, 1), src_dev=Op(65 * n, 65, 1)),
                lambda p: fn(p["points_dev"], p["status_dev"], p["src_dev"], n, None))
    if name == "feldman_commit":
        return (dict(commit_dev=pm(3, n), gtable_dev=table, secrets_dev=bv(n, 32), shares_dev=Op(32 * n, 32, 16, 2, 32 * PITCH)),
                lambda p: fn(p["commit_dev"], PITCH, p["gtable_dev"], p["secrets_dev"], p["shares_dev"], PITCH, 2, n, None))
    if name == "feldman_verify":
        return (dict(ok_dev=bv(n, 1), share_dev=bv(n, 32), commit_dev=pm(3, n), lambda_dev=bv(3, 32), gtable_dev=table,
                     scratch_points_dev=pv(2 * n)),
                lambda p: fn(p["ok_dev"], p["share_dev"], p["commit_dev"], PITCH, 2, p["lambda_dev"], p["gtable_dev"],
                             p["scratch_points_dev"], n, None))
    if name == "ec_mul_two_base":
        return (dict(dst_dev=pv(n), gtable_dev=table, htable_dev=table, a_dev=bv(n, 32), b_dev=bv(n, 32)),
                lambda p: fn(p["dst_dev"], p["gtable_dev"], p["htable_dev"], p["a_dev"], p["b_dev"], n, None))
    if name == "ec_matmul":
        return (dict(dst_dev=pm(2, n), M_dev=bv(4, 32), points_dev=pm(2, n)),
                lambda p: fn(p["dst_dev"], PITCH, p["M_dev"], 2, 2, p["points_dev"], PITCH, n, None))
    if name == "pedersen_commit":
        return (dict(commit_dev=pm(3, n), gtable_dev=table, htable_dev=table, secrets_dev=Op(32 * n, 32, 16, 2, 32 * PITCH),
                     shares_dev=Op(32 * n, 32, 16, 8, 32 * PITCH)),
                lambda p: fn(p["commit_dev"], PITCH, p["gtable_dev"], p["htable_dev"], p["secrets_dev"], PITCH, p["shares_dev"], PITCH,
                             2, 4, n, None))
    if name == "pedersen_verify":
        return (dict(ok_dev=bv(n, 1), share_dev=bv(n, 32), rand_dev=bv(n, 32), commit_dev=pm(3, n), lambda_dev=bv(3, 32),
                     gtable_dev=table, htable_dev=table, scratch_points_dev=pv(2 * n)),
                lambda p: fn(p["ok_dev"], p["share_dev"], p["rand_dev"], p["commit_dev"], PITCH, 2, p["lambda_dev"], p["gtable_dev"],
                             p["htable_dev"], p["scratch_points_dev"], n, None))
    scratch = Op(lib.scl_hip_ec_mul_scratch_bytes(n), PT, 16)
    if name == "ec_mul":
        return (dict(dst_dev=pv(n), points_dev=pv(n), scalars_dev=bv(n, 32), scratch_dev=scratch),
                lambda p: fn(p["dst_dev"], p["points_dev"], p["scalars_dev"], p["scratch_dev"], n, None))
    if name == "ecdsa_conversion":
        return dict(scalars_dev=bv(n, 32), points_dev=pv(n)), lambda p: fn(p["scalars_dev"], p["points_dev"], n, None)
    if name == "ecdsa_sign":
        return (dict(sig_dev=bv(n, 64), gtable_dev=table, sk_dev=bv(n, 32), nonces_dev=bv(n, 32), digests_dev=bv(n, 32),
                     status_dev=bv(1, 4)),
                lambda p: fn(p["sig_dev"], p["gtable_dev"], p["sk_dev"], 1, p["nonces_dev"], p["digests_dev"], p["status_dev"], n, None))
    if name == "ecdsa_verify":
        return (dict(verdict_dev=bv(n, 1), sig_dev=bv(n, 64), digests_dev=bv(n, 32), pk_dev=pv(n), gtable_dev=table, scratch_dev=scratch),
                lambda p: fn(p["verdict_dev"], p["sig_dev"], p["digests_dev"], p["pk_dev"], 1, p["gtable_dev"], p["scratch_dev"], n, None))
    if name == "ecdsa_verify_base":
        return (dict(verdict_dev=bv(n, 1), sig_dev=bv(n, 64), digests_dev=bv(n, 32), qtable_dev=table, gtable_dev=table),
                lambda p: fn(p["verdict_dev"], p["sig_dev"], p["digests_dev"], p["qtable_dev"], p["gtable_dev"], n, None))
    raise KeyError(entry)


RING = O.Z2K(62)
NO_FIELD = {"stream_copy", "sha256", "merkle_build", "merkle_root", "merkle_paths", "merkle_verify"}
WITH_RINGS = {"ew", "ew_status", "scalar_mul", "from_bytes", "additive_share", "additive_share_prg", "additive_recover", "matmul",
              "aos_to_soa", "soa_to_aos"}


def fields_of(entry):
    """a one-limb, a 16-byte and a 32-byte field (and a ring where the entry point takes rings); None where it takes no field"""
    name = entry[len("scl_hip_"):]
    if name in NO_FIELD or name.startswith(("ec_", "ecdsa_", "feldman_", "pedersen_")):
        return [None]
    return FIELDS3 + ([RING] if name in WITH_RINGS else [])


REFUSALS = [(entry, o, x, f, kind) for entry, pairs in ALIASING.items() for (o, x), (kind, _) in pairs.items() for f in fields_of(entry)]


def offsets(o, x, kind):
    """(label, bytes) of where the output goes relative to the input.  One element in: a whole number of the input's elements,
    rounded up to the output's alignment (none where that already leaves the input); one row in: where the input has rows"""
    out = [] if kind == "permit" else [("exact", 0)]
    k = -(-max(x.step, 1) // o.al) * o.al
    if k < x.span:
        out.append(("one element in", k))
    if x.rows > 1:
        out.append(("one row in", x.pitch))
    return out


@pytest.mark.parametrize("entry,o,x,f,kind", REFUSALS,
                         ids=[f"{e[len('scl_hip_'):]}-{o}-on-{x}" + (f"-{fname(f)}" if f is not None else "") + ("-near-miss" if k == "permit" else "")
                              for e, o, x, f, k in REFUSALS])
def test_an_overlap_the_header_does_not_permit_is_refused_before_anything_is_written(env, entry, o, x, f, kind):
    ops, call = spec(entry, f, env.lib)
    places = offsets(ops[o], ops[x], kind)
    assert places, "no placement"
    for label, off in places:
        note = f"{entry} {o} on {x} ({label})" + (f" {fname(f)}" if f is not None else "")
        A = R.Arena()
        win = {name: A.window(name, op.nbytes, 128, 0, rows=op.rows, pitch_bytes=op.pitch, kind="in") for name, op in ops.items()}
        p = {name: w.ptr for name, w in win.items()}
        p[o] = win[x].ptr + off
        assert p[o] % ops[o].al == 0, note
        rc = call(p)
        msg = env.lib.scl_hip_last_error().decode()
        assert rc == ERR_BAD_ARG, f"{note}: status {rc} ({msg})"
        assert o in msg and x in msg and "overlaps" in msg, f"{note}: {msg!r} does not name both operands"
        A.check()                                             # every window is `in`: nothing was written anywhere


# ---------------------------------------------------------------------------------------------- the named shapes
def test_matmul_onto_its_right_factor_is_refused_on_either_kernels_shape(env):
    """x <- M x with C == B, M == K and ldc == ldb: (20, 20, 300) is k_matmul's shape and (9, 9, 300) k_matmul_thin's once the
    columns reach "matmul_lds_min" -- the first returned 4800 wrong elements of 6000 before the refusal, the second none
    (docs/kernels/r1_r4_matrix_layout_wire.md) -- and the tiled kernel's otherwise.  Refused whichever kernel the knobs select"""
    f = M61
    for knobs in ({}, {"mfma": -1, "matmul_lds_min": 1024}, {"mfma": -1}):      # (1024: fuzz_abi.KNOBS; below it the tiled kernel)
        try:
            for k, v in knobs.items():
                env.scl.set_tuning(k, v)
            for M, K, Nc in ((20, 20, 300), (9, 9, 300), (20, 20, 1025), (9, 9, 1025)):
                note = f"matmul C == B at ({M}, {K}, {Nc}) knobs {knobs}"
                A = R.Arena()
                wa = mat(A, "A", f, M, K, K, 0, "in", rnd(env, f, M * K, b"mm-a").reshape(M, K, 1))
                wb = mat(A, "B", f, K, Nc, Nc, 0, "in", rnd(env, f, K * Nc, b"mm-b").reshape(K, Nc, 1))
                rc = env.lib.scl_hip_matmul(f, wb.ptr, Nc, wa.ptr, K, wb.ptr, Nc, M, K, Nc, None)
                msg = env.lib.scl_hip_last_error().decode()
                assert rc == ERR_BAD_ARG and "C_dev" in msg and "B_dev" in msg, f"{note}: status {rc} ({msg})"
                rc = env.lib.scl_hip_matmul(f, wa.ptr, K, wa.ptr, K, wb.ptr, Nc, M, K, K, None)      # C == A
                msg = env.lib.scl_hip_last_error().decode()
                assert rc == ERR_BAD_ARG and "C_dev" in msg and "A_dev" in msg, f"{note}: status {rc} ({msg})"
                A.check()
        finally:
            for k in knobs:
                env.scl.set_tuning(k, KNOB_DEFAULTS[k])


def test_ec_lincomb_onto_a_later_point_row_is_refused(env):
    """m = 257 rows take a second launch that ADDS row 256 into dst (LC_ROWS = 256, ec_unit.hip): a dst lying on row 256 would be
    read after the first launch had overwritten it.  The header always said "must not overlap"; now the call does"""
    m, n, stride = 257, 2, 2
    A = R.Arena()
    wp = raw(A, "points", PT * n, 128, 0, "in", rows=m, pitch=PT * stride)
    ws = raw(A, "scalars", 32 * m, 128, 0, "in")
    for row in (256, 0, 100):
        rc = env.lib.scl_hip_ec_lincomb(wp.ptr + row * stride * PT, wp.ptr, stride, m, ws.ptr, n, None)
        msg = env.lib.scl_hip_last_error().decode()
        assert rc == ERR_BAD_ARG and "dst_dev" in msg and "points_dev" in msg, f"dst on row {row}: status {rc} ({msg})"
    A.check()


def test_operands_that_only_touch_are_accepted(env):
    """the output starting at the very byte the input ends on (and the other way round) is no overlap: one buffer cut in two"""
    f, n = M61, 257
    a0, b0, want0 = G.ew_ref(env, f, O.ADD)
    A = R.Arena()
    w = A.window("both", 2 * n * 8, 16, 0, kind="inout")
    wb = vec(A, "b", f, n, 0, "in", b0[:n])
    for dst_first in (False, True):
        w.view[0, (n * 8 if dst_first else 0):(2 * n * 8 if dst_first else n * 8)].copy_(
            torch.from_numpy(a0[:n].view(np.uint8).reshape(-1).copy()).to(w.view.device))
        pa, pd = (w.ptr + n * 8, w.ptr) if dst_first else (w.ptr, w.ptr + n * 8)
        rc = env.lib.scl_hip_ew(f, O.ADD, pd, pa, wb.ptr, n, None)
        settle(env, A, rc, OK, f"touching halves, dst first = {dst_first}")
        got = w.read(np.uint64).reshape(2 * n, 1)
        same(got[:n] if dst_first else got[n:], want0[:n], "touching halves")


def test_empty_operands_overlap_nothing(env):
    """n == 0 / N == 0: SCL_OK whatever the pointers are, one address for all of them included"""
    A = R.Arena()
    w = vec(A, "x", M61, 4, 0, "in")
    lib = env.lib
    assert lib.scl_hip_ew(M61, O.ADD, w.ptr, w.ptr + 8, w.ptr + 8, 0, None) == OK
    assert lib.scl_hip_matmul(M61, w.ptr, 4, w.ptr, 4, w.ptr, 4, 0, 2, 2, None) == OK
    assert lib.scl_hip_shamir_recover(M61, w.ptr, w.ptr, 4, None, 3, 0, None) == OK
    assert lib.scl_hip_ec_lincomb(w.ptr, w.ptr, 1, 2, w.ptr, 0, None) == OK
    assert lib.scl_hip_sha256(w.ptr, w.ptr, 8, 8, 0, None) == OK
    A.check()


# ---------------------------------------------------------------------------------------------- permitted aliases: element-wise
_REF = {}
NMAX = 32769           # GF(2^128) chains of 128 in 256-thread workgroups: one tile is 32768 elements


def ew_operands(env, f, op):
    """a, b (both invertible: either may be the divisor, and a == b must be too) and nothing else, NMAX elements, once per field"""
    if f not in _REF:
        a, b = rnd(env, f, NMAX, b"al-a"), rnd(env, f, NMAX, b"al-b")
        for t in (a, b):
            if O.is_ring(f):
                t[:, 0] |= np.uint64(1)
            else:
                t[(t == 0).all(axis=1)] = env.port.from_int(f, 1)
        _REF[f] = (a, b)
    return _REF[f]


def ew_want(env, f, op, alias, n):
    key = (f, op, alias, n)
    if key not in _REF:
        a, b = ew_operands(env, f, op)
        a, b = a[:n], (a[:n] if alias in ("a=b", "all") else b[:n])
        _REF[key] = np.asarray(env.port.ew(f, op, a, b if op in (O.ADD, O.SUB, O.MUL, O.DIV) else None))
    return _REF[key]


ALIASES = ("dst=a", "dst=b", "a=b", "all")


def run_ew_alias(env, call, with_status, f, op, alias, shapes):
    binary = op in (O.ADD, O.SUB, O.MUL, O.DIV)
    a0, b0 = ew_operands(env, f, op)
    nmax = max(n for n, _ in shapes)
    want0 = ew_want(env, f, op, alias, nmax)
    for n, pi in shapes:
        note = f"{fname(f)} {OPNAME.get(op, 'sub')} {alias} N={n} placement {place(f, pi)}"
        A = R.Arena()
        if alias == "dst=a":
            wa = vec(A, "a", f, n, pi, "inout", a0[:n])
            wb = vec(A, "b", f, n, pi, "in", b0[:n]) if binary else None
            wd = wa
        elif alias == "dst=b":
            wa = vec(A, "a", f, n, pi, "in", a0[:n])
            wb = vec(A, "b", f, n, pi, "inout", b0[:n])
            wd = wb
        elif alias == "a=b":
            wa = wb = vec(A, "a", f, n, pi, "in", a0[:n])
            wd = vec(A, "dst", f, n, pi, "out")
        else:
            wa = wb = wd = vec(A, "a", f, n, pi, "inout", a0[:n])
        args = [f, op, wd.ptr, wa.ptr, wb.ptr if wb else None, n]
        if with_status:
            ws = raw(A, "status", 4, 16, (0, 4, 12)[(n + pi) % 3], "inout", np.zeros(1, dtype=np.uint32))
            args.append(ws.ptr)
        rc = call(*args, None)
        settle(env, A, rc, OK, note)
        same(el(wd, f), want0[:n], note)
        if with_status:
            assert int(ws.read(np.uint32)[0, 0]) == 0, note


def batch_shapes(f):
    return [(n, pi) for n, pi, _ in placements(f)]


def inv_tiles(f, chain):
    """one tile and one tile plus one element of the chained inversion: 64-lane workgroups (256 for GF(2^128)) of `chain`
    elements per lane (launch_inv_rolled / launch_inv_blocked, capi.hip); Mersenne61 at a 16-byte aligned base takes k_ew_inv,
    256 lanes of 16 packs of two -- 8192 elements -- whatever the chain (ew_inverse, capi.hip)"""
    t = (256 if f == GF else 64) * chain
    sizes = {t, t + 1} | ({8192, 8193} if f == M61 else set())
    phases = (0, 1) if limbs(f) == 1 else (0,)
    return [(n, pi) for n in sorted(sizes) for pi in phases]


def ew_alias_specs():
    out = []
    for f in FIELDS8:
        for op in (O.ADD, O.SUB, O.MUL, O.DIV):
            for alias in ALIASES:
                out.append((f"{fname(f)}-{OPNAME.get(op, 'sub')}-{alias}", dict(f=f, op=op, alias=alias, tiles=0), {}))
        for op in (O.NEG, O.INV):
            out.append((f"{fname(f)}-{OPNAME[op]}-dst=a", dict(f=f, op=op, alias="dst=a", tiles=0), {}))
    # the inversion kernels: one Fermat chain per element (-1), chains of 8 and of 128; fields only (a ring's inverse is k_ew's)
    for f in FIELDS6:
        for v in (-1, 8, 128):
            k = {"inv_batch": v}
            for alias in ("dst=a", "dst=b", "all"):
                out.append((f"{fname(f)}-div-{alias}{knob_label(k)}", dict(f=f, op=O.DIV, alias=alias, tiles=max(v, 0)), k))
            out.append((f"{fname(f)}-inv-dst=a{knob_label(k)}", dict(f=f, op=O.INV, alias="dst=a", tiles=max(v, 0)), k))
    for f in (M127, MONT128):      # the two-level form: chains of 128 in blocks of 4 and of 8
        for v in (4, 8):
            k = {"inv_batch": 128, "inv_two_level": v}
            for alias in ("dst=a", "dst=b", "all"):
                out.append((f"{fname(f)}-div-{alias}{knob_label(k)}", dict(f=f, op=O.DIV, alias=alias, tiles=128), k))
            out.append((f"{fname(f)}-inv-dst=a{knob_label(k)}", dict(f=f, op=O.INV, alias="dst=a", tiles=128), k))
    # one element per lane ("force_scalar"), one workgroup that strides ("max_blocks"), GF(2^128)'s register-only product
    for f in FIELDS3 + [GF]:
        for k in ({"force_scalar": 1}, {"max_blocks": 1}) + (({"inv_batch": -1},) if f == GF else ()):
            for alias in ("dst=a", "dst=b", "all"):
                out.append((f"{fname(f)}-mul-{alias}{knob_label(k)}", dict(f=f, op=O.MUL, alias=alias, tiles=0), k))
    return out


EW_SPECS = ew_alias_specs()


def with_knobs(env, knobs, fn):
    try:
        for key, value in knobs.items():
            env.scl.set_tuning(key, value)
        fn()
    finally:
        for key in knobs:
            env.scl.set_tuning(key, KNOB_DEFAULTS[key])


@pytest.mark.parametrize("entry", ["scl_hip_ew", "scl_hip_ew_status"])
@pytest.mark.parametrize("label,params,knobs", EW_SPECS, ids=[s[0] for s in EW_SPECS])
def test_ew_in_place(env, entry, label, params, knobs):
    """dst == a, dst == b, a == b and all three on one buffer: the oracle's values, and nothing else in the arena moves"""
    f, tiles = params["f"], params["tiles"]
    shapes = batch_shapes(f) + (inv_tiles(f, tiles) if tiles else [])
    with_knobs(env, knobs, lambda: run_ew_alias(env, getattr(env.lib, entry), entry.endswith("_status"), f, params["op"],
                                                params["alias"], shapes))


SM_SPECS = [(fname(f) + knob_label(k), f, k) for f in FIELDS8 for k in ({},)] + \
           [(fname(f) + knob_label(k), f, k) for f in (M61, GF) for k in ({"force_scalar": 1}, {"inv_batch": -1}, {"max_blocks": 1})]


@pytest.mark.parametrize("label,f,knobs", SM_SPECS, ids=[s[0] for s in SM_SPECS])
def test_scalar_mul_in_place(env, label, f, knobs):
    def run():
        s = rnd(env, f, 1, b"al-sm-s")
        a0 = rnd(env, f, 257, b"al-sm-a")
        want0 = env.port.scalar_mul(f, a0, s[0])
        for n, pi in batch_shapes(f):
            note = f"{fname(f)} scalar_mul dst == a N={n} placement {place(f, pi)}"
            A = R.Arena()
            wa = vec(A, "a", f, n, pi, "inout", a0[:n])
            rc = env.lib.scl_hip_scalar_mul(f, wa.ptr, wa.ptr, s.ctypes.data, n, None)
            settle(env, A, rc, OK, note)
            same(el(wa, f), want0[:n], note)
    with_knobs(env, knobs, run)


AS_SPECS = [(f"{fname(f)}-n{n}{knob_label(k)}", f, n, k) for f in FIELDS8 for n in (2, 5) for k in ({},)] + \
           [(f"{fname(f)}-n5{knob_label(k)}", f, 5, k) for f in FIELDS3 for k in ({"force_scalar": 1}, {"max_blocks": 1})]


@pytest.mark.parametrize("label,f,n,knobs", AS_SPECS, ids=[s[0] for s in AS_SPECS])
def test_additive_share_fills_the_matrix_its_randomness_sits_in(env, label, f, n, knobs):
    """rnd == shares at one stride: rows 0 .. n - 2 hold the randomness and keep it, row n - 1 receives secret - sum.  The one
    kernel behind the entry point (k_additive_share) stores back the very pack it loaded, column by column"""
    def run():
        L = limbs(f)
        sec0 = rnd(env, f, 257, b"al-ad-s")
        rnd0 = rnd(env, f, 257 * (n - 1), b"al-ad-r").reshape(n - 1, 257, L)
        last = sec0.copy()
        for i in range(n - 1):
            last = env.port.ew(f, O.SUB, last, rnd0[i])
        for N_, pi, pitch in placements(f):
            note = f"{fname(f)} additive_share rnd == shares n={n} N={N_} placement {place(f, pi)} pitch {pitch}"
            A = R.Arena()
            ws = vec(A, "secrets", f, N_, pi, "in", sec0[:N_])
            wd = mat(A, "shares", f, n, N_, pitch, pi, "inout")
            torch.as_strided(wd.view, (n - 1, N_ * esz(f)), (wd.pitch, 1)).copy_(
                torch.from_numpy(np.ascontiguousarray(rnd0[:, :N_]).view(np.uint8).reshape(n - 1, -1).copy()).to(wd.view.device))
            rc = env.lib.scl_hip_additive_share(f, wd.ptr, pitch, ws.ptr, wd.ptr, pitch, N_, n, None)
            settle(env, A, rc, OK, note)
            got = el(wd, f).reshape(n, N_, L)
            same(got[:n - 1], rnd0[:, :N_], note)
            same(got[n - 1], last[:N_], note)
    with_knobs(env, knobs, run)


FB_SPECS = [(fname(f) + knob_label(k), f, k) for f in FIELDS8 for k in ({},)] + [(fname(f) + "-max_blocks=1", f, {"max_blocks": 1}) for f in FIELDS3]


@pytest.mark.parametrize("label,f,knobs", FB_SPECS, ids=[s[0] for s in FB_SPECS])
def test_from_bytes_in_place(env, label, f, knobs):
    """dst == src where byteSize is the element's size in memory (every field; Z2k<62> and Z2k<128> are 8 and 16 bytes): lane q
    reads the bytes of element q and stores element q (k_from_bytes, k_ring_from_bytes).  The open step's reduce-scatter form
    folds its slice of partial sums this way"""
    def run():
        bs = O.byte_size(f)
        assert bs == esz(f)
        src0 = env.port.prg(b"al-fb", [257 * bs])
        want0 = env.port.from_bytes(f, src0)
        for n, pi in batch_shapes(f):
            note = f"{fname(f)} from_bytes dst == src N={n} placement {place(f, pi)}"
            A = R.Arena()
            w = vec(A, "dst", f, n, pi, "inout", np.frombuffer(src0[:n * bs], dtype=np.uint8))
            rc = env.lib.scl_hip_from_bytes(f, w.ptr, w.ptr, n, None)
            settle(env, A, rc, OK, note)
            same(el(w, f), want0[:n], note)
    with_knobs(env, knobs, run)


def test_from_bytes_in_place_is_refused_for_a_ring_narrower_than_its_limbs(env):
    """Z2k<20> reads 3 bytes per element and stores 8: element 1 would be read from bytes element 0 has overwritten"""
    for K in (20, 56, 100, 120):
        A = R.Arena()
        w = A.window("buf", 64 * 16, 128, 0, kind="in")
        rc = env.lib.scl_hip_from_bytes(O.Z2K(K), w.ptr, w.ptr, 64, None)
        msg = env.lib.scl_hip_last_error().decode()
        assert rc == ERR_BAD_ARG and "dst_dev" in msg and "src_dev" in msg, f"Z2k<{K}>: status {rc} ({msg})"
        A.check()


def test_merkle_build_on_the_buffer_that_holds_its_leaves(env):
    """leaf_digests_dev == tree_dev (no copy): the rows of test_gpu_redzones with the leaves in place, against the hashlib model"""
    for L_, T in G.MERKLE:
        G.run_merkle_build(env, L_, T, True)


# ---------------------------------------------------------------------------------------------- permitted aliases: points
def images(env, pts):
    rawb = host(env.scl.ec_wire_pack(pts.reshape(-1, 12)))
    return [rawb[i].tobytes() for i in range(rawb.shape[0])]


def model_ew(op, p, q):
    import secp256k1_model as F
    return {O.ADD: lambda: F.ec_add(p, q), O.SUB: lambda: F.ec_add(p, F.ec_neg(q)), O.NEG: lambda: F.ec_neg(p),
            EC_DBL: lambda: F.ec_add(p, p)}[op]()


EC_EW_SPECS = [(name + "-" + alias, op, alias) for name, op in (("add", O.ADD), ("sub", O.SUB)) for alias in ALIASES] + \
              [(name + "-dst=a", op, "dst=a") for name, op in (("neg", O.NEG), ("dbl", EC_DBL))]


@pytest.mark.parametrize("label,op,alias", EC_EW_SPECS, ids=[s[0] for s in EC_EW_SPECS])
def test_ec_ew_in_place(env, label, op, alias):
    """byte-equal to the same entry point out of place (the kernels are deterministic), and the first and the last lane equal to
    the big-integer model of tests/secp256k1_model.py through their wire images"""
    import secp256k1_model as F
    binary = op in (O.ADD, O.SUB)
    for n, k in ec_shapes():
        note = f"ec_ew op {op} {alias} n={n} phase {ec_phase(k)}"
        a = points(env, n, b"al-ew-a")
        b = a if alias in ("a=b", "all") else points(env, n, b"al-ew-b")
        want = env.scl.ec_ew(op, a.clone(), b.clone() if binary else None)
        A = R.Arena()
        if alias == "dst=a":
            wa = raw(A, "a", PT * n, 128, ec_phase(k), "inout", host(a))
            wb = raw(A, "b", PT * n, 128, ec_phase(k + 1), "in", host(b)) if binary else None
            wd = wa
        elif alias == "dst=b":
            wa = raw(A, "a", PT * n, 128, ec_phase(k), "in", host(a))
            wd = wb = raw(A, "b", PT * n, 128, ec_phase(k + 1), "inout", host(b))
        elif alias == "a=b":
            wa = wb = raw(A, "a", PT * n, 128, ec_phase(k), "in", host(a))
            wd = raw(A, "dst", PT * n, 128, ec_phase(k + 2), "out")
        else:
            wa = wb = wd = raw(A, "a", PT * n, 128, ec_phase(k), "inout", host(a))
        rc = env.lib.scl_hip_ec_ew(op, wd.ptr, wa.ptr, wb.ptr if wb else None, n, None)
        settle(env, A, rc, OK, note)
        got = wd.read(np.int64).reshape(n, 12)
        same(got, host(want), note)
        ia, ib = images(env, a), images(env, b)
        ig = images(env, torch.from_numpy(got.copy()).cuda())
        for lane in {0, n - 1}:
            m = model_ew(op, F.ec_from_image(ia[lane]), F.ec_from_image(ib[lane]))
            assert ig[lane] == F.ec_image(m), f"{note}: lane {lane} differs from the model"


def test_ec_mul_in_place(env):
    """dst == points: the lane's table in scratch is built from its point before the point is overwritten"""
    import secp256k1_model as F
    from gpu_support import scalars_host
    for n, k in ec_shapes():
        note = f"ec_mul dst == points n={n} phase {ec_phase(k)}"
        pts, s = points(env, n, b"al-ml"), scalars(env, n, b"al-ml-s")
        want = host(env.scl.ec_mul(pts.clone(), s))
        A = R.Arena()
        wp = raw(A, "points", PT * n, 128, ec_phase(k + 1), "inout", host(pts))
        ws = raw(A, "scalars", 32 * n, 128, ec_phase(k + 2), "in", host(s))
        wsc = raw(A, "scratch", env.lib.scl_hip_ec_mul_scratch_bytes(n), 128, ec_phase(k), "inout")
        rc = env.lib.scl_hip_ec_mul(wp.ptr, wp.ptr, ws.ptr, wsc.ptr, n, None)
        settle(env, A, rc, OK, note)
        got = wp.read(np.int64).reshape(n, 12)
        same(got, want, note)
        ip, ig, ks = images(env, pts), images(env, torch.from_numpy(got.copy()).cuda()), scalars_host(env.scl, s)
        for lane in {0, n - 1}:
            assert ig[lane] == F.ec_image(F.ec_mul(ks[lane], F.ec_from_image(ip[lane]))), f"{note}: lane {lane} differs from the model"


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    import scl_amd
    port = O.Port()
    scl_amd.set_mont128_prime((1 << 128) - 159)
    port.mont128_set_prime((1 << 128) - 159)
    return G.Env(scl_amd, port)
