"""Aliasing tests for the inner-product extension: which operands of scl_ip_dot_mask and scl_ip_matmul_mask may share memory, and
that every other overlap of the output with an input is refused.

include/scl_hip_ip.h states the rule per entry point in the style of include/scl_hip.h: d_dev may be r2_dev -- the same pointer and
the same strides --, d_dev must not overlap x_dev or y_dev, and the inputs may overlap one another freely.  ALIASING below is that
contract as data, one decision per (written operand, other operand) pair with the header's words; the table tests (no GPU) tie it
to the prototypes and to the comment in front of each, as tests/test_aliasing_model.py does for the core library.

On the GPU, through the raw C ABI into a tests/redzone.py arena:
* the permitted alias, for every field: the call in place on r2 gives the model's values and writes nothing else (the aliased
  window is `inout`); so does a call whose inputs all coincide (x == y == r2, out of place: sums of squares plus x_0);
* refusals: for d/x and d/y the exact alias, the output one element into the input and the output one row into it; for d/r2 the
  three near misses -- the same pointer at another stride, one element in, one row in.  Each returns SCL_ERR_BAD_ARG, names both
  operands, and leaves the arena untouched with every window declared `in`: nothing was written.  (The operands hold the arena's
  pattern: a refusal reads none of them.)"""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import redzone as R
from cxx_support import ROOT
from gpu_support import el, esz, fname, gpu_env, limbs, mat, placements, pool, settle
from port_models import model_dot_mask, model_matmul_mask

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
ERR_BAD_ARG = 3

_PAIRS = {("d_dev", "x_dev"): ("refuse", "d_dev must not overlap x_dev"), ("d_dev", "y_dev"): ("refuse", "d_dev must not overlap y_dev"),
          ("d_dev", "r2_dev"): ("permit", "d_dev may be r2_dev")}
ALIASING = {"scl_ip_dot_mask": dict(_PAIRS), "scl_ip_matmul_mask": dict(_PAIRS)}
# what the header adds to the permitted alias: the strides that must agree
EXACT = {"scl_ip_dot_mask": "with d_stride == op_stride", "scl_ip_matmul_mask": "with d_stride == r2_stride and, where batch > 1, d_batch_stride == r2_batch_stride"}


# ---------------------------------------------------------------------------------------------- the table against the header
def prototypes():
    """{entry point: (its parameter list [(type, name)], the comment right in front of it)}"""
    src = open(os.path.join(ROOT, "include", "scl_hip_ip.h")).read()
    out, prev = {}, 0
    for m in re.finditer(r"^(?:int|void|size_t|const char\*)\s+(scl_ip_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S):
        between = src[prev:m.start()]
        prev = m.end()
        for stop in ("#define", 'extern "C" {'):
            between = between[between.rfind(stop) + 1:] if stop in between else between
        comment = " ".join(re.findall(r"/\*(.*?)\*/", between, flags=re.S))
        comment = re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", comment, flags=re.M))
        params = []
        for p in re.sub(r"\s+", " ", m.group(2)).split(","):
            p = p.strip()
            if p in ("void", ""):
                continue
            pm = re.match(r"(.*?)(\w+)$", p)
            params.append((pm.group(1).strip(), pm.group(2)))
        out[m.group(1)] = (params, comment)
    return out


def device_operands(params):
    dev = [(t, n) for t, n in params if n.endswith("_dev") and "*" in t]
    return [n for t, n in dev if "const" not in t], [n for t, n in dev]


def test_every_entry_point_has_a_decision_for_every_pair_of_device_operands():
    """(reads the header and the table: needs no GPU)"""
    protos = prototypes()
    writing = {e for e, (params, _) in protos.items() if device_operands(params)[0]}
    assert writing == set(ALIASING)
    for entry, pairs in ALIASING.items():
        written, every = device_operands(protos[entry][0])
        assert written == ["d_dev"] and every == ["d_dev", "x_dev", "y_dev", "r2_dev"], entry
        assert set(pairs) == {(o, x) for o in written for x in every if x != o}, entry


def test_each_decision_is_worded_in_the_comment_of_its_entry_point():
    """(needs no GPU)"""
    protos = prototypes()
    for entry, pairs in ALIASING.items():
        comment = protos[entry][1]
        assert "Aliasing:" in comment, f"{entry}: no aliasing rule in front of its prototype"
        rule = comment.split("Aliasing:")[-1]
        for (o, x), (kind, words) in pairs.items():
            assert words in rule, f"{entry}: ({o}, {x}) is decided as {words!r}; the header says {rule.strip()!r}"
        assert EXACT[entry] in rule and "inputs and may overlap one another" in rule, entry
        for o, x in re.findall(r"(\w+_dev) may be (\w+_dev)", rule):         # the header permits nothing the table refuses
            assert pairs[(o, x)][0] == "permit", (entry, o, x)


# ---------------------------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def env():
    return gpu_env("ip")


@pytest.mark.gpu
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_permitted_alias_and_coinciding_inputs(env, f):
    """N 1, 3, 64, 257 at every placement: dot (7 terms, 3 rows) and matmul ((5,7,3), batch 2; one window holds both batches) in
    place on r2; and dot with x == y == r2 out of place"""
    scl, ip, port = env
    L, terms, rows = limbs(f), 7, 3
    a, K, b, batch = 5, 7, 3, 2
    for k, N in enumerate((1, 3, 64, 257)):
        x, y = [pool(port, f, terms * rows * N, b"al-dot-" + t).reshape(terms, rows, N, L) for t in (b"x", b"y")]
        r2 = pool(port, f, rows * N, b"al-dot-r").reshape(rows, N, L)
        X = pool(port, f, batch * a * K * N, b"al-mm-x").reshape(batch, a, K, N, L)
        Y = pool(port, f, batch * K * b * N, b"al-mm-y").reshape(batch, K, b, N, L)
        R2 = pool(port, f, batch * a * b * N, b"al-mm-r").reshape(batch, a, b, N, L)
        for align, phase, pitch in placements(f, N, k):
            note = f"{fname(f)} N={N} pitch={pitch} phase={phase}"
            A = R.Arena()
            wx = mat(A, "x", f, terms * rows, N, pitch, align, phase, "in", x.reshape(-1, N, L))
            wy = mat(A, "y", f, terms * rows, N, pitch, align, phase, "in", y.reshape(-1, N, L))
            wr = mat(A, "r2", f, rows, N, pitch, align, phase, "inout", r2)
            rc = ip.lib.scl_ip_dot_mask(f, wr.ptr, pitch, wx.ptr, rows * pitch, wy.ptr, rows * pitch, wr.ptr, pitch, terms, rows, N, None)
            settle(ip.lib.scl_ip_last_error, A, rc, "dot_mask in place " + note)
            assert np.array_equal(el(wr, f), model_dot_mask(port, f, x, y, r2)), "dot_mask in place " + note
            A = R.Arena()
            wx = mat(A, "x", f, terms * rows, N, pitch, align, phase, "in", x.reshape(-1, N, L))
            wd = mat(A, "d", f, rows, N, pitch + 2, align, phase)
            rc = ip.lib.scl_ip_dot_mask(f, wd.ptr, pitch + 2, wx.ptr, rows * pitch, wx.ptr, rows * pitch, wx.ptr, pitch, terms, rows, N, None)
            settle(ip.lib.scl_ip_last_error, A, rc, "dot_mask x == y == r2 " + note)
            assert np.array_equal(el(wd, f), model_dot_mask(port, f, x, x, x[0])), "dot_mask x == y == r2 " + note
            A = R.Arena()
            wX = mat(A, "x", f, batch * a * K, N, pitch, align, phase, "in", X.reshape(-1, N, L))
            wY = mat(A, "y", f, batch * K * b, N, pitch, align, phase, "in", Y.reshape(-1, N, L))
            wR = mat(A, "r2", f, batch * a * b, N, pitch, align, phase, "inout", R2.reshape(-1, N, L))
            rc = ip.lib.scl_ip_matmul_mask(f, wR.ptr, pitch, a * b * pitch, wX.ptr, pitch, a * K * pitch, wY.ptr, pitch, K * b * pitch, wR.ptr, pitch,
                                           a * b * pitch, a, K, b, batch, N, None)
            settle(ip.lib.scl_ip_last_error, A, rc, "matmul_mask in place " + note)
            assert np.array_equal(el(wR, f).reshape(batch, a, b, N, L), model_matmul_mask(port, f, X, Y, R2)), "matmul_mask in place " + note


def refused(ip, A, rc, note, *names):
    msg = ip.lib.scl_ip_last_error().decode()
    assert rc == ERR_BAD_ARG, f"{note}: status {rc} ({msg})"
    assert "overlaps" in msg and all(n in msg for n in names), f"{note}: {msg}"
    try:
        A.check()                                   # every window is `in`: nothing at all was written
    except R.RedZoneError as e:
        raise R.RedZoneError(f"{note}\n{e}", e.strays, e.count) from None


@pytest.mark.gpu
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_every_other_overlap_of_the_output_is_refused(env, f):
    """d on x and on y: exactly, one element in, one row in; d on r2: the same pointer at another stride, one element in, one row
    in -- for both entry points (matmul at batch 1 and 2; at batch 2 also the same pointer at another batch stride)"""
    scl, ip, port = env
    e, N, pitch = esz(f), 6, 8
    terms, rows = 3, 3
    a, K, b = 2, 3, 2
    A = R.Arena()
    big = 2 * max(terms * rows, a * K, K * b)       # rows per window: two batches of the largest operand
    w = {nm: mat(A, nm, f, big, N, pitch, 128, 0, "in") for nm in ("d", "x", "y", "r2")}
    p = {nm: w[nm].ptr for nm in w}
    dot = lambda q, ds=pitch: ip.lib.scl_ip_dot_mask(f, q["d"], ds, q["x"], rows * pitch, q["y"], rows * pitch, q["r2"], pitch, terms, rows, N, None)
    mm = lambda q, batch, ds=pitch, dbs=None: ip.lib.scl_ip_matmul_mask(f, q["d"], ds, a * b * ds if dbs is None else dbs, q["x"], pitch, a * K * pitch,
                                                                      q["y"], pitch, K * b * pitch, q["r2"], pitch, a * b * pitch, a, K, b, batch, N, None)
    calls = [("dot_mask", dot)] + [(f"matmul_mask batch={bt}", (lambda q, bt=bt, **kw: mm(q, bt, **kw))) for bt in (1, 2)]
    for name, call in calls:
        for other in ("x", "y", "r2"):
            offsets = [("one element in", e), ("one row in", pitch * e)]
            if other != "r2":
                offsets.append(("exactly", 0))
            for how, off in offsets:
                q = dict(p)
                q["d"] = p[other] + off
                refused(ip, A, call(q), f"{name} {fname(f)}: d on {other} {how}", "d_dev", other + "_dev")
        q = dict(p)
        q["d"] = p["r2"]
        refused(ip, A, call(q, ds=pitch + 2), f"{name} {fname(f)}: d on r2 at another stride", "d_dev", "r2_dev", "may coincide")
    q = dict(p)
    q["d"] = p["r2"]
    refused(ip, A, mm(q, 2, dbs=a * b * pitch + 2), f"matmul_mask {fname(f)}: d on r2 at another batch stride", "d_dev", "r2_dev", "may coincide")
