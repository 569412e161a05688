"""The aliasing contract of include/scl_hip_vf.h on the device: the overlaps the header allows compute the right value -- x, y and
rho are inputs and may share memory: x == y (sum rho x^2), rho inside x, all three one buffer --, and each overlap it forbids
-- out or scratch on any operand or on each other -- is refused before anything is launched, with both operands named and the
buffers untouched.  tests/test_vf_abi.py reaches the same refusals without a device."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from gpu_support import fname, gpu_env, host, pool
from port_models import model_combine

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
ERR_BAD_ARG = 3


@pytest.fixture(scope="module")
def env():
    return gpu_env("vf")


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_inputs_may_overlap_one_another(env, f):
    """rows 3, N 65, reps 2: x == y; rho = rows 1 and 2 of x; rho overlapping x at an offset of one column; product with y = rho"""
    scl, vf, port = env
    L, rows, N = O.LIMBS[f], 3, 65
    xh = pool(port, f, rows * N + 1, b"vf-alias").reshape(-1, L)
    buf = scl.to_device(xh)
    x = buf[:rows * N].reshape(rows, N, L)
    xm = xh[:rows * N].reshape(rows, N, L)
    rho, rm = x[1:3], xm[1:3]
    assert np.array_equal(host(vf.combine(f, x, rho)), model_combine(port, f, xm, rm))
    assert np.array_equal(host(vf.combine(f, x, rho, x)), model_combine(port, f, xm, rm, xm))
    assert np.array_equal(host(vf.combine_prg(f, x, x, seed=b"vf alias", reps=2)), host(vf.combine_prg(f, x, x.clone(), seed=b"vf alias", reps=2)))
    shifted, sm = buf[1:1 + 2 * N].reshape(2, N, L), xh[1:1 + 2 * N].reshape(2, N, L)           # one column into x
    assert np.array_equal(host(vf.combine(f, x, shifted)), model_combine(port, f, xm, sm))
    assert np.array_equal(host(vf.combine(f, x[:2], shifted, shifted)), model_combine(port, f, xm[:2], sm, sm))
    assert np.array_equal(host(buf), xh)


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR], ids=fname)
def test_forbidden_overlaps_are_refused_with_both_operands_named(env, f):
    """through the raw C ABI on one live device buffer: out on x, y, rho and scratch; scratch on x, y and rho; nothing is written"""
    scl, vf, port = env
    L, rows, N, reps = O.LIMBS[f], 3, 8, 2
    e = 8 * L
    buf = scl.to_device(pool(port, f, 4096, b"vf-alias-raw").reshape(-1, L))
    before = buf.clone()
    base = buf.data_ptr()
    at = lambda k: base + k * 512 * e                                   # regions 512 elements apart
    out, x, y, rho, scratch = at(0), at(1), at(2), at(3), at(4)
    for prg in (True, False):
        need = vf.scratch_bytes(f, rows, reps, N, vf.PRG if prg else 0)
        assert need <= 512 * e

        def call(o, xx, yy, rr, ss):
            if prg:
                return vf.lib.scl_vf_combine_prg(f, o, reps, xx, yy, N, rows, N, reps, b"seed", 4, 0, ss, need, None)
            return vf.lib.scl_vf_combine(f, o, reps, xx, yy, N, rr, N, rows, N, reps, ss, need, None)
        who = b"combine_prg" if prg else b"combine"
        cases = [((x, x, y, rho, scratch), b"out_dev overlaps x_dev"), ((y + 16, x, y, rho, scratch), b"out_dev overlaps y_dev"),
                 ((out, x, y, rho, out), b"out_dev overlaps scratch_dev"), ((out, x, y, rho, x + 16), b"scratch_dev overlaps x_dev"),
                 ((out, x, y, rho, y), b"scratch_dev overlaps y_dev")]
        if not prg:
            cases += [((rho, x, y, rho, scratch), b"out_dev overlaps rho_dev"), ((out, x, y, rho, rho + 16), b"scratch_dev overlaps rho_dev")]
        for args, words in cases:
            assert call(*args) == ERR_BAD_ARG
            msg = vf.lib.scl_vf_last_error()
            assert msg.startswith(who) and words in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
