"""The aliasing contract of include/scl_hip_cmp.h on the device: the aliases the header allows -- out == x, out == rlow or out == lt
with one stride in scl_cmp_finish -- give the same words as the call on disjoint buffers, and each overlap it forbids is refused
before anything is launched, with both operands named and the buffers untouched.  tests/test_cmp_abi.py reaches the same refusals
without a device."""
import numpy as np
import pytest
import torch

import cmp_support as CS
import fx_support as FXS
import oracle_lib as O
from gpu_support import fname, gpu_env, placed

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
ERR_BAD_ARG = 3


@pytest.fixture(scope="module")
def env():
    return gpu_env("cmp")


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_permitted_aliases_give_the_disjoint_calls_words(env, f):
    """N = 257, rows 3, w = 9; strides N and N + 3; the finish in place on x, on rlow and on lt, in its three forms, with a flagged
    column"""
    scl, cmp, port = env
    p, N, rows, w = FXS.prime(f), 257, 3, 9
    dev = lambda v: scl.to_device(FXS.limbs_of(f, v))
    lt, rlow, x = (dev(FXS.uniform(p, (rows, N), 9000 + 10 * i + f)) for i in range(3))
    cmod = dev(FXS.uniform(p, (N,), 9100 + f) % (1 << w))
    status = torch.zeros(N, dtype=torch.uint8, device="cuda")
    status[7] = 1
    for what in (CS.MOD, CS.TRUNC, CS.LTZ):
        want = cmp.finish(f, lt, cmod, status, rlow, x, w, what)
        assert not want[:, 7].any().item() and want.any().item()
        for pitch in (N, N + 3):
            for target in range(3):
                views = [placed(t, (pitch,))[1] for t in (lt, rlow, x)]
                y = cmp.finish(f, views[0], cmod, status, views[1], views[2], w, what, out=views[target])
                assert y is views[target] and torch.equal(y, want), (what, pitch, target)
                assert all(torch.equal(v, t) for i, (v, t) in enumerate(zip(views, (lt, rlow, x))) if i != target), (what, pitch, target)


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR], ids=fname)
def test_forbidden_overlaps_are_refused_with_both_operands_named(env, f):
    """through the raw C ABI on one live device buffer: first_mask -- d on the planes, on r2, on csh and on cmod, cmod on the
    status and on csh, the status on the planes; level_mask -- d on the nodes and on r2; finish -- out on cmod and on the status,
    out on x, rlow and lt at an offset or under another stride; nothing is written"""
    scl, cmp, port = env
    L, rows, N, w, B, cnt, m = O.LIMBS[f], 3, 8, 5, 9, 3, 3
    e = 8 * L
    buf = scl.to_device(FXS.limbs_of(f, FXS.uniform(FXS.prime(f), (8192,), 9400 + f)))
    before = buf.clone()
    base = buf.data_ptr()
    at = lambda k: base + k * 512 * e                                   # regions 512 elements apart
    d, cmod, status, csh, bits, r2, out, lt = (at(k) for k in range(8))
    lam = np.ones((m, L), dtype=np.uint64)
    fm = lambda d=d, cmod=cmod, status=status, csh=csh, bits=bits, r2=r2: cmp.lib.scl_cmp_first_mask(
        f, d, N, 6 * N, cmod, status, csh, N, lam.ctypes.data, m, bits, N, B * N, r2, N, 6 * N, w, B, rows, N, 0, None)
    lm = lambda d=d, nodes=bits, r2=r2: cmp.lib.scl_cmp_level_mask(f, d, N, 4 * N, nodes, N, 2 * cnt * N, r2, N, 4 * N, cnt, rows, N, 0, None)
    fi = lambda out=out, cmod=cmod, status=status, lt=lt, rlow=bits, x=r2, os=N: cmp.lib.scl_cmp_finish(
        f, out, os, lt, N, cmod, status, rlow, N, x, N, w, CS.TRUNC, rows, N, None)
    cases = [(lambda: fm(d=bits + 16), b"first_mask: d_dev overlaps bits_dev"), (lambda: fm(d=r2), b"first_mask: d_dev overlaps r2_dev"),
             (lambda: fm(csh=d + 16), b"first_mask: d_dev overlaps csh_dev"), (lambda: fm(cmod=d + (rows * 6 * N - 1) * e), b"first_mask: d_dev overlaps cmod_dev"),
             (lambda: fm(status=cmod + N * e - 1), b"first_mask: cmod_dev overlaps status_dev"), (lambda: fm(cmod=csh + 16), b"first_mask: cmod_dev overlaps csh_dev"),
             (lambda: fm(status=bits + 5), b"first_mask: status_dev overlaps bits_dev"),
             (lambda: lm(d=bits), b"level_mask: d_dev overlaps nodes_dev"), (lambda: lm(r2=d + (rows * 4 * N - 1) * e), b"level_mask: d_dev overlaps r2_dev"),
             (lambda: fi(out=cmod), b"finish: out_dev overlaps cmod_dev"), (lambda: fi(status=out + 3), b"finish: out_dev overlaps status_dev"),
             (lambda: fi(out=r2 + 16), b"finish: out_dev overlaps x_dev"), (lambda: fi(out=r2, os=N + 2), b"finish: out_dev overlaps x_dev"),
             (lambda: fi(out=bits + 16), b"finish: out_dev overlaps rlow_dev"), (lambda: fi(out=lt + 16), b"finish: out_dev overlaps lt_dev")]
    for call, words in cases:
        assert call() == ERR_BAD_ARG, words
        msg = cmp.lib.scl_cmp_last_error()
        assert words in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
