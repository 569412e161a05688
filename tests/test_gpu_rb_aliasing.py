"""The aliasing contract of include/scl_hip_rb.h on the device: the two aliases the header allows -- out == a in scl_rb_sqrt,
b == r with one stride in scl_rb_bits_finish -- give the same words as the call on disjoint buffers, and each overlap it forbids
is refused before anything is launched, with both operands named and the buffers untouched.  tests/test_rb_abi.py reaches the
same refusals without a device."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import rb_support as RBS
from gpu_support import fname, gpu_env, host, placed

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
ERR_BAD_ARG = 3


@pytest.fixture(scope="module")
def env():
    return gpu_env("rb")


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_permitted_aliases_give_the_disjoint_calls_words(env, f):
    """N = 257; sqrt in place under all four flags; bits_finish in place at rows 3 and 17, strides N and N + 3"""
    scl, rb, port = env
    p, N = RBS.prime(f), 257
    a = RBS.seeded(p, N, 9000 + f)
    a[5] = 0
    for flags in range(4):
        dev = scl.to_device(RBS.to_limbs(f, a))
        want, wstatus = rb.sqrt(f, dev.clone(), flags)
        out, status = rb.sqrt(f, dev, flags, out=dev)
        assert out is dev and torch.equal(dev, want) and torch.equal(status, wstatus)
        assert status.cpu().tolist() == [RBS.model_sqrt(p, v, flags)[1] for v in a]
    u = [v * v % p for v in RBS.seeded(p, N, 9100 + f)]
    u[7] = 0
    ud = scl.to_device(RBS.to_limbs(f, u))
    for rows in (3, 17):
        r = scl.to_device(np.stack([RBS.to_limbs(f, RBS.seeded(p, N, 9200 + f + i)) for i in range(rows)]))
        for pitch in (N, N + 3):
            want, wstatus = rb.bits_finish(f, ud, r)
            buf, rv = placed(r, (pitch,))
            out, status = rb.bits_finish(f, ud, rv, out=rv)
            assert out is rv and torch.equal(rv, want) and torch.equal(status, wstatus), (rows, pitch)
            assert np.array_equal(host(ud), RBS.to_limbs(f, u))


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR], ids=fname)
def test_forbidden_overlaps_are_refused_with_both_operands_named(env, f):
    """through the raw C ABI on one live device buffer: sqrt -- out on a at an offset, status on out and on a; bits_finish -- b on
    u, b on r at an offset and under another stride, status on b, u and r; nothing is written"""
    scl, rb, port = env
    L, rows, N = O.LIMBS[f], 3, 8
    e = 8 * L
    buf = scl.to_device(RBS.to_limbs(f, RBS.seeded(RBS.prime(f), 4096, 9300 + f)))
    before = buf.clone()
    base = buf.data_ptr()
    at = lambda k: base + k * 512 * e                                   # regions 512 elements apart
    out, status, a, r = at(0), at(1), at(2), at(3)
    sq = lambda o, st, aa: rb.lib.scl_rb_sqrt(f, o, st, aa, N, 0, None)
    bf = lambda b, st, u, rr, bs=N, rs=N: rb.lib.scl_rb_bits_finish(f, b, bs, st, u, rr, rs, rows, N, None)
    cases = [(lambda: sq(a + 16, status, a), b"sqrt: out_dev overlaps a_dev"), (lambda: sq(out, out + 3, a), b"sqrt: out_dev overlaps status_dev"),
             (lambda: sq(out, a + N * e - 1, a), b"sqrt: a_dev overlaps status_dev"),
             (lambda: bf(a, status, a, r), b"bits_finish: b_dev overlaps u_dev"), (lambda: bf(r + 16, status, a, r), b"bits_finish: b_dev overlaps r_dev"),
             (lambda: bf(r, status, a, r, bs=N + 2), b"bits_finish: b_dev overlaps r_dev"),
             (lambda: bf(out, out + 1, a, r), b"bits_finish: b_dev overlaps status_dev"),
             (lambda: bf(out, a, a, r), b"bits_finish: u_dev overlaps status_dev"), (lambda: bf(out, r + 5, a, r), b"bits_finish: r_dev overlaps status_dev")]
    for call, words in cases:
        assert call() == ERR_BAD_ARG, words
        msg = rb.lib.scl_rb_last_error()
        assert words in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
