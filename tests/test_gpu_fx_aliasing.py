"""The aliasing contract of include/scl_hip_fx.h on the device: the aliases the header allows -- c == x with one stride in
scl_fx_trunc_mask, y == x or y == rlow with one stride in scl_fx_trunc_finish -- give the same words as the call on disjoint
buffers, and each overlap it forbids is refused before anything is launched, with both operands named and the buffers untouched.
tests/test_fx_abi.py reaches the same refusals without a device."""
import numpy as np
import pytest
import torch

import fx_support as FXS
import oracle_lib as O
from gpu_support import fname, gpu_env, placed

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
ERR_BAD_ARG = 3


@pytest.fixture(scope="module")
def env():
    return gpu_env("fx")


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_permitted_aliases_give_the_disjoint_calls_words(env, f):
    """N = 257, rows 3, (B, k, shift) the field's mid shape; strides N and N + 3; the mask in place on x, the finish in place on x
    and on rlow, m = 3 and the opened form"""
    scl, fx, port = env
    p, N, rows = FXS.prime(f), 257, 3
    B, k, shift = FXS.shapes(p)[3]
    dev = lambda v: scl.to_device(FXS.limbs_of(f, v))
    bits = dev(FXS.uniform(p, (B, rows, N), 9000 + f))
    x = dev(FXS.uniform(p, (rows, N), 9100 + f))
    c = FXS.uniform(p, (N,), 9200 + f) % (1 << (B + 1))
    c[7] = 1 << (B + 1)
    csh = dev(FXS.a_share(p, c, 2, 3, 9300 + f))
    wc, wl = fx.trunc_mask(f, x, bits, k, shift)
    for pitch in (N, N + 3):
        xbuf, xv = placed(x, (pitch,))
        out, rlow = fx.trunc_mask(f, xv, bits, k, shift, out=xv)
        assert out is xv and torch.equal(xv, wc) and torch.equal(rlow, wl), pitch
        for shares, lam in ((csh, None), (dev(c), None)):
            wy, ws = fx.trunc_finish(f, shares, x, wl, shift, B, lam=lam)
            assert ws[7].item() == 1 and ws.sum().item() == 1
            for target in ("x", "rlow"):
                _, xv = placed(x, (pitch,))
                _, lv = placed(wl, (pitch,))
                tv = xv if target == "x" else lv
                y, status = fx.trunc_finish(f, shares, xv, lv, shift, B, lam=lam, out=tv)
                assert y is tv and torch.equal(tv, wy) and torch.equal(status, ws), (pitch, target)
                other, want = (lv, wl) if target == "x" else (xv, x)
                assert torch.equal(other, want), (pitch, target)


@pytest.mark.parametrize("f", [O.M61, O.SECP256K1_SCALAR], ids=fname)
def test_forbidden_overlaps_are_refused_with_both_operands_named(env, f):
    """through the raw C ABI on one live device buffer: compose -- out on the planes; trunc_mask -- c on x at an offset and under
    another stride, c on rlow, rlow on x, c and rlow on the planes; trunc_finish -- y on csh, y on x and on rlow at an offset,
    status on y, x, rlow and csh; nothing is written"""
    scl, fx, port = env
    L, rows, N, B, m = O.LIMBS[f], 3, 8, 5, 3
    e = 8 * L
    buf = scl.to_device(FXS.limbs_of(f, FXS.uniform(FXS.prime(f), (4096,), 9400 + f)))
    before = buf.clone()
    base = buf.data_ptr()
    at = lambda k: base + k * 512 * e                                   # regions 512 elements apart
    out, rlow, x, bits, status = at(0), at(1), at(2), at(3), at(5)
    lam = np.ones((m, L), dtype=np.uint64)
    co = lambda o, b: fx.lib.scl_fx_compose(f, o, N, b, N, B * N, B, rows, N, None)
    mk = lambda c, lo, xx, b, cs=N: fx.lib.scl_fx_trunc_mask(f, c, cs, lo, N, xx, N, b, N, B * N, 4, 2, B, rows, N, None)
    fi = lambda y, lo, xx, cs, st, ys=N: fx.lib.scl_fx_trunc_finish(f, y, ys, st, cs, N, lam.ctypes.data, m, xx, N, lo, N, 2, B, rows, N, None)
    cases = [(lambda: co(bits + 16, bits), b"compose: out_dev overlaps bits_dev"),
             (lambda: co(bits + (rows * B * N - 1) * e, bits), b"compose: out_dev overlaps bits_dev"),
             (lambda: mk(x + 16, rlow, x, bits), b"trunc_mask: c_dev overlaps x_dev"), (lambda: mk(x, rlow, x, bits, cs=N + 2), b"trunc_mask: c_dev overlaps x_dev"),
             (lambda: mk(out, out, x, bits), b"trunc_mask: c_dev overlaps rlow_dev"), (lambda: mk(out, x, x, bits), b"trunc_mask: x_dev overlaps rlow_dev"),
             (lambda: mk(bits, rlow, x, bits), b"trunc_mask: c_dev overlaps bits_dev"), (lambda: mk(out, bits + 16, x, bits), b"trunc_mask: rlow_dev overlaps bits_dev"),
             (lambda: fi(bits, rlow, x, bits, status), b"trunc_finish: y_dev overlaps csh_dev"),
             (lambda: fi(x + 16, rlow, x, bits, status), b"trunc_finish: y_dev overlaps x_dev"),
             (lambda: fi(x, rlow, x, bits, status, ys=N + 2), b"trunc_finish: y_dev overlaps x_dev"),
             (lambda: fi(rlow + 16, rlow, x, bits, status), b"trunc_finish: y_dev overlaps rlow_dev"),
             (lambda: fi(out, rlow, x, bits, out + 1), b"trunc_finish: y_dev overlaps status_dev"),
             (lambda: fi(out, rlow, x, bits, x + 5), b"trunc_finish: x_dev overlaps status_dev"),
             (lambda: fi(out, rlow, x, bits, rlow), b"trunc_finish: rlow_dev overlaps status_dev"),
             (lambda: fi(out, rlow, x, bits, bits + m * N * e - 1), b"trunc_finish: csh_dev overlaps status_dev")]
    for call, words in cases:
        assert call() == ERR_BAD_ARG, words
        msg = fx.lib.scl_fx_last_error()
        assert words in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
