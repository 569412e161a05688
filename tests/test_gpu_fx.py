"""Probabilistic truncation on the device (libscl_hip_fx.so): scl_fx_compose, scl_fx_trunc_mask and scl_fx_trunc_finish against the
Python model of tests/fx_support.py on every element -- all five prime fields, Mont128 at 2^128 - 159 and at 2^127 - 1; N in
{1, 2, 3, 257, 513} (the pair path of Mersenne61, its odd tail, a workgroup edge), rows in {1, 3}; (B, k, shift) at the smallest
and the largest shape, a wide kappa, one mid case and shift on both sides of every limb boundary; x at the ends of its range, 0,
-1 and seeded values; planes of seeded shares and planes whose every share is p - 1 at B = max (the worst case of the Horner
accumulator); the status at c = 2^(B+1) exactly and one below --, the whole pipeline over scl_amd.hm and scl_amd.rb end to end
(deal, extract, random bits, truncate: the reconstructed y equals floor((x + 2^(k-1)) / 2^shift) + carry - 2^(k-1-shift) in every
column, the carry computed from the recovered bits), the fixed-point product, the three calls captured into a graph as the first
calls of a fresh process, and the C++ mirror.  Everything is exact."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import fx_support as FXS
import oracle_lib as O
from gpu_support import MONT_P, deal_all, gpu_env, host, placed

pytestmark = pytest.mark.gpu

CASES = FXS.CASES
IDS = [c[0] for c in CASES]
NS = [1, 2, 3, 257, 513]
ROWS = [1, 3]
MAIN = ["smallest", "largest", "wide-kappa", "mid"]          # the first four of FXS.shapes


@pytest.fixture(scope="module")
def env():
    return gpu_env("fx", "rb", "hm")


@pytest.fixture
def modulus(env):
    """sets the Mont128 modulus of a case on this thread, and the tests' own afterwards"""
    scl = env[0]

    def use(mp):
        if mp is not None:
            scl.set_mont128_prime(mp)
        return mp or FXS.MONT_P0
    yield use
    scl.set_mont128_prime(MONT_P)


def dev(scl, f, values, mp):
    return scl.to_device(FXS.limbs_of(f, values, mp))


def xs_of(p, k, shape, seed):
    """x: the ends of the signed k-bit range, 0 and -1 in the first columns, seeded in-range values after them"""
    v = (FXS.uniform(p, shape, seed) % (1 << k) - (1 << (k - 1))) % p
    flat = v.reshape(-1)
    for i, e in enumerate([-(1 << (k - 1)), (1 << (k - 1)) - 1, 0, -1][:flat.size]):
        flat[i] = e % p
    return flat.reshape(shape)


def three_calls(env, f, mp, p, B, k, shift, N, rows, pitch, seed, planes=None):
    """compose, mask and finish at one shape against the model, every element; the operands are left alone and nothing but the
    views of the outputs is written"""
    scl, fx = env[0], env[1]
    note = (B, k, shift, N, rows, pitch)
    planes = FXS.uniform(p, (B, rows, N), seed) if planes is None else planes
    x = xs_of(p, k, (rows, N), seed + 1)
    bbuf, bv = placed(dev(scl, f, planes, mp), (pitch, B * pitch))
    xbuf, xv = placed(dev(scl, f, x, mp), (pitch,))
    before = (bbuf.clone(), xbuf.clone())
    # compose
    obuf, ov = placed(torch.zeros(rows, N, FXS.limbs(f), dtype=torch.int64, device="cuda"), (pitch + 2,))
    fx.compose(f, bv, out=ov)
    assert (FXS.ints_of(f, host(ov.contiguous()), mp) == FXS.a_compose(p, planes)).all(), ("compose",) + note
    # mask
    cbuf, cv = placed(torch.zeros_like(ov), (pitch + 2,))
    lbuf, lv = placed(torch.zeros_like(ov), (pitch,))
    fx.trunc_mask(f, xv, bv, k, shift, out=cv, rlow=lv)
    wc, wl = FXS.a_mask(p, x, planes, k, shift)
    assert (FXS.ints_of(f, host(cv.contiguous()), mp) == wc).all(), ("mask c",) + note
    assert (FXS.ints_of(f, host(lv.contiguous()), mp) == wl).all(), ("mask rlow",) + note
    # finish: shares of seeded in-range values of c under m = 3, the two edges of the range planted; x and rlow are any elements
    m = 3
    c = FXS.uniform(p, (N,), seed + 2) % (1 << (B + 1))
    if N >= 2:
        c[0], c[N - 1] = 1 << (B + 1), (1 << (B + 1)) - 1
    csh = FXS.a_share(p, c, m - 1, m, seed + 3)
    lam = FXS.limbs_of(f, np.array(FXS.lagrange_at_zero(p, m), dtype=object), mp)
    sbuf, sv = placed(dev(scl, f, csh, mp), (pitch + 1,))
    ybuf, yv = placed(torch.zeros_like(ov), (pitch,))
    _, status = fx.trunc_finish(f, sv, xv, lv, shift, B, lam=lam, out=yv)
    wy, ws = FXS.a_finish(p, c, x, wl, shift, B)
    assert status.cpu().numpy().tolist() == ws.tolist() and (N < 2 or (ws[0] == 1 and ws[N - 1] == 0)), ("finish status",) + note
    assert (FXS.ints_of(f, host(yv.contiguous()), mp) == wy).all(), ("finish y",) + note
    assert N < 2 or not yv[:, 0].any().item(), note
    # the already opened form: m = 1, lambda = {1}
    y1, st1 = fx.trunc_finish(f, dev(scl, f, c, mp), xv, lv, shift, B)
    assert torch.equal(y1, yv.contiguous()) and torch.equal(st1, status), ("finish opened",) + note
    assert torch.equal(bbuf, before[0]) and torch.equal(xbuf, before[1]), note
    for buf, view in ((obuf, ov), (cbuf, cv), (lbuf, lv), (ybuf, yv)):
        rest = buf.clone()
        torch.as_strided(rest, tuple(view.shape), view.stride(), view.storage_offset() - buf.storage_offset()).zero_()
        assert not rest.any().item(), note


@pytest.mark.parametrize("which", range(4), ids=MAIN)
@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_the_three_calls_equal_the_model(env, modulus, name, f, mp, which):
    """N in {1, 2, 3, 257, 513} x rows in {1, 3}; the row pitch is N for one row count and N + 3 for the other (Mersenne61: two
    columns per lane under the even strides, one under the odd ones)"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    B, k, shift = FXS.shapes(p)[which]
    for i, N in enumerate(NS):
        for j, rows in enumerate(ROWS):
            three_calls(env, f, mp, p, B, k, shift, N, rows, N + 3 * ((i + j) % 2), 100 * IDS.index(name) + 10 * which + i)


@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_every_share_p_minus_one_at_the_largest_b(env, modulus, name, f, mp):
    """the worst case of the Horner accumulator: B = max planes whose every share is p - 1, N = 3 and 513, rows 3 and 1"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    B = FXS.max_bits(p)
    for N, rows, k, shift in ((3, 3, B, B - 1), (513, 1, B // 2, B // 4), (258, 3, 2, 1)):
        planes = np.full((B, rows, N), p - 1, dtype=object)
        three_calls(env, f, mp, p, B, k, shift, N, rows, N + 1, 900 + IDS.index(name), planes=planes)


@pytest.mark.parametrize("name,f,mp", [c for c in CASES if c[1] != FXS.M61], ids=[i for i in IDS if i != "m61"])
def test_shift_on_both_sides_of_every_limb_boundary(env, modulus, name, f, mp):
    """shift in {63, 64, 65} for the 16-byte fields, and {127, 128, 129}, {191, 192, 193} for the 32-byte fields: the mask of
    c mod 2^shift ends in any limb, the second accumulator starts at any plane"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    edges = FXS.shapes(p)[4:]
    assert len(edges) == (9 if FXS.limbs(f) == 4 else 3) and {s for _, _, s in edges} >= {63, 64, 65}
    for i, (B, k, shift) in enumerate(edges):
        N, rows = ((3, 3), (257, 1))[i % 2]
        three_calls(env, f, mp, p, B, k, shift, N, rows, N + 3, 500 + 20 * IDS.index(name) + i)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def dealt(env, f, n, t, count, tag):
    """`count` extracted double sharings for all n parties: (R_lo, R_hi) [n][count][L]"""
    scl, fx, rb, hm, port = env
    L, m = O.LIMBS[f], n - t
    S = -(-count // m)
    z = lambda *shape: torch.zeros(*shape, L, dtype=torch.int64, device="cuda")
    lo, hi, R_lo, R_hi = z(n, n, S), z(n, n, S), z(n, m, S), z(n, m, S)
    deal_all(hm, f, S, t, n, [b"fx %s dealer %d" % (tag, i) for i in range(n)], lo, hi)
    Md = scl.to_device(hm.hyper_invertible(f, m, n))
    hm.apply_matrix(f, Md, lo.transpose(0, 1), out=R_lo)
    hm.apply_matrix(f, Md, hi.transpose(0, 1), out=R_hi)
    return R_lo.reshape(n, m * S, L)[:, :count], R_hi.reshape(n, m * S, L)[:, :count]


def random_bit_planes(env, f, n, t, B, N, R_lo, R_hi, spares=64):
    """B * N random shared bits as planes [B][n][N][L] from 2 (B N + spares) double sharings; a column whose rb status is set is
    replaced from the spares -> (planes, the recovered bits [B][N] as integers)"""
    scl, fx, rb, hm, port = env
    cols = B * N + spares
    r = R_lo[:, :cols]
    b, status = rb.random_bits(f, r, R_lo[:, cols:2 * cols], R_hi[:, cols:2 * cols], scl.lagrange_basis(f, n), scl.lagrange_basis(f, t + 1))
    bad = torch.nonzero(status[:B * N]).reshape(-1).tolist()
    good = [cols - 1 - i for i in range(spares) if not status[cols - 1 - i].item()]
    assert len(bad) <= len(good), (len(bad), len(good))
    for col, spare in zip(bad, good):
        b[:, col] = b[:, spare]
    b = b[:, :B * N].contiguous()
    opened = FXS.ints_of(f, host(scl.shamir_recover(f, b[:t + 1].contiguous())))
    assert set(opened.tolist()) == {0, 1}
    return b.view(n, B, N, O.LIMBS[f]).transpose(0, 1), opened.reshape(B, N)


@pytest.mark.parametrize("n,t", [(4, 1), (10, 3)], ids=["4-1", "10-3"])
@pytest.mark.parametrize("f", [O.M61, O.M127], ids=["m61", "m127"])
def test_truncation_end_to_end(env, f, n, t):
    """hm deals, rb.random_bits makes B * 257 bits (flagged columns replaced from spares), fx.trunc_pr truncates: shamir_recover of y
    -- from the first t + 1 shares and from the last -- equals the exact form in every column, computed from the recovered bits;
    both values of the carry occur"""
    scl, fx, rb, hm, port = env
    p, N, (B, k, shift) = FXS.prime(f), 257, (28, 20, 8)
    R_lo, R_hi = dealt(env, f, n, t, 2 * (B * N + 64), b"e2e")
    planes, bits = random_bit_planes(env, f, n, t, B, N, R_lo, R_hi)
    x = xs_of(p, k, (N,), 77 + n)
    xsh = dev(scl, f, FXS.a_share(p, x, t, n, 88 + n), None)
    y, status = fx.trunc_pr(f, xsh, planes, k, shift, lam=scl.lagrange_basis(f, t + 1))
    assert tuple(y.shape) == (n, N, O.LIMBS[f]) and not status.any().item()
    first = FXS.ints_of(f, host(scl.shamir_recover(f, y[:t + 1].contiguous())))
    nodes = np.stack([hm.element(f, i + 1) for i in range(n - t - 1, n)])
    last = FXS.ints_of(f, host(scl.shamir_recover(f, y[n - t - 1:].contiguous(), lam=scl.lagrange_basis(f, t + 1, nodes))))
    want = [FXS.exact_trunc(p, int(x[s]), [int(bits[i][s]) for i in range(B)], k, shift) for s in range(N)]
    assert first.tolist() == want and last.tolist() == want
    signed = lambda v: v if v < p // 2 else v - p
    plus_one = sum(signed(w) - (signed(int(v)) >> shift) for w, v in zip(want, x))
    assert 20 < plus_one < N - 20, plus_one


@pytest.mark.parametrize("f", [O.M61, O.M127], ids=["m61", "m127"])
def test_mul_trunc_is_the_fixed_point_product(env, f):
    """(n, t) = (4, 1), fixed-point encodings with 8 fractional bits: hm.mul_mask, hm.mul_finish and fx.trunc_pr in one call;
    the reconstructed product equals floor(x y / 2^8) plus the model's carry in every column"""
    scl, fx, rb, hm, port = env
    n, t, p, N, (B, k, shift) = 4, 1, FXS.prime(f), 257, (32, 24, 8)
    R_lo, R_hi = dealt(env, f, n, t, 2 * (B * N + 64) + N, b"mul")
    planes, bits = random_bit_planes(env, f, n, t, B, N, R_lo, R_hi)
    a = xs_of(p, 12, (N,), 5)                                       # |a|, |b| < 2^11: |a b| < 2^22 < 2^(k-1)
    b = xs_of(p, 12, (N,), 6)[::-1].copy()
    ash, bsh = dev(scl, f, FXS.a_share(p, a, t, n, 15), None), dev(scl, f, FXS.a_share(p, b, t, n, 16), None)
    z, status = fx.mul_trunc(f, ash, bsh, R_lo[:, -N:].contiguous(), R_hi[:, -N:].contiguous(), planes, k, shift, lam_2t=scl.lagrange_basis(f, n), lam_t=scl.lagrange_basis(f, t + 1))
    assert not status.any().item()
    got = FXS.ints_of(f, host(scl.shamir_recover(f, z[:t + 1].contiguous())))
    want = [FXS.exact_trunc(p, int(a[s]) * int(b[s]) % p, [int(bits[i][s]) for i in range(B)], k, shift) for s in range(N)]
    assert got.tolist() == want


_CAPTURE_CHILD = r"""
import json, sys
root = sys.argv[1]
sys.path[:0] = [root + "/secure-computation-library_amd", root + "/tests"]
import numpy as np
import torch
import fx_support as FXS
import scl_amd as scl
from scl_amd import fx

f, N, rows, m, (B, k, shift) = scl.M61, 257, 3, 2, (40, 30, 10)
p = FXS.prime(f)
torch.cuda.set_device(0)
bits, x, csh = scl.empty(f, B, rows, N), scl.empty(f, rows, N), scl.empty(f, m, N)
r, c, rlow, y = (scl.empty(f, rows, N) for _ in range(4))
status = torch.zeros(N, dtype=torch.uint8, device="cuda")
lam = FXS.limbs_of(f, np.array(FXS.lagrange_at_zero(p, m), dtype=object))
g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        fx.compose(f, bits, out=r)                                  # the first calls of this process
        fx.trunc_mask(f, x, bits, k, shift, out=c, rlow=rlow)
        fx.trunc_finish(f, csh, x, rlow, shift, B, lam=lam, out=y, status=status)
torch.cuda.synchronize()
planes, xv = FXS.uniform(p, (B, rows, N), 50), FXS.uniform(p, (rows, N), 51)
cv = FXS.uniform(p, (N,), 52) % (1 << (B + 1))
cv[3] = 1 << (B + 1)
bits.copy_(scl.to_device(FXS.limbs_of(f, planes)))
x.copy_(scl.to_device(FXS.limbs_of(f, xv)))
csh.copy_(scl.to_device(FXS.limbs_of(f, FXS.a_share(p, cv, m - 1, m, 53))))
for t in (r, c, rlow, y, status):
    t.fill_(7)
g.replay()
torch.cuda.synchronize()
wc, wl = FXS.a_mask(p, xv, planes, k, shift)
wy, ws = FXS.a_finish(p, cv, xv, wl, shift, B)
ints = lambda t: FXS.ints_of(f, scl.to_host(t))
assert (ints(r) == FXS.a_compose(p, planes)).all() and (ints(c) == wc).all() and (ints(rlow) == wl).all()
assert (ints(y) == wy).all() and status.cpu().numpy().tolist() == ws.tolist() and ws[3] == 1 and ws.sum() == 1
print(json.dumps({"ok": True, "replays": 1}))
"""


def test_the_three_calls_are_capturable_from_their_first_call():
    """a fresh child process captures scl_fx_compose, scl_fx_trunc_mask and scl_fx_trunc_finish into one graph as its first calls
    of the library and replays it once on new operands: r, c, rlow, y and the status equal the model"""
    r = subprocess.run([sys.executable, "-c", _CAPTURE_CHILD, FXS.cxx_support.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "replays": 1}


def test_wrapper_refuses_what_the_header_refuses(env):
    scl, fx = env[0], env[1]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device="cuda")
    x, bits = z(3, 8, 2), z(5, 3, 8, 2)
    for tag, word in ((O.GF2_128, "no integers below a prime"), (O.Z2K(64), "not a field")):
        with pytest.raises(scl.SclError) as ei:
            fx.trunc_mask(tag, x[..., :1].contiguous() if tag == O.Z2K(64) else x, bits[..., :1].contiguous() if tag == O.Z2K(64) else bits, 4, 2)
        assert ei.value.status == scl.ERR_BAD_ARG and word in str(ei.value)
    for k, shift, word in ((4, 0, "shift == 0"), (4, 4, "shift >= k"), (6, 2, "k > B")):
        with pytest.raises(scl.SclError) as ei:
            fx.trunc_mask(O.M127, x, bits, k, shift)
        assert ei.value.status == scl.ERR_BAD_ARG and word in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        fx.compose(O.M127, z(126, 8, 2))
    assert ei.value.status == scl.ERR_BAD_ARG and "B must be in 1..125" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        fx.trunc_mask(O.M127, x, bits, 4, 2, out=z(3, 9, 2))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        fx.trunc_mask(O.M127, x, bits, 4, 2, out=x, rlow=x)
    assert ei.value.status == scl.ERR_BAD_ARG and "overlaps" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        fx.trunc_finish(O.M127, z(65, 8, 2), x, x, 2, 5, lam=np.zeros((65, 2), dtype=np.uint64))
    assert ei.value.status == scl.ERR_BAD_ARG and "1..64" in str(ei.value)
    assert not x.any() and not bits.any()


def test_cxx_round_trips(env):
    """tests/cxx/test_fx_api.cc --gpu, a fresh child process: hip::composeBits, hip::truncMask and hip::truncFinish equal the host
    forms ss::composeBits, ss::truncMask and ss::truncFinish word for word"""
    r = subprocess.run([FXS.fx_api_binary(), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
