"""Exact comparison and truncation on the device (libscl_hip_cmp.so): scl_cmp_first_mask, scl_cmp_level_mask and scl_cmp_finish
against the Python-integer model of tests/cmp_support.py on every element -- all five prime fields, Mont128 at 2^128 - 159 and at
2^127 - 1; N in {1, 2, 257, 513} (the pair path of Mersenne61, its odd tail, a workgroup edge), rows in {1, 4}, pitched strides;
w in {1, 2, 3, 5} and the largest; for the wide fields w on both sides of every limb boundary; cnt in {2, 3, 7, 8} with and without
SCL_CMP_LT_ONLY (which is refused where more than one node comes out); operands whose every share is p - 1; an opened c at
2^(B+1) exactly, which sets the status and yields a zero column --, the pipelines end to end at (n, t) = (4, 1) and (10, 3) with
dealt bits that hit c' == r', r' = 0, r' = 2^w - 1 and the corners of x (trunc is exactly x >> w, never plus one; ltz is [x < 0];
lt is [x < y]), one run on bits from scl_amd.rb.random_bits, the three calls captured into a graph as the first calls of a fresh
process, and the C++ mirror.  Everything is exact."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import cmp_support as CS
import fx_support as FXS
import oracle_lib as O
from gpu_support import MONT_P, deal_all, gpu_env, host, only_the_view_was_written, placed

pytestmark = pytest.mark.gpu

CASES = FXS.CASES
IDS = [c[0] for c in CASES]
NS = [1, 2, 257, 513]
ROWS = [1, 4]
CNTS = [2, 3, 7, 8]


@pytest.fixture(scope="module")
def env():
    return gpu_env("cmp", "fx", "rb", "hm")


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


def elements(p, shape, seed, worst):
    """seeded elements, or p - 1 everywhere"""
    return np.full(shape, p - 1, dtype=object) if worst else FXS.uniform(p, shape, seed)


def ints(f, t, mp):
    return FXS.ints_of(f, host(t.contiguous()), mp)


def check_first(env, f, mp, p, w, B, N, rows, pitch, seed, worst=False):
    """first_mask at one shape against the model: d, cmod and the status; with w <= 2 under SCL_CMP_LT_ONLY as well"""
    scl, cmp = env[0], env[1]
    note = ("first", w, B, N, rows, pitch)
    m = 3
    bits = elements(p, (w, rows, N), seed, worst)
    c = FXS.uniform(p, (N,), seed + 1) % (1 << (B + 1))
    if worst:
        c[:] = (1 << (B + 1)) - 1
    if N >= 2:
        c[0], c[N - 1] = 1 << (B + 1), (1 << (B + 1)) - 1                # out of range exactly; the largest in range
    csh = FXS.a_share(p, c, m - 1, m, seed + 2)
    lam = FXS.limbs_of(f, np.array(FXS.lagrange_at_zero(p, m), dtype=object), mp)
    wc, ws = CS.a_open_col(c.copy(), w, B)
    assert N < 2 or (ws[0] == 1 and ws[N - 1] == 0 and wc[0] == 0), note
    bbuf, bv = placed(dev(scl, f, bits, mp), (pitch, w * pitch))
    sbuf, sv = placed(dev(scl, f, csh, mp), (pitch + 1,))
    for lt_only in ([False, True] if w <= 2 else [False]):
        P = 1 if lt_only else 2 * ((w + 1) // 2)
        r2 = elements(p, (P, rows, N), seed + 3, worst)
        rbuf, rv = placed(dev(scl, f, r2, mp), (pitch, P * pitch))
        before = (bbuf.clone(), sbuf.clone(), rbuf.clone())
        dbuf, dv = placed(torch.zeros(P, rows, N, FXS.limbs(f), dtype=torch.int64, device="cuda"), (pitch + 2, P * (pitch + 2)))
        _, cmod, status = cmp.first_mask(f, sv, bv, rv, w, B, lam=lam, flags=CS.LT_ONLY if lt_only else 0, out=dv)
        assert status.cpu().numpy().tolist() == ws.tolist(), note
        assert (ints(f, cmod, mp) == wc).all(), ("cmod",) + note
        assert (ints(f, dv, mp) == CS.a_first(p, wc, bits, r2, w, lt_only)).all(), ("d", lt_only) + note
        assert only_the_view_was_written(dbuf, dv), note
        assert torch.equal(bbuf, before[0]) and torch.equal(sbuf, before[1]) and torch.equal(rbuf, before[2]), note
    # the already opened form: m = 1, lambda = {1}
    d1, cmod1, st1 = cmp.first_mask(f, dev(scl, f, c, mp), bv, rv, w, B, flags=CS.LT_ONLY if w <= 2 else 0)
    assert torch.equal(d1, dv.contiguous()) and torch.equal(cmod1, cmod) and torch.equal(st1, status), ("opened",) + note


def check_level(env, f, mp, p, cnt, N, rows, pitch, seed, worst=False):
    scl, cmp = env[0], env[1]
    note = ("level", cnt, N, rows, pitch)
    nodes = elements(p, (2 * cnt, rows, N), seed, worst)
    nbuf, nv = placed(dev(scl, f, nodes, mp), (pitch, 2 * cnt * pitch))
    for lt_only in ([False, True] if cnt == 2 else [False]):
        P = 1 if lt_only else 2 * ((cnt + 1) // 2)
        r2 = elements(p, (P, rows, N), seed + 1, worst)
        rbuf, rv = placed(dev(scl, f, r2, mp), (pitch + 2, P * (pitch + 2)))
        before = (nbuf.clone(), rbuf.clone())
        dbuf, dv = placed(torch.zeros(P, rows, N, FXS.limbs(f), dtype=torch.int64, device="cuda"), (pitch + 4, P * (pitch + 4) + 2))
        cmp.level_mask(f, nv, rv, flags=CS.LT_ONLY if lt_only else 0, out=dv)
        assert (ints(f, dv, mp) == CS.a_level(p, nodes, r2, lt_only)).all(), (lt_only,) + note
        assert only_the_view_was_written(dbuf, dv), note
        assert torch.equal(nbuf, before[0]) and torch.equal(rbuf, before[1]), note
    if cnt > 2:
        with pytest.raises(scl.SclError) as ei:
            cmp.level_mask(f, nv, rv[:1], flags=CS.LT_ONLY)
        assert ei.value.status == scl.ERR_BAD_ARG and "single node" in str(ei.value), note


def check_finish(env, f, mp, p, w, N, rows, pitch, seed, worst=False):
    scl, cmp = env[0], env[1]
    note = ("finish", w, N, rows, pitch)
    lt, rlow, x = (elements(p, (rows, N), seed + i, worst) for i in range(3))
    cmod = FXS.uniform(p, (N,), seed + 3) % (1 << w)
    status = np.zeros(N, dtype=np.uint8)
    if N >= 2:
        status[0], cmod[0] = 1, 0
    bufs = [placed(dev(scl, f, a, mp), (pitch + 2 * i,)) for i, a in enumerate((lt, rlow, x))]
    (tbuf, tv), (lbuf, lv), (xbuf, xv) = bufs
    before = [b.clone() for b, _ in bufs]
    cd, sd = dev(scl, f, cmod, mp), torch.from_numpy(status).cuda()
    for what in (CS.MOD, CS.TRUNC, CS.LTZ):
        ybuf, yv = placed(torch.zeros(rows, N, FXS.limbs(f), dtype=torch.int64, device="cuda"), (pitch + 6,))
        cmp.finish(f, tv, cd, sd, lv, None if what == CS.MOD else xv, w, what, out=yv)
        assert (ints(f, yv, mp) == CS.a_finish(p, lt, cmod, status, rlow, x, w, what)).all(), (what,) + note
        assert only_the_view_was_written(ybuf, yv) and (N < 2 or not yv[:, 0].any().item()), note
    assert all(torch.equal(b, was) for (b, _), was in zip(bufs, before)), note


def widths(p):
    top = FXS.max_bits(p)
    return [1, 2, 3, 5, top - 1]


@pytest.mark.parametrize("which", range(5), ids=["w1", "w2", "w3", "w5", "largest"])
@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_the_three_calls_equal_the_model(env, modulus, name, f, mp, which):
    """N in {1, 2, 257, 513} x rows in {1, 4}; the pitch is N for one half and N + 3 for the other (Mersenne61: two columns per
    lane under the even strides, one under the odd ones).  At the largest w the wide fields take N = 65 (and 513 at one row for
    the 16-byte fields): the model is Python integers"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    w = widths(p)[which]
    B = min(FXS.max_bits(p), w + 7)
    shapes = [(N, rows) for N in NS for rows in ROWS]
    if which == 4 and FXS.limbs(f) > 1:
        shapes = [(65, 4)] + ([(513, 1)] if FXS.limbs(f) == 2 else [])
    for i, (N, rows) in enumerate(shapes):
        pitch, seed = N + 3 * (i % 2), 1000 * IDS.index(name) + 100 * which + i
        check_first(env, f, mp, p, w, B, N, rows, pitch, seed)
        check_finish(env, f, mp, p, w, N, rows, pitch, seed + 50)
        check_level(env, f, mp, p, CNTS[(i + which) % 4], N, rows, pitch, seed + 70)


@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_every_node_count_of_a_level(env, modulus, name, f, mp):
    """cnt in {2, 3, 7, 8} -- a pair, a lone last node, both at once -- at N = 2, 257 and rows = 1, 4, LT_ONLY at cnt == 2 and
    refused elsewhere"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    for i, cnt in enumerate(CNTS):
        for j, (N, rows) in enumerate([(2, 4), (257, 1), (257, 4)]):
            check_level(env, f, mp, p, cnt, N, rows, N + (i + j) % 2, 3000 + 100 * IDS.index(name) + 10 * i + j)


@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_every_share_p_minus_one(env, modulus, name, f, mp):
    """worst-case operands: p - 1 in every plane of the bits, the nodes, r2, lt, rlow and x, and the largest c in range"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    top = FXS.max_bits(p)
    for i, (w, N, rows) in enumerate([(top - 1, 3, 4), (5, 258, 1), (2, 65, 4)]):
        check_first(env, f, mp, p, w, top, N, rows, N + 1, 5000 + i, worst=True)
        check_finish(env, f, mp, p, w, N, rows, N + 1, 5100 + i, worst=True)
        check_level(env, f, mp, p, CNTS[i], N, rows, N + 1, 5200 + i, worst=True)
    check_level(env, f, mp, p, 8, 65, 4, 66, 5300, worst=True)


@pytest.mark.parametrize("name,f,mp", [c for c in CASES if c[1] != FXS.M61], ids=[i for i in IDS if i != "m61"])
def test_w_on_both_sides_of_every_limb_boundary(env, modulus, name, f, mp):
    """w in {63, 64, 65} for the 16-byte fields, and {127, 128, 129}, {191, 192, 193} for the 32-byte fields: the public bit is
    taken from any limb, the mask of c mod 2^w ends in any limb"""
    mp = modulus(mp)
    p = FXS.prime(f, mp)
    top = FXS.max_bits(p)
    ws = [w for edge in (64, 128, 192) if edge + 1 < top for w in (edge - 1, edge, edge + 1)]
    assert len(ws) == (9 if FXS.limbs(f) == 4 else 3)
    for i, w in enumerate(ws):
        N, rows = ((3, 4), (65, 1))[i % 2]
        check_first(env, f, mp, p, w, top, N, rows, N + 3, 7000 + 20 * IDS.index(name) + i)
        check_finish(env, f, mp, p, w, N, rows, N + 3, 7500 + 20 * IDS.index(name) + i)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
X_CORNERS = lambda k: [-(1 << (k - 1)), -1, 0, 1, (1 << (k - 1)) - 1]


def corner_columns(p, k, w, B, seed, extra=17):
    """(x [N] signed integers, bits [B][N] of 0 / 1): every corner of x under low bits that are all zero (r' = 0), all one
    (r' = 2^w - 1) and seeded -- x = 0 and x = -2^(k-1) have x mod 2^w = 0, which is c' == r' under any bits --, then seeded columns"""
    xs, cols = [], []
    for kind in ("zero", "ones", "any"):
        for x in X_CORNERS(k):
            xs.append(x)
            cols.append(CS.corner_bits(w, B, kind, seed + len(xs)))
    for i in range(extra):
        xs.append(FXS.seeded(p, 1, seed + 100 + i)[0] % (1 << k) - (1 << (k - 1)))
        cols.append(CS.corner_bits(w, B, "any", seed + 200 + i))
    return np.array(xs, dtype=object), np.array(cols, dtype=object).T.copy()


def double_sharings(env, f, p, n, t, count, seed):
    """`count` double sharings of seeded values for all n parties, from the model: (R_lo, R_hi) [n][count][L]"""
    scl = env[0]
    r = FXS.uniform(p, (count,), seed)
    return dev(scl, f, FXS.a_share(p, r, t, n, seed + 1), None), dev(scl, f, FXS.a_share(p, r, 2 * t, n, seed + 50), None)


def opened(env, f, y, n, t):
    """a degree-t sharing [n][N][L] recovered from the first t + 1 shares and from the last: both, as signed integers"""
    scl, hm = env[0], env[4]
    p = FXS.prime(f)
    first = FXS.ints_of(f, host(scl.shamir_recover(f, y[:t + 1].contiguous())))
    nodes = np.stack([hm.element(f, i + 1) for i in range(n - t - 1, n)])
    last = FXS.ints_of(f, host(scl.shamir_recover(f, y[n - t - 1:].contiguous(), lam=scl.lagrange_basis(f, t + 1, nodes))))
    assert first.tolist() == last.tolist()
    return [CS.signed(p, int(v)) for v in first]


@pytest.mark.parametrize("n,t", [(4, 1), (10, 3)], ids=["4-1", "10-3"])
@pytest.mark.parametrize("f", [O.M61, O.M127], ids=["m61", "m127"])
def test_the_pipelines_end_to_end(env, f, n, t):
    """dealt bits that hit c' == r', r' = 0, r' = 2^w - 1 and the corners of x: the recovered trunc is exactly x >> w, mod2m is
    x mod 2^w, ltz is [x < 0] and lt(x, y) is [x < y], in every column; the opened c' and r' are checked to hit the corners"""
    scl, cmp = env[0], env[1]
    p, k, B, w = FXS.prime(f), 16, 20, 8
    x, bits = corner_columns(p, k, w, B, 40 + n)
    N = len(x)
    rlow = [sum(int(bits[i][s]) << i for i in range(w)) for s in range(N)]
    cprime = [(int(x[s]) + rlow[s]) % (1 << w) for s in range(N)]
    assert any(c == r for c, r in zip(cprime, rlow)) and 0 in rlow and (1 << w) - 1 in rlow
    assert any(c < r for c, r in zip(cprime, rlow)) and any(c > r for c, r in zip(cprime, rlow))
    xsh = dev(scl, f, FXS.a_share(p, x % p, t, n, 60 + n), None)
    planes = dev(scl, f, np.stack([FXS.a_share(p, bits[i], t, n, 70 + i) for i in range(B)]), None)
    lam_t, lam_2t = scl.lagrange_basis(f, t + 1), scl.lagrange_basis(f, 2 * t + 1)
    R_lo, R_hi = double_sharings(env, f, p, n, t, cmp.planes(k) * N, 90 + n)
    y, status = cmp.trunc(f, xsh, planes, R_lo, R_hi, k, w, lam_t=lam_t, lam_2t=lam_2t)
    assert not status.any().item() and opened(env, f, y, n, t) == [int(v) >> w for v in x]
    y, status = cmp.mod2m(f, xsh, planes, R_lo, R_hi, k, w)                                    # the default bases: all n shares
    assert not status.any().item() and opened(env, f, y, n, t) == [int(v) % (1 << w) for v in x]
    y, status = cmp.ltz(f, xsh, planes, R_lo, R_hi, k, lam_t=lam_t, lam_2t=lam_2t)
    assert not status.any().item() and opened(env, f, y, n, t) == [int(v < 0) for v in x]
    yv = np.roll(x, 7)
    yv[:5] = x[:5]                                                                             # x == y among them
    ysh = dev(scl, f, FXS.a_share(p, yv % p, t, n, 95 + n), None)
    z, status = cmp.lt(f, xsh, ysh, planes, R_lo, R_hi, k, lam_t=lam_t, lam_2t=lam_2t)
    want = [int(a < b) for a, b in zip(x, yv)]
    assert not status.any().item() and opened(env, f, z, n, t) == want and 0 < sum(want) < N


def test_trunc_on_random_bits(env):
    """(n, t) = (4, 1) over Mersenne61: hm deals and extracts, rb.random_bits makes B N shared bits (flagged columns replaced from
    spares), cmp.trunc at w = 8: exactly x >> 8 in every column"""
    scl, cmp, fx, rb, hm, port = env
    f, n, t, N, (B, k, w) = O.M61, 4, 1, 64, (14, 12, 8)
    p, L, m, spares = FXS.prime(f), 1, 3, 32
    cols = B * N + spares
    count = 2 * cols + cmp.planes(w) * N
    S = -(-count // m)
    z = lambda *shape: torch.zeros(*shape, L, dtype=torch.int64, device="cuda")
    lo, hi, R_lo, R_hi = z(n, n, S), z(n, n, S), z(n, m, S), z(n, m, S)
    deal_all(hm, f, S, t, n, [b"cmp rb dealer %d" % i for i in range(n)], lo, hi)
    Md = scl.to_device(hm.hyper_invertible(f, m, n))
    hm.apply_matrix(f, Md, lo.transpose(0, 1), out=R_lo)
    hm.apply_matrix(f, Md, hi.transpose(0, 1), out=R_hi)
    R_lo, R_hi = R_lo.reshape(n, m * S, L)[:, :count], R_hi.reshape(n, m * S, L)[:, :count]
    b, status = rb.random_bits(f, R_lo[:, :cols], R_lo[:, cols:2 * cols], R_hi[:, cols:2 * cols], scl.lagrange_basis(f, n), scl.lagrange_basis(f, t + 1))
    bad = torch.nonzero(status[:B * N]).reshape(-1).tolist()
    good = [cols - 1 - i for i in range(spares) if not status[cols - 1 - i].item()]
    assert len(bad) <= len(good), (len(bad), len(good))
    for col, spare in zip(bad, good):
        b[:, col] = b[:, spare]
    planes = b[:, :B * N].contiguous().view(n, B, N, L).transpose(0, 1)
    x = np.array([v % (1 << k) - (1 << (k - 1)) for v in FXS.seeded(p, N, 9)], dtype=object)
    x[:5] = X_CORNERS(k)
    xsh = dev(scl, f, FXS.a_share(p, x % p, t, n, 10), None)
    y, status = cmp.trunc(f, xsh, planes, R_lo[:, 2 * cols:].contiguous(), R_hi[:, 2 * cols:].contiguous(), k, w, lam_t=scl.lagrange_basis(f, t + 1))
    assert not status.any().item() and opened((scl, cmp, fx, rb, hm), f, y, n, t) == [int(v) >> w for v in x]


_CAPTURE_CHILD = r"""
import json, sys
root = sys.argv[1]
sys.path[:0] = [root + "/secure-computation-library_amd", root + "/tests"]
import numpy as np
import torch
import cmp_support as CS
import fx_support as FXS
import scl_amd as scl
from scl_amd import cmp

f, N, rows, m, (w, B, cnt) = scl.M61, 257, 3, 2, (5, 12, 3)
p = FXS.prime(f)
torch.cuda.set_device(0)
P1, P2 = 2 * ((w + 1) // 2), 2 * ((cnt + 1) // 2)
bits, csh, r2a, d1 = scl.empty(f, w, rows, N), scl.empty(f, m, N), scl.empty(f, P1, rows, N), scl.empty(f, P1, rows, N)
r2b, d2 = scl.empty(f, P2, rows, N), scl.empty(f, P2, rows, N)
lt, rlow, x, y = (scl.empty(f, rows, N) for _ in range(4))
cmod, status = scl.empty(f, N), torch.zeros(N, dtype=torch.uint8, device="cuda")
lam = FXS.limbs_of(f, np.array(FXS.lagrange_at_zero(p, m), dtype=object))
g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        cmp.first_mask(f, csh, bits, r2a, w, B, lam=lam, out=d1, cmod=cmod, status=status)      # the first calls of this process
        cmp.level_mask(f, d1, r2b, out=d2)
        cmp.finish(f, lt, cmod, status, rlow, x, w, cmp.TRUNC, out=y)
torch.cuda.synchronize()
vb, vr1, vr2 = FXS.uniform(p, (w, rows, N), 50), FXS.uniform(p, (P1, rows, N), 51), FXS.uniform(p, (P2, rows, N), 52)
vl, vlow, vx = (FXS.uniform(p, (rows, N), 53 + i) for i in range(3))
cv = FXS.uniform(p, (N,), 56) % (1 << (B + 1))
cv[3] = 1 << (B + 1)
up = lambda t, v: t.copy_(scl.to_device(FXS.limbs_of(f, v)))
up(bits, vb), up(r2a, vr1), up(r2b, vr2), up(lt, vl), up(rlow, vlow), up(x, vx), up(csh, FXS.a_share(p, cv, m - 1, m, 57))
for t in (d1, d2, y, cmod, status):
    t.fill_(7)
g.replay()
torch.cuda.synchronize()
wc, ws = CS.a_open_col(cv.copy(), w, B)
wd1 = CS.a_first(p, wc, vb, vr1, w)
ints = lambda t: FXS.ints_of(f, scl.to_host(t))
assert (ints(cmod) == wc).all() and status.cpu().numpy().tolist() == ws.tolist() and ws[3] == 1 and ws.sum() == 1
assert (ints(d1) == wd1).all() and (ints(d2) == CS.a_level(p, wd1[:2 * cnt], vr2)).all()
assert (ints(y) == CS.a_finish(p, vl, wc, ws, vlow, vx, w, CS.TRUNC)).all()
print(json.dumps({"ok": True, "replays": 1}))
"""


def test_the_three_calls_are_capturable_from_their_first_call():
    """a fresh child process captures scl_cmp_first_mask, scl_cmp_level_mask and scl_cmp_finish into one graph as its first calls
    of the library and replays it once on new operands: d, cmod, the status and y equal the model"""
    r = subprocess.run([sys.executable, "-c", _CAPTURE_CHILD, FXS.cxx_support.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "replays": 1}


def test_wrapper_refuses_what_the_header_refuses(env):
    scl, cmp = env[0], env[1]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device="cuda")
    csh, bits, r2, nodes = z(3, 8, 2), z(5, 3, 8, 2), z(6, 3, 8, 2), z(6, 3, 8, 2)
    lt, cmod, st = z(3, 8, 2), z(8, 2), torch.zeros(8, dtype=torch.uint8, device="cuda")
    one = lambda t: t[..., :1].contiguous()
    for tag, word in ((O.GF2_128, "no integers below a prime"), (O.Z2K(64), "not a field")):
        ring = tag == O.Z2K(64)
        with pytest.raises(scl.SclError) as ei:
            cmp.level_mask(tag, one(nodes) if ring else nodes, one(r2[:4]) if ring else r2[:4])
        assert ei.value.status == scl.ERR_BAD_ARG and word in str(ei.value)
    refused = [(lambda: cmp.first_mask(O.M127, csh, bits, r2, 0, 9), "w == 0"), (lambda: cmp.first_mask(O.M127, csh, bits, r2, 5, 5), "w >= B"),
               (lambda: cmp.first_mask(O.M127, csh, bits, r2, 5, 126), "B > |p| - 2"),
               (lambda: cmp.first_mask(O.M127, z(65, 8, 2), bits, r2, 5, 9, lam=np.zeros((65, 2), dtype=np.uint64)), "1..64"),
               (lambda: cmp.first_mask(O.M127, csh, bits, r2[:1], 5, 9, flags=cmp.LT_ONLY), "single node"),
               (lambda: cmp.first_mask(O.M127, csh, bits, r2, 5, 9, flags=2), "unknown flag"),
               (lambda: cmp.first_mask(O.M127, csh, bits, r2, 5, 9, out=r2), "overlaps"),
               (lambda: cmp.level_mask(O.M127, nodes[:2], r2[:2]), "cnt < 2"),
               (lambda: cmp.finish(O.M127, lt, cmod, st, lt, lt, 3, 7), "unknown `what`"),
               (lambda: cmp.finish(O.M127, lt, cmod, st, lt, None, 3, cmp.TRUNC), "x_dev is NULL"),
               (lambda: cmp.finish(O.M127, lt, cmod, st, lt, lt, 125, cmp.MOD), "w >= |p| - 2")]
    for call, word in refused:
        with pytest.raises(scl.SclError) as ei:
            call()
        assert ei.value.status == scl.ERR_BAD_ARG and word in str(ei.value), (word, str(ei.value))
    with pytest.raises(scl.SclError) as ei:
        cmp.first_mask(O.M127, csh, bits, r2[:4], 5, 9)
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    assert not any(t.any().item() for t in (csh, bits, r2, nodes, lt, cmod, st))


def test_cxx_round_trips(env):
    """tests/cxx/test_cmp_api.cc --gpu, a fresh child process: hip::cmpFirstMask, hip::cmpLevelMask and hip::cmpFinish equal the
    host forms of ss/compare.h word for word"""
    r = subprocess.run([CS.cmp_api_binary(), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
