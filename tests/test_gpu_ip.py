"""Inner and matrix products of Shamir sharings at one opening on the GPU (scl_amd.ip over libscl_hip_ip.so) against the Python
model of tests/port_models.py, which tests/test_ip_host.py pins to what the reference produced: device output equals the model byte for byte.
Each test's docstring names its shapes.  One model run per field at the largest shape -- the sums are prefix sums over the terms
and every smaller N is a prefix of the columns -- uploaded once; every layout is a device copy of it."""
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
from cxx_support import mirror_binary
from gpu_support import deal_all, fname, gpu_env, host, only_the_view_was_written, placed, pm1, pool, rnd
from gpu_support import hm_chain_buffers as chain_buffers
from port_models import TAGS3 as TAGS
from port_models import ew as _ew
from port_models import golden, inner_entry, matrix_entry, model_dot_mask, model_matmul_mask

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
TERMS = [1, 2, 7, 64, 65]
ROWS = [1, 10]
NS = [1, 2, 3, 64, 257, 1025]
NMAX, TMAX, RMAX = max(NS), max(TERMS), max(ROWS)
WORST_TERMS = [63, 64, 65, 127, 128, 129, 300]
SHAPES = [(1, 1, 1), (2, 3, 2), (4, 4, 4), (5, 7, 3), (3, 65, 2), (9, 2, 9)]
MAT_NS = [1, 3, 64, 257]


@pytest.fixture(scope="module")
def env():
    return gpu_env("hm", "ip")


def pitches(f, N):
    """row pitches: N, an even one larger than N (Mersenne61: two columns per lane) and an odd one"""
    return [N, N + 2 + (N % 2), N + 3 + (N % 2)]


_DOT = {}


def dot_reference(scl, port, f):
    """x, y [TMAX][RMAX][NMAX][L], r [RMAX][NMAX][L] on the device and, per term count, the model's sums without and with r"""
    if f not in _DOT:
        L = O.LIMBS[f]
        x = pool(port, f, TMAX * RMAX * NMAX, b"ip-x").reshape(TMAX, RMAX, NMAX, L)
        y = pool(port, f, TMAX * RMAX * NMAX + 11, b"ip-y")[11:].reshape(TMAX, RMAX, NMAX, L)
        r = pool(port, f, RMAX * NMAX, b"ip-r").reshape(RMAX, NMAX, L)
        want, acc = {}, None
        for k in range(TMAX):                                    # prefix sums: one pass serves every term count
            prod = _ew(port, f, O.MUL, x[k], y[k])
            acc = prod if acc is None else _ew(port, f, O.ADD, acc, prod)
            if k + 1 in TERMS:
                want[k + 1] = (acc, _ew(port, f, O.ADD, acc, r))
        assert np.array_equal(want[7][1][:, :5], model_dot_mask(port, f, x[:7, :, :5], y[:7, :, :5], r[:, :5]))
        _DOT[f] = (scl.to_device(x), scl.to_device(y), scl.to_device(r), want)
    return _DOT[f]


# ---- dot ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_dot_equals_the_model(env, f):
    """terms 1, 2, 7, 64, 65 x rows 1, 10 x N 1, 2, 3, 64, 257, 1025 (the one-limb field also 513: 256 pairs fill block 0 and the
    tail is lane 0 of block 1) x the three row pitches (x the two base phases for the one-limb field: 8 bytes past a 16-byte
    boundary is the one-column fallback, an even pitch at phase 0 the two-column path with its tail lane at odd N), and an odd
    term stride at N = 3 and 257: with r2, without it and in place on r2; the inputs are unchanged, the gaps between rows
    unwritten; terms == 1 is hm.mul_mask on the same buffers"""
    scl, hm, ip, port = env
    xd, yd, rd, want = dot_reference(scl, port, f)
    for terms in TERMS:
        w0, w1 = want[terms]
        for rows in ROWS:
            for N in (sorted(NS + [513]) if O.LIMBS[f] == 1 else NS):
                x, y, r = xd[:terms, :rows, :N], yd[:terms, :rows, :N], rd[:rows, :N]
                cases = [(p, ph, 0) for p in pitches(f, N) for ph in ((0, 1) if O.LIMBS[f] == 1 else (0,))]
                if N in (3, 257):
                    cases.append((pitches(f, N)[1], 0, 1))
                for pitch, phase, tgap in cases:
                    note = f"{fname(f)} dot terms={terms} rows={rows} N={N} pitch={pitch} phase={phase} tgap={tgap}"
                    _, xv = placed(x, (rows * pitch + tgap, pitch), phase)
                    _, yv = placed(y, (rows * pitch + tgap, pitch), phase)
                    rbuf, rv = placed(r, (pitch,), phase)
                    dbuf, dv = placed(torch.zeros_like(r), (pitch + 2,), phase)
                    got = ip.dot_mask(f, xv, yv, rv, out=dv)
                    assert got.data_ptr() == dv.data_ptr()
                    assert np.array_equal(host(dv), w1[:rows, :N]), note
                    assert only_the_view_was_written(dbuf, dv), note + ": a gap was written"
                    if terms == 1:
                        assert torch.equal(hm.mul_mask(f, xv[0], yv[0], rv), dv), note + ": differs from hm.mul_mask"
                    dv.zero_()
                    ip.dot_mask(f, xv, yv, None, out=dv)
                    assert np.array_equal(host(dv), w0[:rows, :N]), note + " without r2"
                    assert torch.equal(xv, x) and torch.equal(yv, y) and torch.equal(rv, r), note + ": an input changed"
                    ip.dot_mask(f, xv, yv, rv, out=rv)                                   # in place
                    assert np.array_equal(host(rv), w1[:rows, :N]), note + " in place"
                    assert only_the_view_was_written(rbuf, rv), note + " in place: a gap was written"
    # one row given as [terms][N][L] and [N][L]; x == y: sums of squares
    got = ip.dot_mask(f, xd[:7, 0, :67], yd[:7, 0, :67], rd[0, :67])
    assert got.shape == (67, O.LIMBS[f]) and np.array_equal(host(got), want[7][1][0, :67])
    sq = host(ip.dot_mask(f, xd[:7, :, :67], xd[:7, :, :67]))
    xs = host(xd[:7, :, :67])
    assert np.array_equal(sq, model_dot_mask(port, f, xs, xs))


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_dot_equals_the_composition_at_full_width(env, f):
    """rows = 10, N = 1025, terms = 7 and 65, on the device over every column: hm.mul_mask, then scl.ew MUL and ADD per further
    term -- what a caller composes today"""
    scl, hm, ip, port = env
    xd, yd, rd, _ = dot_reference(scl, port, f)
    for terms in (7, 65):
        acc = hm.mul_mask(f, xd[0], yd[0], rd)
        for k in range(1, terms):
            acc = scl.ew(f, scl.ADD, acc, scl.ew(f, scl.MUL, xd[k].contiguous(), yd[k].contiguous()))
        assert torch.equal(ip.dot_mask(f, xd[:terms], yd[:terms], rd), acc), f"{fname(f)} terms={terms}"


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_dot_at_the_worst_case(env, f):
    """every operand p - 1 (GF(2^128): all ones), terms 63, 64, 65, 127, 128, 129, 300, with and without r2, rows = 2, N = 3.
    Mersenne61 holds 64 terms: 63 products and the addend meet the bound, 64 products and the addend pass it (the fold BEFORE
    the addend), 127 / 128 / 129 pass it twice with the addend on each side of the second fold, 300 five times; a kernel that
    does not fold overflows 128 bits from 65 terms on.  The other fields' bounds (2^24 terms and above) cannot be reached in a
    test: for them this is the largest-operand case of the plain accumulation."""
    scl, hm, ip, port = env
    top, rows, N = pm1(port, f), 2, 3
    sq = port.ew(f, O.MUL, top[None], top[None])
    acc, want = None, {}
    for k in range(max(WORST_TERMS)):
        acc = sq if acc is None else port.ew(f, O.ADD, acc, sq)
        if k + 1 in WORST_TERMS:
            want[k + 1] = (acc[0], port.ew(f, O.ADD, acc, top[None])[0])
    full = lambda e, *lead: np.broadcast_to(e, lead + e.shape).copy()
    ops = scl.to_device(full(top, max(WORST_TERMS), rows, N))
    r = scl.to_device(full(top, rows, N))
    for terms in WORST_TERMS:
        assert np.array_equal(host(ip.dot_mask(f, ops[:terms], ops[:terms], r)), full(want[terms][1], rows, N)), f"{fname(f)} terms={terms} with r2"
        assert np.array_equal(host(ip.dot_mask(f, ops[:terms], ops[:terms])), full(want[terms][0], rows, N)), f"{fname(f)} terms={terms}"


# ---- matmul ------------------------------------------------------------------------------------------------------------------
def test_the_shapes_reach_every_tile_edge(env):
    """for every field at least one shape has a % TI != 0 and one has b % TL != 0 (the clamped rows and columns), and one is the
    1 x 1 route"""
    scl, hm, ip, port = env
    for f in FIELDS:
        ti, tl = ip.matmul_tile(f)
        assert any(a % ti for a, _, _ in SHAPES) and any(b % tl for _, _, b in SHAPES), fname(f)
        assert any(a > ti and b > tl for a, _, b in SHAPES), fname(f)            # more than one tile on both axes
    assert (1, 1, 1) in SHAPES


def model_columns(batch, N):
    """the columns the model checks: all where there are at most 300, else the head and the tail of every batch"""
    if batch * N <= 300:
        return np.arange(N)
    half = 150 // batch
    return np.concatenate([np.arange(half), np.arange(N - half, N)])


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_matmul_equals_dot_and_the_model(env, f):
    """(a,K,b) in (1,1,1) (2,3,2) (4,4,4) (5,7,3) (3,65,2) (9,2,9) x batch 1, 3 (batch strides five rows larger than the
    matrices) x N 1, 3, 64, 257, the entry pitch cycling through the three pitches: with r2, without, in place.  Compared at full
    width on the device with a b calls of dot_mask through term strides (the matrix layout is expressible that way), and with the
    model on at most 300 columns (the oracle's products are the cost of that comparison); gaps unwritten, inputs unchanged"""
    scl, hm, ip, port = env
    L, BM, NM = O.LIMBS[f], 3, max(MAT_NS)
    for si, (a, K, b) in enumerate(SHAPES):
        Xh = pool(port, f, BM * a * K * NM, b"ip-X%d" % si).reshape(BM, a, K, NM, L)
        Yh = pool(port, f, BM * K * b * NM + 7, b"ip-Y%d" % si)[7:].reshape(BM, K, b, NM, L)
        Rh = pool(port, f, BM * a * b * NM, b"ip-R%d" % si).reshape(BM, a, b, NM, L)
        Xd, Yd, Rd = scl.to_device(Xh), scl.to_device(Yh), scl.to_device(Rh)
        for batch in (1, BM):
            for ni, N in enumerate(MAT_NS):
                pitch = pitches(f, N)[(si + ni + batch) % 3]
                bs = (max(a * K, K * b, a * b) + 5) * pitch                  # one batch stride for all: dot_mask's op_stride
                note = f"{fname(f)} matmul ({a},{K},{b}) batch={batch} N={N} pitch={pitch}"
                X, Y, R = Xd[:batch, :, :, :N], Yd[:batch, :, :, :N], Rd[:batch, :, :, :N]
                _, Xv = placed(X, (bs, K * pitch, pitch))
                _, Yv = placed(Y, (bs, b * pitch, pitch))
                rbuf, Rv = placed(R, (bs, b * pitch, pitch))
                dbuf, Dv = placed(torch.zeros_like(R), (bs, b * pitch, pitch))
                arg = (lambda t: t) if batch > 1 else (lambda t: t[0])
                ip.matmul_mask(f, arg(Xv), arg(Yv), arg(Rv), out=arg(Dv))
                assert only_the_view_was_written(dbuf, Dv), note + ": a gap was written"
                ref = torch.zeros_like(R)
                for i in range(a):
                    for l in range(b):
                        ip.dot_mask(f, Xv[:, i].transpose(0, 1), Yv[:, :, l].transpose(0, 1), Rv[:, i, l], out=ref[:, i, l])
                assert torch.equal(Dv, ref), note + ": differs from a b calls of dot_mask"
                cols = model_columns(batch, N)
                sel = lambda t: np.ascontiguousarray(t[:batch][:, :, :, cols])
                assert np.array_equal(host(Dv)[:, :, :, cols], model_matmul_mask(port, f, sel(Xh), sel(Yh), sel(Rh))), note + ": differs from the model"
                none = ip.matmul_mask(f, arg(Xv), arg(Yv))
                assert none.shape == arg(Dv).shape
                assert np.array_equal(host(none).reshape(Dv.shape)[:, :, :, cols], model_matmul_mask(port, f, sel(Xh), sel(Yh))), note + " without r2"
                assert torch.equal(Xv, X) and torch.equal(Yv, Y) and torch.equal(Rv, R), note + ": an input changed"
                ip.matmul_mask(f, arg(Xv), arg(Yv), arg(Rv), out=arg(Rv))            # in place
                assert torch.equal(Rv, ref), note + " in place"
                assert only_the_view_was_written(rbuf, Rv), note + " in place: a gap was written"


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_matmul_at_the_worst_case(env, f):
    """every operand p - 1 at K = 65 and K = 129, a 3 x 2 result (a clamped tile edge for every field), batch 2, N = 3: Mersenne61
    folds the whole tile once and twice on the way, and at K = 128 once more for the addend"""
    scl, hm, ip, port = env
    top, N = pm1(port, f), 3
    full = lambda e, *lead: np.broadcast_to(e, lead + e.shape).copy()
    for K in (65, 128, 129):
        X, Y, R = full(top, 2, 3, K, N), full(top, 2, K, 2, N), full(top, 2, 3, 2, N)
        for r2 in (None, R):
            got = host(ip.matmul_mask(f, scl.to_device(X), scl.to_device(Y), None if r2 is None else scl.to_device(r2)))
            assert np.array_equal(got, model_matmul_mask(port, f, X, Y, r2)), f"{fname(f)} K={K} r2={r2 is not None}"


# ---- the protocol ------------------------------------------------------------------------------------------------------------
def test_the_fixture_end_to_end_on_the_device(env):
    """every entry of golden_ip.json: the shares of x_k and y_k rebuilt by the model -> dot_mask (matmul_mask) -> hm.mul_finish
    -> scl.shamir_recover; every intermediate equals what the reference computed"""
    scl, hm, ip, port = env
    g = golden("ip")
    for e in g["inner"]:
        f = TAGS[e["field"]]
        xs, ys, lo, hi, want = inner_entry(port, f, e)
        note = (e["field"], e["n"], e["K"])
        d = ip.dot_mask(f, scl.to_device(xs), scl.to_device(ys), scl.to_device(hi))
        assert np.array_equal(host(d), want["d_shares"]), note
        assert np.array_equal(host(scl.shamir_recover(f, d)), want["d"]), note
        z = hm.mul_finish(f, d, scl.to_device(lo))
        assert np.array_equal(host(z), want["z_shares"]), note
        assert np.array_equal(host(scl.shamir_recover(f, z)), want["z"]), note
        assert np.array_equal(host(scl.shamir_recover(f, z[:e["t"] + 1])), want["z"]), note
    for e in g["matrix"]:
        f = TAGS[e["field"]]
        X, Y, lo, hi, want = matrix_entry(port, f, e)
        n, a, b, L = e["n"], e["a"], e["b"], O.LIMBS[f]
        d = ip.matmul_mask(f, scl.to_device(X), scl.to_device(Y), scl.to_device(hi))
        assert np.array_equal(host(d), want["d_shares"]), e["field"]
        cols = d.reshape(n, a * b, L)                                   # the output as a b N columns per party: the pitch equals N
        assert np.array_equal(host(scl.shamir_recover(f, cols)), want["d"]), e["field"]
        z = hm.mul_finish(f, cols, scl.to_device(lo).reshape(n, a * b, L))
        assert np.array_equal(host(z).reshape(want["z_shares"].shape), want["z_shares"]), e["field"]
        assert np.array_equal(host(scl.shamir_recover(f, z)), want["z"]), e["field"]


def ip_buffers(f, n, t, S, K):
    B = chain_buffers(f, n, t, S)
    B["xs"], B["ys"] = [torch.zeros(K, n, (n - t) * S, O.LIMBS[f], dtype=torch.int64, device="cuda") for _ in range(2)]
    return B


def run_chain(scl, hm, ip, f, n, t, S, P, seeds, Md, xs, ys, lam, B, scratch=None, flags=0):
    """ten dealers deal -> the extraction at both degrees -> dot_mask -> mul_finish -> recover"""
    L, m = O.LIMBS[f], n - t
    deal_all(hm, f, S, t, n, seeds, B["lo"], B["hi"], scratch, flags)
    hm.apply_matrix(f, Md, B["lo"].transpose(0, 1), out=B["R_lo"])
    hm.apply_matrix(f, Md, B["hi"].transpose(0, 1), out=B["R_hi"])
    r_lo, r_hi = B["R_lo"].reshape(n, m * S, L)[:, :P], B["R_hi"].reshape(n, m * S, L)[:, :P]
    ip.dot_mask(f, xs, ys, r_hi, out=B["d"][:, :P])
    hm.mul_finish(f, B["d"][:, :P], r_lo, lam=lam, out=B["z"][:, :P])
    scl.shamir_recover(f, B["z"][:, :P], lam=lam, out=B["out"][:P])


def chain_inputs(scl, port, f, n, t, K, P, B, tag):
    """K x P secrets and their degree-t sharings at the pitch of the extracted rows -> x, y [K][P][L] (host), views [K][n][P][L]"""
    x, y = [rnd(port, f, K * P, tag + s).reshape(K, P, -1) for s in (b"-x", b"-y")]
    for k in range(K):
        B["xs"][k, :, :P] = scl.shamir_share_prg(f, scl.to_device(x[k]), t, n, tag + b"-xs%d" % k)
        B["ys"][k, :, :P] = scl.shamir_share_prg(f, scl.to_device(y[k]), t, n, tag + b"-ys%d" % k)
    return x, y, B["xs"][:, :, :P], B["ys"][:, :, :P]


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_inner_products_without_a_dealer(env, f):
    """(10,3), K = 8, 257 inner products: ten dealers deal with hm.double_share (37 double sharings each, 7 x 37 = 259 extracted,
    the first 257 used), hm.apply_matrix at both degrees, ip.dot_mask, hm.mul_finish, recover: port.dot of the secrets, and [z]
    recovers from any t + 1 rows"""
    scl, hm, ip, port = env
    n, t, S, P, K = 10, 3, 37, 257, 8
    B = ip_buffers(f, n, t, S, K)
    x, y, xs, ys = chain_inputs(scl, port, f, n, t, K, P, B, b"ip-chain")
    seeds = [b"ip dealer %d" % i for i in range(n)]
    run_chain(scl, hm, ip, f, n, t, S, P, seeds, scl.to_device(hm.hyper_invertible(f, n - t, n)), xs, ys, scl.lagrange_basis(f, n), B)
    want = np.stack([port.dot(f, np.ascontiguousarray(x[:, s]), np.ascontiguousarray(y[:, s])) for s in range(P)])
    assert np.array_equal(host(B["out"])[:P], want)
    for rows in ([0, 1, 2, 3], [6, 7, 8, 9], [1, 4, 5, 8]):
        lam = scl.lagrange_basis(f, t + 1, alphas=np.stack([port.from_int(f, i + 1) for i in rows]))
        assert np.array_equal(host(scl.shamir_recover(f, B["z"][rows, :P].contiguous(), lam=lam)), want), rows


@pytest.mark.parametrize("f,flags", [(O.M61, 0), (O.SECP256K1_SCALAR, 0)], ids=["m61", "secp_scalar"])
def test_the_chain_captured_into_one_graph(env, f, flags):
    """the chain above on one stream, captured as a linear chain (no parallel branches) and replayed once with every buffer
    cleared in between.  The two-pass deal's scratch is the caller's and its engine tables exist after the run before the
    capture, as scl_hip_hm.h asks; dot_mask itself is capturable from its first call"""
    scl, hm, ip, port = env
    n, t, S, P, K = 10, 3, 37, 257, 8
    need = hm.double_scratch_bytes(f, S, n, t, flags)
    scratch = torch.zeros(need // 8, dtype=torch.int64, device="cuda") if need else None
    B = ip_buffers(f, n, t, S, K)
    x, y, xs, ys = chain_inputs(scl, port, f, n, t, K, P, B, b"ip-graph")
    inputs = {k: B.pop(k) for k in ("xs", "ys")}                       # (not cleared between the runs: they are the chain's inputs)
    lam = scl.lagrange_basis(f, n)
    Md = scl.to_device(hm.hyper_invertible(f, n - t, n))
    seeds = [b"ip graph dealer %d" % i for i in range(n)]
    chain = lambda: run_chain(scl, hm, ip, f, n, t, S, P, seeds, Md, xs, ys, lam, B, scratch, flags)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                   # every kernel has run once before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = np.stack([port.dot(f, np.ascontiguousarray(x[:, s]), np.ascontiguousarray(y[:, s])) for s in range(P)])
    assert np.array_equal(host(B["out"])[:P], want)
    first = {k: host(v).copy() for k, v in B.items()}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for v in list(B.values()) + ([scratch] if need else []):
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(B["out"])[:P], want)
    for k, v in B.items():
        assert np.array_equal(host(v), first[k]), k
    assert inputs["xs"].any()


# ---- the wrapper and the mirror ----------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_the_header_refuses(env):
    scl, hm, ip, port = env
    z = lambda *shape: torch.zeros(*shape, 1, dtype=torch.int64, device="cuda")
    x = z(4, 3, 8)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.Z2K(64), x, x)
    assert ei.value.status == scl.ERR_BAD_ARG and "unknown field tag" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, x[:0], x[:0])
    assert ei.value.status == scl.ERR_BAD_ARG and "terms" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, x, x, out=x[0])
    assert ei.value.status == scl.ERR_BAD_ARG and "d_dev overlaps x_dev" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, x, x, z(3, 8), out=x[3])
    assert ei.value.status == scl.ERR_BAD_ARG and "overlaps" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, x, z(4, 3, 9)[:, :, :8])                      # y at another row pitch
    assert ei.value.status == scl.ERR_BAD_ARG and "op_stride" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, x, z(4, 3, 7))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, x, x, z(2, 8))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    # a row stride below N is refused, never rounded up: operands of one row expanded over three (row stride 0), an output
    # expanded the same way, and an output whose rows lie N - 1 elements apart
    one = z(4, 1, 8)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, one.expand(4, 3, 8, 1), one.expand(4, 3, 8, 1))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH and "op_stride < N" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, one.expand(4, 3, 8, 1), one.expand(4, 3, 8, 1), z(1, 8).expand(3, 8, 1))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH and "op_stride < N" in str(ei.value)
    narrow = z(64)
    for bad in (z(1, 8).expand(3, 8, 1), torch.as_strided(narrow, (3, 8, 1), (7, 1, 1))):
        with pytest.raises(scl.SclError) as ei:
            ip.dot_mask(O.M61, x, x, out=bad)
        assert ei.value.status == scl.ERR_SIZE_MISMATCH and "d_stride < N" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.dot_mask(O.M61, torch.as_strided(narrow, (2, 3, 8, 1), (21, 7, 1, 1)), torch.as_strided(narrow, (2, 3, 8, 1), (21, 7, 1, 1)))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH and "op_stride < N" in str(ei.value)
    assert not one.any() and not narrow.any()
    assert ip.dot_mask(O.M61, torch.as_strided(narrow, (4, 1, 8, 1), (8, 3, 1, 1)), one).shape == (1, 8, 1)   # one row: no row stride to judge
    assert ip.dot_mask(O.M61, x[:1].expand(4, 3, 8, 1), x).shape == (3, 8, 1)                       # a term stride of 0 is in order
    X, Y = z(2, 2, 3, 8), z(2, 3, 2, 8)
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.M61, X, z(2, 1, 1, 8).expand(2, 3, 2, 8, 1))     # every entry of Y the same row: an entry stride of 0
    assert ei.value.status == scl.ERR_SIZE_MISMATCH and "y_stride < N" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.M61, X, Y, out=z(1, 2, 2, 8).expand(2, 2, 2, 8, 1))    # both batches of the output on one matrix
    assert ei.value.status == scl.ERR_BAD_ARG and "d_batch_stride" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.M61, X, z(2, 4, 2, 8))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.M61, X, Y, out=Y.reshape(2, 2, 3, 8, 1)[:, :, :2])
    assert ei.value.status == scl.ERR_BAD_ARG and ("row-major" in str(ei.value) or "overlaps" in str(ei.value))
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.M61, X, Y, out=X[:, :, :2])
    assert ei.value.status == scl.ERR_BAD_ARG
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.M61, X.transpose(1, 2), Y)                      # not row-major
    assert ei.value.status in (scl.ERR_BAD_ARG, scl.ERR_SIZE_MISMATCH)
    with pytest.raises(scl.SclError) as ei:
        ip.matmul_mask(O.Z2K(64), X, Y)
    assert ei.value.status == scl.ERR_BAD_ARG
    assert not x.any() and not X.any() and not Y.any()
    assert ip.dot_mask(O.M61, x[:, :, :0], x[:, :, :0]).shape == (3, 0, 1)             # N == 0: nothing to do


def test_cxx_round_trips(env):
    """tests/cxx/test_ip_api.cc --gpu, a fresh child process: hip::dotMask and hip::matmulMask equal the per-element form of
    detail/ip.hpp on the host, and share -> dotMask -> hip::mulFinish -> recover is the inner product"""
    r = subprocess.run([mirror_binary("ip"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
