"""Honest-majority multiplication on the GPU (scl_amd.hm over libscl_hip_hm.so) against the Python model of tests/port_models.py,
which tests/test_hm_host.py pins to what the reference produced: device output equals the model byte for byte.  Each test's docstring names
its shapes.  One model run per (field, shape) at the largest N; every smaller N is a prefix of it."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
from cxx_support import mirror_binary
from gpu_support import HM_N, deal_all, fname, gpu_env, host, pm1, pool, rnd
from gpu_support import HM_SEED as SEED
from gpu_support import hm_chain_buffers as chain_buffers
from gpu_support import hm_reference as reference
from port_models import TAGS, double_blocks, golden, model_apply, model_double, model_finish, model_him, model_inputs, model_mask, model_open
from port_models import hm_protocol_entry as protocol_entry

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
FUSED_FIELDS = [O.M61, O.M127, O.GF2_128]
NS = [1, 2, 3, 64, 257, 1025]
NMAX = max(NS)
assert NMAX == HM_N          # the shape of the shared reference (tests/gpu_support.py)
DOUBLE_NT = [(3, 1), (4, 1), (7, 3), (10, 3), (9, 4)]
APPLY_MN = [(1, 1), (3, 4), (7, 10), (17, 20), (40, 41), (5, 16), (5, 17), (43, 12), (90, 12)]
APPLY_NS = [1, 3, 64, 257, 1025]
PAIR_NS = [2, 513]           # Mersenne61's pair loop: one pair and no tail; 256 pairs fill block 0 and the tail is lane 0 of block 1


def ns(f, base):
    """the shapes of a streaming kernel: the one-limb field also at PAIR_NS"""
    return sorted(set(base) | set(PAIR_NS)) if O.LIMBS[f] == 1 else base


@pytest.fixture(scope="module")
def env():
    return gpu_env("hm")


def same(got, want, N, note):
    for g, w, k in zip(got, want, ("lo", "hi")):
        assert np.array_equal(host(g), w[:, :N]), f"{note}: {k}"


def expect_scratch(hm, f, N, n, t, flags=0):
    need = hm.double_scratch_bytes(f, N, n, t, flags)
    fused = f in FUSED_FIELDS and t <= 3 and not flags
    assert need == (0 if fused else (1 + 3 * t) * N * 8 * O.LIMBS[f]), (fname(f), N, n, t, flags)
    return fused


# ---- double sharings -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_double_sharings_equal_the_model(env, f):
    """fused where the header says so, two passes elsewhere; the two paths deal the same sharings; both degrees hide the same r"""
    scl, hm, port = env
    for n, t in DOUBLE_NT:
        want = reference(port, f, n, t)
        for N in NS:
            fused = expect_scratch(hm, f, N, n, t)
            same(hm.double_share(f, N, t, n, SEED), want, N, f"{fname(f)} ({n},{t}) N={N} {'fused' if fused else 'two-pass'}")
            if fused:
                expect_scratch(hm, f, N, n, t, hm.TWO_PASS)
                same(hm.double_share(f, N, t, n, SEED, flags=hm.TWO_PASS), want, N, f"{fname(f)} ({n},{t}) N={N} forced two-pass")
        lo, hi = hm.double_share(f, 64, t, n, SEED)
        assert np.array_equal(host(scl.shamir_recover(f, lo[:t + 1])), want[2][:64])
        assert np.array_equal(host(scl.shamir_recover(f, hi[:2 * t + 1])), want[2][:64])


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_largest_threshold_the_dealer_takes(env, f):
    """2t = 48 (16 for the 32-byte fields): the last degree at which the engine's share call stays asynchronous; one past it is
    refused, and so is n = 2t"""
    scl, hm, port = env
    n, t = (18, 8) if O.LIMBS[f] == 4 else (50, 24)
    N = 67
    same(hm.double_share(f, N, t, n, SEED), reference(port, f, n, t, N=N), N, f"{fname(f)} ({n},{t})")
    with pytest.raises(scl.SclError) as ei:
        hm.double_share(f, N, t + 1, n + 2, SEED)
    assert ei.value.status == scl.ERR_BAD_ARG and "degree" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        hm.double_share(f, N, t, 2 * t, SEED)
    assert ei.value.status == scl.ERR_BAD_ARG and "2t" in str(ei.value)


@pytest.mark.parametrize("f", FUSED_FIELDS, ids=fname)
def test_every_fused_threshold(env, f):
    """t = 0 .. 3 each have a kernel of their own: n = 8, N = 67, fused and forced through two passes"""
    scl, hm, port = env
    for t in range(4):
        assert expect_scratch(hm, f, 67, 8, t)
        want = reference(port, f, 8, t, N=67)
        same(hm.double_share(f, 67, t, 8, SEED), want, 67, f"{fname(f)} (8,{t}) fused")
        same(hm.double_share(f, 67, t, 8, SEED, flags=hm.TWO_PASS), want, 67, f"{fname(f)} (8,{t}) two-pass")
    assert not expect_scratch(hm, f, 67, 9, 4)


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_a_launch_across_a_multiple_of_2_to_the_32_blocks(env, f):
    """counter0 = 2^32 - 5, N = 3: the first double sharing starts below the boundary, the last ends above it"""
    scl, hm, port = env
    c0, N = 2 ** 32 - 5, 3
    for n, t in ((10, 3), (9, 4)):
        assert c0 + N * double_blocks(f, t) > 2 ** 32 > c0
        same(hm.double_share(f, N, t, n, SEED, counter0=c0), reference(port, f, n, t, c0, N), N, f"{fname(f)} ({n},{t}) straddle")


@pytest.mark.parametrize("f", [O.M61, O.GF2_128, O.SECP256K1_SCALAR], ids=fname)
def test_a_shard_equals_its_slice_of_the_long_run(env, f):
    """double sharings [first, first + k) dealt with counter0 = first * B"""
    scl, hm, port = env
    first, k = 100, 57
    for n, t in ((10, 3), (9, 4)):
        want = [m[:, first:first + k] for m in reference(port, f, n, t)[:2]]
        assert hm.double_blocks(f, n, t) == double_blocks(f, t)
        same(hm.double_share(f, k, t, n, SEED, counter0=first * hm.double_blocks(f, n, t)), want, k, f"{fname(f)} ({n},{t}) shard")


def test_mersenne61_on_an_odd_stride_and_an_odd_base(env):
    """an odd stride, a base 8 bytes past a 16-byte boundary: the same sharings, and the gaps between rows stay unwritten"""
    scl, hm, port = env
    f = O.M61
    for N in (2, 3, 64, 257):
        for stride, phase in ((N + (N % 2) + 1, 0), (N + (N % 2), 1), (N + (N % 2) + 1, 1), (N + (N % 2) + 2, 0)):
            for n, t in ((10, 3), (9, 4)):
                buf = torch.zeros(2 * n * stride + 2, dtype=torch.int64, device="cuda")
                out = [torch.as_strided(buf, (n, N, 1), (stride, 1, 1), phase + m * n * stride) for m in range(2)]
                hm.double_share(f, N, t, n, SEED, out=out)
                same(out, reference(port, f, n, t), N, f"m61 N={N} stride={stride} phase={8 * phase} ({n},{t})")
                gaps = torch.ones(2 * n * stride + 2, dtype=torch.bool)
                for m in range(2):
                    for i in range(n):
                        lo = phase + (m * n + i) * stride
                        gaps[lo:lo + N] = False
                assert not buf.cpu()[gaps].any(), f"m61 N={N} stride={stride} phase={8 * phase} ({n},{t}): a row gap was written"


# ---- apply -------------------------------------------------------------------------------------------------------------------
def matmul_raw(scl, f, out, ldc, A, lda, B, ldb, M, K, N):
    rc = scl.lib.scl_hip_matmul(f, C.c_void_p(out.data_ptr()), C.c_size_t(ldc), C.c_void_p(A.data_ptr()), C.c_size_t(lda),
                                C.c_void_p(B.data_ptr()), C.c_size_t(ldb), C.c_size_t(M), C.c_size_t(K), C.c_size_t(N), scl._stream())
    assert rc == 0, scl.lib.scl_hip_last_error()


def pitches(f, N):
    """row pitches larger than N: Mersenne61 an even one (two columns per lane) and an odd one, wider fields one"""
    return [N + 2 + (N % 2), N + 3 + (N % 2)] if O.LIMBS[f] == 1 else [N + 3]


def run_apply(env, f, m, n, N, batch, pitch, M, x_all, note):
    """batch == 1: in [n][pitch]; batch == n: the dealers' layout [dealer][party][pitch] read with in_stride = batch * pitch and
    in_batch_stride = pitch, out laid out the same way -- so ONE matmul over the whole width is the same product"""
    scl, hm, port = env
    L, ldm = O.LIMBS[f], n + 3
    width = (batch - 1) * pitch + N
    x = np.zeros((n, batch * pitch, L), dtype=np.uint64)
    for b in range(batch):
        x[:, b * pitch:b * pitch + N] = x_all[:n * N].reshape(n, N, L) if batch == 1 else np.roll(x_all, 7 * b, axis=0)[:n * N].reshape(n, N, L)
    xd = scl.to_device(x)
    Md = torch.zeros(m, ldm, L, dtype=torch.int64, device="cuda")
    Md[:, :n] = scl.to_device(M)
    out = torch.zeros(m, batch * pitch, L, dtype=torch.int64, device="cuda")
    x4 = torch.as_strided(xd, (batch, n, N, L), (pitch * L, batch * pitch * L, L, 1))
    o4 = torch.as_strided(out, (batch, m, N, L), (pitch * L, batch * pitch * L, L, 1))
    got = hm.apply_matrix(f, Md[:, :n], x4 if batch > 1 else x4[0], out=o4 if batch > 1 else o4[0])
    assert got.data_ptr() == out.data_ptr()
    ref = torch.zeros_like(out)
    matmul_raw(scl, f, ref, batch * pitch, Md, ldm, xd, batch * pitch, m, n, width)
    mask = np.zeros(batch * pitch, dtype=bool)
    for b in range(batch):
        mask[b * pitch:b * pitch + N] = True
    g, r = host(out), host(ref)
    assert np.array_equal(g[:, mask], r[:, mask]), f"{note}: differs from scl_hip_matmul"
    assert not g[:, ~mask].any(), f"{note}: a gap was written"
    cols = np.flatnonzero(mask)          # the model on the head of the first batch and the tail of the last: at most 300 columns,
    half = max(4, min(150, 1500 // (m * n)))      # fewer for the large matrices (the oracle's products are the cost of this test)
    if len(cols) > 2 * half:
        cols = np.concatenate([cols[:half], cols[-half:]])
    assert np.array_equal(g[:, cols], model_apply(port, f, M, np.ascontiguousarray(x[:, cols]))), f"{note}: differs from the model"


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_apply_equals_matmul_and_the_model(env, f):
    scl, hm, port = env
    x_all = pool(port, f, 41 * NMAX + 300, b"apply-x")
    for m, n in APPLY_MN:
        # the hyper-invertible matrix where it is small, uniform entries elsewhere (the oracle's Lagrange bases over GF(2^128) take seconds)
        M = model_him(port, f, m, n) if m * n <= 100 else pool(port, f, m * n, b"apply-m").reshape(m, n, -1).copy()
        for N in ns(f, APPLY_NS):
            for pitch in pitches(f, N):
                for batch in (1, n):
                    if batch > 1 and N == NMAX and n > 10:
                        continue       # (the widest shapes at batch = n are a copy of the batch = 1 case 41 times over)
                    run_apply(env, f, m, n, N, batch, pitch, M, x_all, f"{fname(f)} apply ({m},{n}) N={N} batch={batch} pitch={pitch}")


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_apply_at_the_worst_case(env, f):
    """every entry of M and every input p - 1 (GF(2^128): all ones) at n = 64, 65 and 300 terms -- past the LDS tile of M, past
    Mersenne127's bound of 256 prepared products per accumulator -- and at 1100, past Mersenne61's of 1024; m = 9 (two or three
    groups of rows), N = 3"""
    scl, hm, port = env
    top, N, m = pm1(port, f), 3, 9
    for n in (64, 65, 300, 1100):
        M = np.repeat(np.repeat(top[None, None], m, axis=0), n, axis=1)
        x = np.repeat(np.repeat(top[None, None], n, axis=0), N, axis=1)
        got = host(hm.apply_matrix(f, scl.to_device(M), scl.to_device(x)))
        assert np.array_equal(got, model_apply(port, f, M, x)), f"{fname(f)} n={n}"
        assert np.array_equal(got, host(scl.matmul(f, scl.to_device(M), scl.to_device(x)))), f"{fname(f)} n={n} vs matmul"


# ---- mask and finish ---------------------------------------------------------------------------------------------------------
def strided(scl, a, pitch, phase=0):
    """[rows][N][L] host array -> a device view with row pitch `pitch` (elements), `phase` elements into its buffer"""
    rows, N, L = a.shape
    buf = torch.zeros((rows * pitch + phase + 2) * L, dtype=torch.int64, device="cuda")
    v = torch.as_strided(buf, (rows, N, L), (pitch * L, L, 1), phase * L)
    v.copy_(scl.to_device(a))
    return v


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_mask_equals_the_model(env, f):
    scl, hm, port = env
    n = 10
    ops = [pool(port, f, n * NMAX, tag).reshape(n, NMAX, -1) for tag in (b"mask-x", b"mask-y", b"mask-r")]
    top = pm1(port, f)
    for rows in (1, n):
        for N in ns(f, NS):
            x, y, r2 = [np.ascontiguousarray(o[:rows, :N]) for o in ops]
            want = model_mask(port, f, x, y, r2)
            for pitch in pitches(f, N) + [N]:
                for phase in ((0, 1) if O.LIMBS[f] == 1 else (0,)):
                    xd, yd, rd = [strided(scl, a, pitch, phase) for a in (x, y, r2)]
                    note = f"{fname(f)} mask rows={rows} N={N} pitch={pitch} phase={phase}"
                    assert np.array_equal(host(hm.mul_mask(f, xd, yd, rd)), want), note
                    assert np.array_equal(host(rd), r2), note + ": r2 changed"
                    hm.mul_mask(f, xd, yd, rd, out=rd)                                # in place
                    assert np.array_equal(host(rd), want), note + " in place"
        t3 = np.repeat(np.repeat(top[None, None], rows, axis=0), 67, axis=1)
        assert np.array_equal(host(hm.mul_mask(f, *[scl.to_device(t3)] * 3)), model_mask(port, f, t3, t3, t3)), f"{fname(f)} mask at p - 1"
    assert np.array_equal(host(hm.mul_mask(f, *[scl.to_device(o[0, :5]) for o in ops])), model_mask(port, f, *[o[:1, :5] for o in ops])[0])


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_finish_equals_the_model(env, f):
    scl, hm, port = env
    n = 10
    dsh_all = pool(port, f, 64 * NMAX, b"finish-d").reshape(64, NMAX, -1)
    r_all = pool(port, f, n * NMAX, b"finish-r").reshape(n, NMAX, -1)
    one = port.from_int(f, 1)[None]
    for m in (1, 3, 10, 64):
        lam = one if m == 1 else scl.lagrange_basis(f, m)
        for rows in (1, n):
            for N in ns(f, NS):
                dsh, r = np.ascontiguousarray(dsh_all[:m, :N]), np.ascontiguousarray(r_all[:rows, :N])
                want = model_finish(port, f, model_open(port, f, dsh, lam), r)
                for pitch in (pitches(f, N) + [N])[:: (1 if N in (3, 257) else 2)]:
                    for phase in ((0, 1) if O.LIMBS[f] == 1 else (0,)):
                        dd, rd = strided(scl, dsh, pitch, phase), strided(scl, r, pitch, phase)
                        note = f"{fname(f)} finish m={m} rows={rows} N={N} pitch={pitch} phase={phase}"
                        assert np.array_equal(host(hm.mul_finish(f, dd, rd, lam=lam)), want), note
                        hm.mul_finish(f, dd, rd, lam=lam, out=rd)                     # in place
                        assert np.array_equal(host(rd), want), note + " in place"
    top = pm1(port, f)                                                                 # every operand p - 1 at m = 64
    dsh, r, lam = [np.repeat(np.repeat(top[None, None], k, axis=0), 67, axis=1) for k in (64, n)] + [np.repeat(top[None], 64, axis=0)]
    got = hm.mul_finish(f, scl.to_device(dsh), scl.to_device(r), lam=lam)
    assert np.array_equal(host(got), model_finish(port, f, model_open(port, f, dsh, lam), r)), f"{fname(f)} finish at p - 1"
    # an opened d: m = 1, lambda = one
    d = np.ascontiguousarray(dsh_all[0, :67])
    assert np.array_equal(host(hm.mul_finish(f, scl.to_device(d), scl.to_device(r_all[:, :67].copy()))), model_finish(port, f, d, r_all[:, :67]))
    with pytest.raises(scl.SclError) as ei:
        hm.mul_finish(f, scl.to_device(np.ascontiguousarray(dsh_all[:, :8]).repeat(2, axis=0)[:65]), scl.to_device(r_all[:, :8].copy()),
                      lam=np.repeat(one, 65, axis=0))
    assert ei.value.status == scl.ERR_BAD_ARG and "1..64" in str(ei.value)


# ---- the protocol ------------------------------------------------------------------------------------------------------------
def test_the_fixtures_protocol_end_to_end_on_the_device(env):
    """n dealers with the fixture's seeds -> the extraction at both degrees, every party in one launch -> mask -> finish ->
    shamir_recover: every intermediate equals what the reference computed"""
    scl, hm, port = env
    for e in golden("hm")["protocol"]:
        f, n, t = TAGS[e["field"]], e["n"], e["t"]
        want, S = protocol_entry(port, f, e)
        L, m = O.LIMBS[f], n - t
        lo, hi = [torch.zeros(n, n, S, L, dtype=torch.int64, device="cuda") for _ in range(2)]
        deal_all(hm, f, S, t, n, [d["seed"].encode() for d in e["dealers"]], lo, hi)
        assert np.array_equal(host(lo), want["lo"]) and np.array_equal(host(hi), want["hi"])
        Md = scl.to_device(hm.hyper_invertible(f, m, n))
        R_lo = hm.apply_matrix(f, Md, lo.transpose(0, 1)).reshape(n, m * S, L)          # [party][k][s] -> product p = S k + s
        R_hi = hm.apply_matrix(f, Md, hi.transpose(0, 1)).reshape(n, m * S, L)
        assert np.array_equal(host(R_lo), want["R_lo"]) and np.array_equal(host(R_hi), want["R_hi"])
        x, y, xs, ys = model_inputs(port, f, b"hm inputs", m * S, t, n)
        assert np.array_equal(x, want["x"]) and np.array_equal(y, want["y"])
        d_shares = hm.mul_mask(f, scl.to_device(xs), scl.to_device(ys), R_hi)
        assert np.array_equal(host(d_shares), want["d_shares"])
        assert np.array_equal(host(scl.shamir_recover(f, d_shares)), want["d"])
        z_shares = hm.mul_finish(f, d_shares, R_lo)
        assert np.array_equal(host(z_shares), want["z_shares"])
        z = host(scl.shamir_recover(f, z_shares))
        assert np.array_equal(z, want["z"]) and np.array_equal(z, port.ew(f, O.MUL, want["x"], want["y"]))


def pitched(t, width):
    """a copy of [rows][P][L] whose rows lie `width` elements apart: the pitch of the extracted rows it is multiplied with"""
    rows, P, L = t.shape
    buf = torch.zeros(rows, width, L, dtype=torch.int64, device=t.device)
    buf[:, :P] = t
    return buf[:, :P]


def run_chain(scl, hm, f, n, t, S, P, seeds, Md, xs, ys, lam, B, scratch=None, flags=0):
    L, m = O.LIMBS[f], n - t
    deal_all(hm, f, S, t, n, seeds, B["lo"], B["hi"], scratch, flags)
    hm.apply_matrix(f, Md, B["lo"].transpose(0, 1), out=B["R_lo"])
    hm.apply_matrix(f, Md, B["hi"].transpose(0, 1), out=B["R_hi"])
    r_lo, r_hi = B["R_lo"].reshape(n, m * S, L)[:, :P], B["R_hi"].reshape(n, m * S, L)[:, :P]
    hm.mul_mask(f, xs, ys, r_hi, out=B["d"][:, :P])
    hm.mul_finish(f, B["d"][:, :P], r_lo, lam=lam, out=B["z"][:, :P])
    scl.shamir_recover(f, B["z"][:, :P], lam=lam, out=B["out"][:P])


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_multiplication_without_a_dealer(env, f):
    """(10,3), 257 products: ten dealers, 37 double sharings each, 7 x 37 = 259 extracted, the first 257 used; against the
    model's x y, and [z] is a degree-t sharing"""
    scl, hm, port = env
    n, t, S, P = 10, 3, 37, 257
    x, y = rnd(port, f, P, b"hm-x"), rnd(port, f, P, b"hm-y")
    xs = pitched(scl.shamir_share_prg(f, scl.to_device(x), t, n, b"hm-xs"), (n - t) * S)
    ys = pitched(scl.shamir_share_prg(f, scl.to_device(y), t, n, b"hm-ys"), (n - t) * S)
    seeds = [b"hm dealer %d" % i for i in range(n)]
    B = chain_buffers(f, n, t, S)
    run_chain(scl, hm, f, n, t, S, P, seeds, scl.to_device(hm.hyper_invertible(f, n - t, n)), xs, ys, scl.lagrange_basis(f, n), B)
    want = port.ew(f, O.MUL, x, y)
    assert np.array_equal(host(B["out"])[:P], want)
    assert np.array_equal(host(scl.shamir_recover(f, B["z"][:t + 1, :P])), want)
    # the extraction against the model, and what it extracts are double sharings
    lo = np.stack([model_double(port, f, s, 0, S, t, n)[0] for s in seeds])
    M = model_him(port, f, n - t, n)
    for j in (0, n - 1):
        assert np.array_equal(host(B["R_lo"][j]), model_apply(port, f, M, np.ascontiguousarray(lo[:, j])))
    assert np.array_equal(host(scl.shamir_recover(f, B["R_lo"].reshape(n, -1, O.LIMBS[f])[:t + 1])),
                          host(scl.shamir_recover(f, B["R_hi"].reshape(n, -1, O.LIMBS[f])[:2 * t + 1])))


@pytest.mark.parametrize("f,flags", [(O.M61, 0), (O.M61, 1), (O.SECP256K1_SCALAR, 0), (O.MONT128, 0)],
                         ids=["m61-fused", "m61-two-pass", "secp_scalar-two-pass", "mont128-two-pass"])
def test_the_chain_captured_into_one_graph(env, f, flags):
    """deal x n -> apply at both degrees -> mask -> finish -> recover on one stream, captured as a linear chain and replayed once
    with every buffer cleared in between.  The two-pass deal's scratch is the caller's and its engine tables exist after the run
    before the capture, as the header asks"""
    scl, hm, port = env
    n, t, S, P = 10, 3, 37, 257
    need = hm.double_scratch_bytes(f, S, n, t, flags)
    assert (need == 0) == (f == O.M61 and not flags)
    scratch = torch.zeros(need // 8, dtype=torch.int64, device="cuda") if need else None
    x, y = rnd(port, f, P, b"graph-x"), rnd(port, f, P, b"graph-y")
    xs = pitched(scl.shamir_share_prg(f, scl.to_device(x), t, n, b"graph-xs"), (n - t) * S)
    ys = pitched(scl.shamir_share_prg(f, scl.to_device(y), t, n, b"graph-ys"), (n - t) * S)
    lam = scl.lagrange_basis(f, n)
    Md = scl.to_device(hm.hyper_invertible(f, n - t, n))
    seeds = [b"graph dealer %d" % i for i in range(n)]
    B = chain_buffers(f, n, t, S)
    chain = lambda: run_chain(scl, hm, f, n, t, S, P, seeds, Md, xs, ys, lam, B, scratch, flags)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                   # every kernel has run once before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = port.ew(f, O.MUL, x, y)
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
    assert np.array_equal(host(B["lo"][3]), model_double(port, f, seeds[3], 0, S, t, n)[0])


def test_wrapper_refuses_what_the_header_refuses(env):
    scl, hm, port = env
    with pytest.raises(scl.SclError) as ei:
        hm.double_share(O.Z2K(64), 8, 1, 4, SEED)
    assert ei.value.status == scl.ERR_BAD_ARG
    with pytest.raises(scl.SclError) as ei:
        hm.double_share(O.M61, 8, 1, 4, SEED, flags=2)
    assert ei.value.status == scl.ERR_BAD_ARG and "flags" in str(ei.value)
    m = torch.zeros(4, 8, 1, dtype=torch.int64, device="cuda")
    with pytest.raises(scl.SclError) as ei:
        hm.double_share(O.M61, 8, 1, 4, SEED, out=(m, m))
    assert ei.value.status == scl.ERR_BAD_ARG and "overlap" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        hm.double_share(O.M61, 8, 4, 9, SEED, scratch=torch.zeros(8, dtype=torch.int64, device="cuda"))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        hm.apply_matrix(O.M61, torch.zeros(3, 5, 1, dtype=torch.int64, device="cuda"), m)
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        hm.apply_matrix(O.M61, torch.zeros(4, 4, 1, dtype=torch.int64, device="cuda"), m, out=m)
    assert ei.value.status == scl.ERR_BAD_ARG and "overlap" in str(ei.value)
    assert not m.any()


def test_cxx_round_trips(env):
    """tests/cxx/test_hm_api.cc --gpu: hip::dealDoubleSharings equals ss::doubleShare on one PRG, and deal, hip::applyMatrix,
    hip::mulMask, hip::mulFinish, recover multiplies"""
    r = subprocess.run([mirror_binary("hm"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
