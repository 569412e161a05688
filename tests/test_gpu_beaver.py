"""Beaver multiplication on the GPU (scl_amd.mpc over libscl_hip_mpc.so): the fused mask and finish kernels.

Parity: both calls word for word against the same values composed from the oracle's element-wise calls (O.Port().ew) on identical
PRG-seeded inputs, at the smallest shapes where the pack / tail / per-row logic can go wrong -- N one either side of a wavefront
and of a block's pairs, one pair and no tail (2), 256 pairs and the tail in lane 0 of the next block (513), an odd N behind the
two-per-lane body, more than one block; one row and three; dense rows and a pitch of N + 5 (odd for even N: the one-per-lane
form of the one-limb fields); for the one-limb fields also a base 8 bytes past a 16-byte boundary.  Extremes: operands from extremes.pool against extremes.Model's integer arithmetic, a second and independent statement
of the result.  Aliasing, the protocol end to end between existing entry points (Shamir and additive, all parties at once and
party by party), capture into one graph, and the C++ mirror's round trips.

One oracle reference per field at the largest shape; every shape takes a prefix of it."""
import itertools
import subprocess

import numpy as np
import pytest
import torch

import extremes as X
import oracle_lib as O
from cxx_support import mirror_binary
from gpu_support import BEAVER_N, BEAVER_ROWS, fname, gpu_env, host, rnd
from gpu_support import beaver_reference as reference

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
TAGS = FIELDS + [O.Z2K(K) for K in X.RING_BITS]
PRIME_FIELDS = [O.M61, O.M127, O.MONT128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 63, 64, 65, 255, 257, 513, 4099]
ROWS = [1, 3]
NMAX, RMAX = max(NS), max(ROWS)
assert (RMAX, NMAX) == (BEAVER_ROWS, BEAVER_N)          # the shape of the shared reference (tests/gpu_support.py)


@pytest.fixture(scope="module")
def env():
    return gpu_env("mpc")


def place(arr, stride, phase_words=0, fill=True):
    """a device view [rows][N][L] whose rows lie `stride` elements apart, the first `phase_words` 64-bit words into a fresh
    allocation (torch aligns those to 256 bytes and more)"""
    rows, N, L = arr.shape
    buf = torch.zeros(rows * stride * L + 2, dtype=torch.int64, device="cuda")
    v = torch.as_strided(buf, (rows, N, L), (stride * L, L, 1), phase_words)
    if fill:
        v.copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda())
    return v


def layouts(f, N):
    out = [(N, 0), (N + 5, 0)]
    if O.LIMBS[f] == 1:
        out += [(N, 1), (N + 5, 1)]       # 8 bytes past a 16-byte boundary
    return out


@pytest.mark.parametrize("f", TAGS, ids=fname)
def test_mask_matches_the_oracle(env, f):
    scl, mpc, port = env
    r = reference(port, f)
    for N in NS:
        for rows in ROWS:
            for stride, ph in layouts(f, N):
                note = f"{fname(f)} N={N} rows={rows} stride={stride} phase={8 * ph}"
                ops = [place(r[k][:rows, :N], stride, ph) for k in ("x", "y", "a", "b")]
                out = place(np.zeros((2 * rows, N, O.LIMBS[f]), dtype=np.uint64), stride, ph, fill=False)
                e_rows, d_rows = mpc.beaver_mask(f, *ops, out=out)
                assert np.array_equal(host(e_rows), r["mask_e"][:rows, :N]), note
                assert np.array_equal(host(d_rows), r["mask_d"][:rows, :N]), note
                for k, t in zip(("x", "y", "a", "b"), ops):
                    assert np.array_equal(host(t), r[k][:rows, :N]), note + ": an operand changed"
    # the vector form: one row, (e, d) the two rows of one tensor -- the reference's packet
    e1, d1 = mpc.beaver_mask(f, *[scl.to_device(r[k][0, :65]) for k in ("x", "y", "a", "b")])
    assert e1.shape == d1.shape == (65, O.LIMBS[f]) and e1.data_ptr() + 65 * 8 * O.LIMBS[f] == d1.data_ptr()
    assert np.array_equal(host(e1), r["mask_e"][0, :65]) and np.array_equal(host(d1), r["mask_d"][0, :65])


@pytest.mark.parametrize("f", TAGS, ids=fname)
def test_finish_matches_the_oracle(env, f):
    scl, mpc, port = env
    r = reference(port, f)
    for N in NS:
        for rows in ROWS:
            for stride, ph in layouts(f, N):
                a, b, c = [place(r[k][:rows, :N], stride, ph) for k in ("a", "b", "c")]
                e, d = [place(r[k][None, :N], N, ph)[0] for k in ("e", "d")]
                for ed_rows in sorted({0, 1, rows}):
                    note = f"{fname(f)} N={N} rows={rows} stride={stride} phase={8 * ph} ed_rows={ed_rows}"
                    out = place(np.zeros((rows, N, O.LIMBS[f]), dtype=np.uint64), stride, ph, fill=False)
                    z = mpc.beaver_finish(f, e, d, a, b, c, ed_rows, out=out)
                    want = np.concatenate([r["z1"][:ed_rows, :N], r["z0"][ed_rows:rows, :N]])
                    assert np.array_equal(host(z), want), note
    z1 = mpc.beaver_finish(f, *[scl.to_device(r[k][:65]) for k in ("e", "d")], *[scl.to_device(r[k][0, :65]) for k in ("a", "b", "c")], 1)
    assert z1.shape == (65, O.LIMBS[f]) and np.array_equal(host(z1), r["z1"][0, :65])


def extreme_tuples(f):
    """(e, d, a, b, c) over the pool.  The full cross of the five positions where it has at most 4096 tuples (the rings).  The
    longer pools (31 words for Mersenne127: 2.9 10^7 tuples, each through the big-integer model) get two things: the FULL cross
    of the five positions over six of their words -- 0, 1, p - 1, p - 2, (p - 1) / 2, (p + 1) / 2 (GF(2^128): 0, 1, all ones,
    all ones but the lowest, all ones but the highest, the top bit alone): 7776 tuples, which hold all five operands at
    p - 1, at 0 and at 1, and b + d wrapping to 0, to p - 1 and to p - 2 --, and every ordered pair of the WHOLE pool in each
    of the position pairs that meet in a product or in b + d -- (e, b), (d, a), (b, d), (e, d) -- three times, with the other
    three positions walking the pool at strides of their own."""
    pool = X.pool(f)
    P = len(pool)
    if P ** 5 <= 4096:
        return list(itertools.product(pool, repeat=5))
    if f == O.GF2_128:
        six = [0, 1, X.GF_MASK, X.GF_MASK ^ 1, X.GF_MASK >> 1, 1 << 127]
    else:
        p = X.Model(f).p
        six = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2]
    out = list(itertools.product(six, repeat=5))
    for i in range(P):
        for j in range(P):
            for s in range(3):
                u, v = pool[i], pool[j]
                w = [pool[(i + 2 * j + s) % P], pool[(2 * i + j + 3 * s + 1) % P], pool[(i + j + 5 * s + 2) % P]]
                out.append((u, w[0], w[1], v, w[2]))      # (e, b) = (u, v)
                out.append((w[0], u, v, w[1], w[2]))      # (d, a) = (u, v)
                out.append((w[0], v, w[1], u, w[2]))      # (b, d) = (u, v)
                out.append((u, v, w[0], w[1], w[2]))      # (e, d) = (u, v)
    return out


@pytest.mark.parametrize("f", TAGS, ids=fname)
def test_extreme_operands_match_the_integer_model(env, f):
    """both kernels at the operands that reach the accumulators' bounds (p - 1, all-ones limbs, pairs summing to p), checked by
    big-integer arithmetic; two rows with ed_rows = 1, so both forms of the finish run in one call"""
    scl, mpc, port = env
    m = X.Model(f)
    tup = extreme_tuples(f)
    n = len(tup)
    col = lambda k: m.arr([t[k] for t in tup])
    e, d, a, b, c = [col(k) for k in range(5)]
    two = lambda v: scl.to_device(np.stack([v, v]))
    z = host(mpc.beaver_finish(f, scl.to_device(e), scl.to_device(d), two(a), two(b), two(c), 1))
    base = [m.add(m.add(m.mul(te, tb), m.mul(td, ta)), tc) for te, td, ta, tb, tc in tup]
    with_ed = [m.add(zb, m.mul(te, td)) for zb, (te, td, _, _, _) in zip(base, tup)]
    assert m.ints(z[0]) == with_ed, f"{fname(f)}: finish with e d, {n} extreme tuples"
    assert m.ints(z[1]) == base, f"{fname(f)}: finish without e d, {n} extreme tuples"
    er, dr = mpc.beaver_mask(f, scl.to_device(e), scl.to_device(b), scl.to_device(d), scl.to_device(a))   # e - d and b - a
    assert m.ints(host(er)) == [m.sub(t[0], t[1]) for t in tup] and m.ints(host(dr)) == [m.sub(t[3], t[2]) for t in tup]


@pytest.mark.parametrize("f", TAGS, ids=fname)
def test_finish_in_place(env, f):
    """z is a, z is b, z is c: each equal to the out-of-place result (a lane reads its elements of a row before it writes them)"""
    scl, mpc, port = env
    r = reference(port, f)
    for N, rows, stride in ((255, 3, 260), (4099, 3, 4099), (65, 1, 65)):
        e, d = [scl.to_device(r[k][:N]) for k in ("e", "d")]
        want = np.concatenate([r["z1"][:1, :N], r["z0"][1:rows, :N]])
        for target in range(3):
            ops = [place(r[k][:rows, :N], stride) for k in ("a", "b", "c")]
            z = mpc.beaver_finish(f, e, d, *ops, 1, out=ops[target])
            assert z.data_ptr() == ops[target].data_ptr()
            assert np.array_equal(host(z), want), f"{fname(f)} N={N} rows={rows} z is {'abc'[target]}"
            for k in range(3):
                if k != target:
                    assert np.array_equal(host(ops[k]), r["abc"[k]][:rows, :N])


@pytest.mark.parametrize("f", PRIME_FIELDS, ids=fname)
def test_shamir_multiplication_end_to_end(env, f):
    """(n, t) = (5, 2), 257 secrets: share x, y and a triple, mask all parties at once, open e and d with shamir_recover, finish
    with ed_rows = n (a constant is its own sharing), recover z: x y element-wise.  Then party by party (rows = 1, ed_rows = 1):
    the same rows."""
    scl, mpc, port = env
    n, t, N = 5, 2, 257
    sec = {k: rnd(port, f, N, b"sh-" + k.encode()) for k in ("x", "y", "a", "b")}
    sec["c"] = port.ew(f, O.MUL, sec["a"], sec["b"])
    sh = {k: scl.shamir_share_prg(f, scl.to_device(v), t, n, b"beaver-share-" + k.encode()) for k, v in sec.items()}
    e_rows, d_rows = mpc.beaver_mask(f, sh["x"], sh["y"], sh["a"], sh["b"])
    e, d = scl.shamir_recover(f, e_rows), scl.shamir_recover(f, d_rows)
    assert np.array_equal(host(e), port.ew(f, O.SUB, sec["x"], sec["a"]))
    assert np.array_equal(host(d), port.ew(f, O.SUB, sec["y"], sec["b"]))
    z = mpc.beaver_finish(f, e, d, sh["a"], sh["b"], sh["c"], n)
    assert np.array_equal(host(scl.shamir_recover(f, z)), port.ew(f, O.MUL, sec["x"], sec["y"]))
    for i in range(n):
        zi = mpc.beaver_finish(f, e, d, sh["a"][i], sh["b"][i], sh["c"][i], 1)
        assert np.array_equal(host(zi), host(z[i])), f"party {i}"


@pytest.mark.parametrize("f", [O.GF2_128, O.Z2K(64), O.Z2K(128)], ids=fname)
def test_additive_multiplication_end_to_end(env, f):
    """n = 3 additive shares: only party 0 adds e d (ed_rows = 1 with row 0 party 0); additive_recover(z) == x y.  Party by
    party (rows = 1; ed_rows 1 for party 0, 0 otherwise): the same rows."""
    scl, mpc, port = env
    n, N = 3, 257
    sec = {k: rnd(port, f, N, b"ad-" + k.encode()) for k in ("x", "y", "a", "b")}
    sec["c"] = port.ew(f, O.MUL, sec["a"], sec["b"])
    sh = {k: scl.additive_share_prg(f, scl.to_device(v), n, b"beaver-add-" + k.encode()) for k, v in sec.items()}
    e_rows, d_rows = mpc.beaver_mask(f, sh["x"], sh["y"], sh["a"], sh["b"])
    e, d = scl.additive_recover(f, e_rows), scl.additive_recover(f, d_rows)
    assert np.array_equal(host(e), port.ew(f, O.SUB, sec["x"], sec["a"]))
    z = mpc.beaver_finish(f, e, d, sh["a"], sh["b"], sh["c"], 1)
    assert np.array_equal(host(scl.additive_recover(f, z)), port.ew(f, O.MUL, sec["x"], sec["y"]))
    for i in range(n):
        zi = mpc.beaver_finish(f, e, d, sh["a"][i], sh["b"][i], sh["c"][i], 1 if i == 0 else 0)
        assert np.array_equal(host(zi), host(z[i])), f"party {i}"


@pytest.mark.parametrize("f", [O.M61, O.MONT128, O.SECP256K1_SCALAR], ids=fname)
def test_mask_then_finish_captured_into_one_graph(env, f):
    """mask, then finish on the mask's own output (one party: its e and d are the opened values), captured as a linear chain and
    replayed twice with the inputs rewritten in between: z = x y each time"""
    scl, mpc, port = env
    N, L = 1000, O.LIMBS[f]

    def inputs(tag):
        s = {k: rnd(port, f, N, tag + k.encode()) for k in ("x", "y", "a", "b")}
        s["c"] = port.ew(f, O.MUL, s["a"], s["b"])
        return s
    first = inputs(b"g0-")
    buf = {k: scl.to_device(v) for k, v in first.items()}
    de = torch.empty(2, N, L, dtype=torch.int64, device="cuda")
    z = torch.empty(N, L, dtype=torch.int64, device="cuda")

    def chain():
        e, d = mpc.beaver_mask(f, buf["x"], buf["y"], buf["a"], buf["b"], out=de)
        mpc.beaver_finish(f, e, d, buf["a"], buf["b"], buf["c"], 1, out=z)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                   # every kernel has run once before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert np.array_equal(host(z), port.ew(f, O.MUL, first["x"], first["y"]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for tag in (b"g1-", b"g2-"):
        s = inputs(tag)
        for k, v in s.items():
            buf[k].copy_(scl.to_device(v))
        z.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(z), port.ew(f, O.MUL, s["x"], s["y"])), tag


def test_wrapper_refuses_what_the_header_refuses(env):
    scl, mpc, port = env
    r = reference(port, O.M61)
    a = scl.to_device(r["a"][:3, :64])
    e = scl.to_device(r["e"][:64])
    with pytest.raises(scl.SclError) as ei:
        mpc.beaver_finish(O.M61, e, e, a, a, a, 4)
    assert ei.value.status == scl.ERR_BAD_ARG
    with pytest.raises(scl.SclError) as ei:
        mpc.beaver_mask(O.M61, a, a, a, a[:, :63])
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        mpc.beaver_finish(O.M61, e, e, a, a, a, 1, out=e.new_empty(3, 63, 1))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    a1 = scl.to_device(r["a"][0, :64])
    with pytest.raises(scl.SclError) as ei:
        mpc.beaver_finish(O.M61, e, e, a1, a1, a1, 1, out=e)          # z is e: the library's own refusal of the overlap
    assert ei.value.status == scl.ERR_BAD_ARG and "overlaps" in str(ei.value)


def test_cxx_round_trips(env):
    """tests/cxx/test_beaver_api.cc: hip::beaverMask / beaverFinish over Secp256k1Scalar and Mersenne61 (Shamir) and the
    reference's two-party additive shape (party 0 adds e d)"""
    r = subprocess.run(["timeout", "-k", "10", "120", mirror_binary("beaver")], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
