"""Random shared bits on the device (libscl_hip_rb.so): scl_rb_sqrt and scl_rb_bits_finish against the Python model of
tests/rb_support.py on every element -- all five prime fields, Mont128 at 2^128 - 159 (s = 5) and at 2^127 - 1 (s = 1), the four
flag combinations, planted zeros and non-residues --, the whole pipeline over scl_amd.hm end to end (deal, extract, square, open,
finish; the opened bits are 0 or 1, equal the model's, and both values occur), both calls captured into a graph as the first
calls of a fresh process, and the C++ mirror.  Everything is exact."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle_lib as O
import rb_support as RBS
from gpu_support import MONT_P, deal_all, gpu_env, host, placed

pytestmark = pytest.mark.gpu

# (name, tag, the Mont128 modulus or None)
CASES = [("m61", O.M61, None), ("m127", O.M127, None), ("mont128-s5", O.MONT128, RBS.MONT_P0), ("mont128-s1", O.MONT128, RBS.MONT_P1),
         ("secp_scalar", O.SECP256K1_SCALAR, None), ("secp_field", O.SECP256K1_FIELD, None)]
IDS = [c[0] for c in CASES]
NS = [1, 63, 64, 65, 257, 4099]      # the wave edge, the two-column tail, more than one workgroup
NMAX = max(NS)
_MODEL = {}


@pytest.fixture(scope="module")
def env():
    return gpu_env("rb", "hm")


@pytest.fixture
def modulus(env):
    """sets the Mont128 modulus of a case on this thread, and the tests' own afterwards"""
    scl = env[0]

    def use(mp):
        if mp is not None:
            scl.set_mont128_prime(mp)
        return mp or RBS.MONT_P0
    yield use
    scl.set_mont128_prime(MONT_P)


def inputs(name, p):
    """NMAX seeded integers below p (about half are non-residues) and the model's (value, status) per flags, once per case"""
    if name not in _MODEL:
        a = RBS.seeded(p, NMAX, 2000 + IDS.index(name))
        _MODEL[name] = (a, {fl: [RBS.model_sqrt(p, v, fl) for v in a] for fl in range(4)})
    return _MODEL[name]


@pytest.mark.parametrize("flags", [0, RBS.ODD_ROOT, RBS.INVERSE, RBS.ODD_ROOT | RBS.INVERSE], ids=["even", "odd", "even-inverse", "odd-inverse"])
@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_sqrt_equals_the_model_on_every_element(env, modulus, name, f, mp, flags):
    """N in {1, 63, 64, 65, 257, 4099}; root (or inverse root) and status of every element; the input is left alone; residues and
    non-residues both make up more than a quarter"""
    scl, rb, hm, port = env
    mp = modulus(mp)
    p = RBS.prime(f, mp)
    base, model = inputs(name, p)
    for N in NS:
        a, want = list(base[:N]), list(model[flags][:N])
        for z in {0, N - 1, N // 2}:                               # zeros at both ends and in the middle
            a[z], want[z] = 0, (0, RBS.ZERO)
        dev = scl.to_device(RBS.to_limbs(f, a, mp))
        before = dev.clone()
        out, status = rb.sqrt(f, dev, flags)
        assert RBS.from_limbs(f, host(out), mp) == [v for v, _ in want], (name, N, flags)
        assert status.cpu().tolist() == [s for _, s in want], (name, N, flags)
        assert torch.equal(dev, before)
        counts = np.bincount(status.cpu().numpy(), minlength=3)
        assert N < 64 or (counts[0] > N // 4 and counts[2] > N // 4), counts


def bits_case(env, f, mp, p, rows, N, pitch, tag):
    """u = squares of seeded values with u = 0 and a non-residue planted, r seeded: b and status against the model; nothing but
    the view of b is written"""
    scl, rb, hm, port = env
    roots = RBS.seeded(p, N, 3000 + tag)
    u = [v * v % p for v in roots]
    planted = {}
    if N >= 3:
        z = 2
        while RBS.is_residue(p, z):
            z += 1
        u[N // 2], u[N - 1] = 0, z * u[N - 1] % p                    # a zero; a residue times a non-residue
        planted = {N // 2: RBS.ZERO, N - 1: RBS.NONRESIDUE} if u[N - 1] else {}
    r = [RBS.seeded(p, N, 4000 + tag + i) for i in range(rows)]
    for i in range(min(rows, 2)):                                  # rows that ARE the root: the even one gives 1, the odd one 0
        r[i][0] = RBS.model_sqrt(p, u[0], RBS.ODD_ROOT if i else 0)[0]
    want, wstatus = RBS.model_bits(p, u, r)
    assert all(wstatus[k] == s for k, s in planted.items()) and want[0][0] == 1 and (rows < 2 or want[1][0] == 0)
    ud = scl.to_device(RBS.to_limbs(f, u, mp))
    rbuf, rv = placed(scl.to_device(np.stack([RBS.to_limbs(f, row, mp) for row in r])), (pitch,))
    bbuf, bv = placed(torch.zeros_like(rv), (pitch,))
    b, status = rb.bits_finish(f, ud, rv, out=bv)
    note = (rows, N, pitch)
    assert status.cpu().tolist() == wstatus, note
    got = RBS.from_limbs(f, host(bv.contiguous()), mp)
    assert got == [v for row in want for v in row], note
    for k in planted:
        assert not bv[:, k].any().item(), note
    rest = bbuf.clone()
    torch.as_strided(rest, tuple(bv.shape), bv.stride(), bv.storage_offset() - bbuf.storage_offset()).zero_()
    assert not rest.any().item(), note


@pytest.mark.parametrize("name,f,mp", CASES, ids=IDS)
def test_bits_finish_equals_the_model(env, modulus, name, f, mp):
    """rows in {1, 3, 10}, row strides N and N + 3, N in {1, 65, 257} (Mersenne61 also 2, one pair and no tail, and 513, 256 pairs
    and the tail in lane 0 of the next block): a planted u = 0 and a planted non-residue carry their status and a column of
    zeros; Mersenne61 also at 17 rows (past the rows whose loads are issued before the chain); its odd strides take one column
    per lane, its even ones two"""
    mp = modulus(mp)
    p = RBS.prime(f, mp)
    tag = 100 * IDS.index(name)
    for N in (1, 65, 257) + ((2, 513) if f == O.M61 else ()):
        for rows in (1, 3, 10) + ((17,) if f == O.M61 else ()):
            for pitch in (N, N + 3):
                bits_case(env, f, mp, p, rows, N, pitch, tag + rows)


@pytest.mark.parametrize("n,t", [(4, 1), (10, 3)], ids=["4-1", "10-3"])
@pytest.mark.parametrize("f", [O.M61, O.M127], ids=["m61", "m127"])
def test_random_bits_end_to_end(env, f, n, t):
    """hm.double_share for every dealer, hm.apply_matrix with the hyper-invertible matrix, rb.random_bits: N = 257 bits.  No
    status byte is set; the shares 1..t+1 and the last t+1 shares reconstruct the same b, every b is 0 or 1 and equals the model's
    (r / root(r^2) + 1) / 2 of the reconstructed r; both values occur"""
    scl, rb, hm, port = env
    L, m, N, p = O.LIMBS[f], n - t, 257, RBS.prime(f)
    S = -(-2 * N // m)                                             # double sharings per dealer: 2 N extracted in all
    z = lambda *shape: torch.zeros(*shape, L, dtype=torch.int64, device="cuda")
    lo, hi, R_lo, R_hi = z(n, n, S), z(n, n, S), z(n, m, S), z(n, m, S)
    deal_all(hm, f, S, t, n, [b"rb dealer %d" % i for i in range(n)], lo, hi)
    Md = scl.to_device(hm.hyper_invertible(f, m, n))
    hm.apply_matrix(f, Md, lo.transpose(0, 1), out=R_lo)
    hm.apply_matrix(f, Md, hi.transpose(0, 1), out=R_hi)
    R_lo, R_hi = R_lo.reshape(n, m * S, L), R_hi.reshape(n, m * S, L)
    r = R_lo[:, :N]                                                # the random [r]_t; the next N double sharings mask the square
    b, status = rb.random_bits(f, r, R_lo[:, N:2 * N], R_hi[:, N:2 * N], scl.lagrange_basis(f, n), scl.lagrange_basis(f, t + 1))
    assert tuple(b.shape) == (n, N, L) and not status.any().item()
    first = RBS.from_limbs(f, host(scl.shamir_recover(f, b[:t + 1].contiguous())))
    nodes = np.stack([hm.element(f, i + 1) for i in range(n - t - 1, n)])
    last = RBS.from_limbs(f, host(scl.shamir_recover(f, b[n - t - 1:].contiguous(), lam=scl.lagrange_basis(f, t + 1, nodes))))
    rr = RBS.from_limbs(f, host(scl.shamir_recover(f, r[:t + 1].contiguous())))
    want, wstatus = RBS.model_bits(p, [v * v % p for v in rr], [rr])
    assert not any(wstatus) and first == last == want[0]
    assert set(first) == {0, 1}


_CAPTURE_CHILD = r"""
import json, sys
root = sys.argv[1]
sys.path[:0] = [root + "/secure-computation-library_amd", root + "/tests"]
import numpy as np
import torch
import rb_support as RBS
import scl_amd as scl
from scl_amd import rb

f, N, rows = scl.M61, 257, 3
p = RBS.prime(f)
torch.cuda.set_device(0)
a, u, r = scl.empty(f, N), scl.empty(f, N), scl.empty(f, rows, N)
root, b = scl.empty(f, N), scl.empty(f, rows, N)
st_a, st_b = (torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(2))
g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
with torch.cuda.stream(s):
    with torch.cuda.graph(g, stream=s):
        rb.sqrt(f, a, RBS.INVERSE, out=root, status=st_a)          # the first calls of this process
        rb.bits_finish(f, u, r, out=b, status=st_b)
torch.cuda.synchronize()
for rep in range(2):
    av = RBS.seeded(p, N, 50 + rep)
    uv = [v * v % p for v in RBS.seeded(p, N, 60 + rep)]
    uv[rep] = 0
    rv = [RBS.seeded(p, N, 70 + 3 * rep + i) for i in range(rows)]
    a.copy_(scl.to_device(RBS.to_limbs(f, av)))
    u.copy_(scl.to_device(RBS.to_limbs(f, uv)))
    r.copy_(scl.to_device(np.stack([RBS.to_limbs(f, row) for row in rv])))
    for t in (root, b, st_a, st_b):
        t.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    want = [RBS.model_sqrt(p, v, RBS.INVERSE) for v in av]
    assert RBS.from_limbs(f, scl.to_host(root)) == [v for v, _ in want] and st_a.cpu().tolist() == [s for _, s in want], rep
    wb, ws = RBS.model_bits(p, uv, rv)
    assert RBS.from_limbs(f, scl.to_host(b)) == [v for row in wb for v in row] and st_b.cpu().tolist() == ws and ws[rep] == RBS.ZERO, rep
print(json.dumps({"ok": True, "replays": 2}))
"""


def test_both_calls_are_capturable_from_their_first_call():
    """a fresh child process captures scl_rb_sqrt and scl_rb_bits_finish into one graph as its first calls of the library and
    replays it twice on new operands: root, bits and both status vectors equal the model"""
    r = subprocess.run([sys.executable, "-c", _CAPTURE_CHILD, RBS.cxx_support.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "replays": 2}


def test_wrapper_refuses_what_the_header_refuses(env):
    scl, rb, hm, port = env
    a = torch.zeros(8, 2, dtype=torch.int64, device="cuda")
    for tag, word in ((O.GF2_128, "bijection"), (O.Z2K(64), "not a field")):
        with pytest.raises(scl.SclError) as ei:
            rb.sqrt(tag, a[:, :1].contiguous() if tag == O.Z2K(64) else a)
        assert ei.value.status == scl.ERR_BAD_ARG and word in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        rb.sqrt(O.M127, a, flags=4)
    assert ei.value.status == scl.ERR_BAD_ARG and "flags" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        rb.bits_finish(O.M127, a, torch.zeros(3, 8, 2, dtype=torch.int64, device="cuda"), out=torch.zeros(3, 9, 2, dtype=torch.int64, device="cuda"))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        rb.bits_finish(O.M127, a, a, out=a)
    assert ei.value.status == scl.ERR_BAD_ARG and "overlaps" in str(ei.value)
    assert not a.any()


def test_cxx_round_trips(env):
    """tests/cxx/test_rb_api.cc --gpu, a fresh child process: hip::sqrt and hip::bitsFinish equal the host forms math::sqrt and
    ss::randomBitFinish word for word"""
    r = subprocess.run([RBS.rb_api_binary(), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
