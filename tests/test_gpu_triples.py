"""The triple dealer on the GPU (scl_amd.prep over libscl_hip_prep.so) against the Python model of tests/port_models.py, which
tests/test_triples_host.py pins to what the reference dealt: device output equals the model byte for byte.

Shapes: N in {1, 2, 3, 64, 257} -- one triple, one pair (the two-per-lane form of Mersenne61), a pair and the tail launch, a
wavefront, a block and one; additive n in {2, 3, 5}; Shamir (4,1), (10,3), (16,7) -- fused for Mersenne61, Mersenne127 and
GF(2^128), two passes for the Montgomery fields -- and (20,9), two passes everywhere.  Fused equals two-pass (flags = 1) wherever
both exist.  counter0 = 2^32 - 5 with N = 3 puts the launch across a multiple of 2^32 blocks (the eight-lookup first round).  A
shard dealt at counter0 = f B equals its slice of the long run.  Mersenne61 also on an odd stride and a base 8 bytes past a
16-byte boundary (the one-per-lane form).  Then the protocol: the fixture's "Beaver multiplication protocol" run end to end on
the device from PRG::create(), (10,3) with 257 secrets against the oracle's x y, and the chain captured into one graph.

One model run per (field, scheme, shape) at N = 257; every smaller N is a prefix of it (triple s does not depend on N)."""
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
from cxx_support import mirror_binary
from gpu_support import TRIPLES_N, fname, gpu_env, host, rnd
from gpu_support import TRIPLES_SEED as SEED
from gpu_support import triples_reference as reference
from port_models import additive_blocks, from_hex, golden, model_shamir, protocol_from_model, shamir_blocks

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
RINGS = [O.Z2K(1), O.Z2K(62), O.Z2K(64), O.Z2K(65), O.Z2K(128)]
FUSED_FIELDS = [O.M61, O.M127, O.GF2_128]
NS = [1, 2, 3, 64, 257]
NMAX = max(NS)
assert NMAX == TRIPLES_N          # the shape of the shared reference (tests/gpu_support.py)
ADDITIVE_N = [2, 3, 5]
SHAMIR_NT = [(4, 1), (10, 3), (16, 7), (20, 9)]


@pytest.fixture(scope="module")
def env():
    return gpu_env("mpc", "prep")


def same(got, want, N, note):
    for g, w, k in zip(got, want, "abc"):
        assert np.array_equal(host(g), w[:, :N]), f"{note}: {k}"


def expect_scratch(prep, f, N, n, t, flags=0):
    need = prep.triples_scratch_bytes(f, N, n, t, flags)
    fused = f in FUSED_FIELDS and t <= 7 and not flags
    assert need == (0 if fused else (3 + 3 * t) * N * 8 * O.LIMBS[f]), (fname(f), N, n, t, flags)
    return fused


@pytest.mark.parametrize("f", FIELDS + RINGS, ids=fname)
def test_additive_triples_equal_the_model(env, f):
    scl, mpc, prep, port = env
    for n in ADDITIVE_N:
        want = reference(port, f, n)
        for N in NS:
            same(prep.deal_triples_additive(f, N, n, SEED), want, N, f"{fname(f)} additive n={n} N={N}")


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_shamir_triples_equal_the_model(env, f):
    """fused where the header says so, two passes elsewhere; and the two paths deal the same triples"""
    scl, mpc, prep, port = env
    for n, t in SHAMIR_NT:
        want = reference(port, f, n, t)
        for N in NS:
            fused = expect_scratch(prep, f, N, n, t)
            same(prep.deal_triples_shamir(f, N, t, n, SEED), want, N, f"{fname(f)} Shamir ({n},{t}) N={N} {'fused' if fused else 'two-pass'}")
            if fused:
                expect_scratch(prep, f, N, n, t, prep.TWO_PASS)
                same(prep.deal_triples_shamir(f, N, t, n, SEED, flags=prep.TWO_PASS), want, N, f"{fname(f)} Shamir ({n},{t}) N={N} forced two-pass")


@pytest.mark.parametrize("f", FUSED_FIELDS, ids=fname)
def test_every_fused_threshold(env, f):
    """t = 0 .. 7 each have a kernel of their own (and 8 is the first two-pass threshold): n = 6, N = 67"""
    scl, mpc, prep, port = env
    for t in range(9):
        assert expect_scratch(prep, f, 67, 6, t) == (t <= 7)
        same(prep.deal_triples_shamir(f, 67, t, 6, SEED), reference(port, f, 6, t, N=67), 67, f"{fname(f)} Shamir (6,{t})")


@pytest.mark.parametrize("f", FIELDS + RINGS[-2:], ids=fname)
def test_a_launch_across_a_multiple_of_2_to_the_32_blocks(env, f):
    """counter0 = 2^32 - 5, N = 3: the first triple starts below the boundary, the last ends above it"""
    scl, mpc, prep, port = env
    c0, N = 2 ** 32 - 5, 3
    assert c0 + N * additive_blocks(f, 3) > 2 ** 32 > c0
    same(prep.deal_triples_additive(f, N, 3, SEED, counter0=c0), reference(port, f, 3, None, c0, N), N, f"{fname(f)} additive straddle")
    if f in FIELDS:
        for n, t in ((10, 3), (20, 9)):
            assert c0 + N * shamir_blocks(f, t) > 2 ** 32
            same(prep.deal_triples_shamir(f, N, t, n, SEED, counter0=c0), reference(port, f, n, t, c0, N), N, f"{fname(f)} Shamir ({n},{t}) straddle")


@pytest.mark.parametrize("f", [O.M61, O.GF2_128, O.SECP256K1_SCALAR], ids=fname)
def test_a_shard_equals_its_slice_of_the_long_run(env, f):
    """triples [first, first + k) dealt with counter0 = first * B"""
    scl, mpc, prep, port = env
    first, k = 100, 57
    want = [m[:, first:first + k] for m in reference(port, f, 3)]
    same(prep.deal_triples_additive(f, k, 3, SEED, counter0=first * prep.triple_blocks(f, prep.ADDITIVE, 3)), want, k, f"{fname(f)} additive shard")
    for n, t in ((10, 3), (20, 9)):
        want = [m[:, first:first + k] for m in reference(port, f, n, t)]
        got = prep.deal_triples_shamir(f, k, t, n, SEED, counter0=first * prep.triple_blocks(f, prep.SHAMIR, n, t))
        same(got, want, k, f"{fname(f)} Shamir ({n},{t}) shard")


def test_mersenne61_on_an_odd_stride_and_an_odd_base(env):
    """the two-per-lane form needs 16-byte bases and an even stride: everything else is one triple per lane, the same triples"""
    scl, mpc, prep, port = env
    f = O.M61
    for N in (2, 3, 64, 257):
        for stride, phase in ((N + (N % 2) + 1, 0), (N + (N % 2), 1), (N + (N % 2) + 1, 1), (N + (N % 2) + 2, 0)):
            assert stride >= N
            for n, t in ((3, None), (10, 3), (20, 9)):
                buf = torch.zeros(3 * n * stride + 2, dtype=torch.int64, device="cuda")
                out = [torch.as_strided(buf, (n, N, 1), (stride, 1, 1), phase + m * n * stride) for m in range(3)]
                if t is None:
                    prep.deal_triples_additive(f, N, n, SEED, out=out)
                else:
                    prep.deal_triples_shamir(f, N, t, n, SEED, out=out)
                same(out, reference(port, f, n, t), N, f"m61 N={N} stride={stride} phase={8 * phase} n={n} t={t}")
                gaps = torch.ones(3 * n * stride + 2, dtype=torch.bool)
                for m in range(3):
                    for i in range(n):
                        lo = phase + (m * n + i) * stride
                        gaps[lo:lo + N] = False
                assert not buf.cpu()[gaps].any(), f"m61 N={N} stride={stride} phase={8 * phase} n={n} t={t}: a row gap was written"


def test_the_references_protocol_test_end_to_end_on_the_device(env):
    """test_protocol.cc:36-41 and BeaverMul for both parties from PRG::create(): xs and ys by the engine's additive_share_prg at
    blocks 0 and 1, the triple dealt at block 2, mask, open, finish (party 0 adds e d), recover: every value is the fixture's, the
    product is 462"""
    scl, mpc, prep, port = env
    f, g, seed = O.M61, golden("triples")["protocol"], b""
    x, y = scl.to_device(port.from_int(f, 42)[None]), scl.to_device(port.from_int(f, 11)[None])
    xs = scl.additive_share_prg(f, x, 2, seed, counter0=0)
    ys = scl.additive_share_prg(f, y, 2, seed, counter0=1)
    a, b, c = prep.deal_triples_additive(f, 1, 2, seed, counter0=2)
    for t, k in ((xs, "xs"), (ys, "ys"), (a, "a"), (b, "b"), (c, "c")):
        assert np.array_equal(host(t)[:, 0], from_hex(port, f, g[k])), k
    e_rows, d_rows = mpc.beaver_mask(f, xs, ys, a, b)
    e, d = scl.additive_recover(f, e_rows), scl.additive_recover(f, d_rows)
    assert np.array_equal(np.concatenate([host(e_rows)[:, 0], host(e)]), from_hex(port, f, g["e"]))
    assert np.array_equal(np.concatenate([host(d_rows)[:, 0], host(d)]), from_hex(port, f, g["d"]))
    z = mpc.beaver_finish(f, e, d, a, b, c, 1)
    total = scl.additive_recover(f, z)
    assert np.array_equal(np.concatenate([host(z)[:, 0], host(total)]), from_hex(port, f, g["z"]))
    assert O.to_ints(host(total)) == [462]
    m = protocol_from_model(port)
    assert np.array_equal(host(a)[:, 0], m["a"]) and np.array_equal(host(c)[:, 0], m["c"])


@pytest.mark.parametrize("f", [O.M61, O.GF2_128, O.SECP256K1_SCALAR], ids=fname)
def test_shamir_multiplication_from_one_seed(env, f):
    """(10,3), 257 secrets: x and y shared by the engine, the triples dealt behind them on the same PRG stream, mask, open, finish
    (every party adds e d), recover: the oracle's x y"""
    scl, mpc, prep, port = env
    n, t, N = 10, 3, 257
    x, y = rnd(port, f, N, b"triples-x"), rnd(port, f, N, b"triples-y")
    per = ((t + 1) * O.byte_size(f) + 15) // 16                      # blocks one shamirSecretShare draws
    xs = scl.shamir_share_prg(f, scl.to_device(x), t, n, SEED, counter0=0)
    ys = scl.shamir_share_prg(f, scl.to_device(y), t, n, SEED, counter0=N * per)
    a, b, c = prep.deal_triples_shamir(f, N, t, n, SEED, counter0=2 * N * per)
    same((a, b, c), reference(port, f, n, t, 2 * N * per, N), N, f"{fname(f)} triples behind the shares")
    assert np.array_equal(host(scl.shamir_recover(f, c)), port.ew(f, O.MUL, host(scl.shamir_recover(f, a)), host(scl.shamir_recover(f, b))))
    e_rows, d_rows = mpc.beaver_mask(f, xs, ys, a, b)
    e, d = scl.shamir_recover(f, e_rows), scl.shamir_recover(f, d_rows)
    z = mpc.beaver_finish(f, e, d, a, b, c, n)
    assert np.array_equal(host(scl.shamir_recover(f, z)), port.ew(f, O.MUL, x, y))
    assert np.array_equal(host(scl.shamir_recover(f, z[:t + 1])), port.ew(f, O.MUL, x, y))          # [z] is a degree-t sharing


@pytest.mark.parametrize("f,flags", [(O.M61, 0), (O.M61, 1), (O.SECP256K1_SCALAR, 0), (O.MONT128, 0)],
                         ids=["m61-fused", "m61-two-pass", "secp_scalar-two-pass", "mont128-two-pass"])
def test_the_chain_captured_into_one_graph(env, f, flags):
    """deal -> mask -> open -> finish -> recover on one stream, captured as a linear chain and replayed once with the outputs
    cleared in between.  The fused deal and the two-pass one (forced, and as the Montgomery fields take it), whose scratch is the
    caller's and whose engine tables exist after the run before the capture, as the header asks"""
    scl, mpc, prep, port = env
    n, t, N, L = 10, 3, 1000, O.LIMBS[f]
    need = prep.triples_scratch_bytes(f, N, n, t, flags)
    assert (need == 0) == (f == O.M61 and not flags)
    scratch = torch.zeros(need // 8, dtype=torch.int64, device="cuda") if need else None
    x, y = rnd(port, f, N, b"graph-x"), rnd(port, f, N, b"graph-y")
    xs = scl.shamir_share_prg(f, scl.to_device(x), t, n, b"graph-xs")
    ys = scl.shamir_share_prg(f, scl.to_device(y), t, n, b"graph-ys")
    lam = scl.lagrange_basis(f, n)
    abc = [torch.zeros(n, N, L, dtype=torch.int64, device="cuda") for _ in range(3)]
    de = torch.zeros(2 * n, N, L, dtype=torch.int64, device="cuda")
    ed = torch.zeros(2, N, L, dtype=torch.int64, device="cuda")
    z = torch.zeros(n, N, L, dtype=torch.int64, device="cuda")
    out = torch.zeros(N, L, dtype=torch.int64, device="cuda")

    def chain():
        a, b, c = prep.deal_triples_shamir(f, N, t, n, b"graph-triples", counter0=7, out=abc, scratch=scratch, flags=flags)
        e_rows, d_rows = mpc.beaver_mask(f, xs, ys, a, b, out=de)
        scl.shamir_recover(f, e_rows, lam=lam, out=ed[0])
        scl.shamir_recover(f, d_rows, lam=lam, out=ed[1])
        mpc.beaver_finish(f, ed[0], ed[1], a, b, c, n, out=z)
        scl.shamir_recover(f, z, lam=lam, out=out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                   # every kernel has run once before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = port.ew(f, O.MUL, x, y)
    assert np.array_equal(host(out), want)
    triples = [host(m).copy() for m in abc]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for m in abc + [de, ed, z, out] + ([scratch] if need else []):
        m.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(out), want)
    for m, w in zip(abc, triples):
        assert np.array_equal(host(m), w)
    same(abc, model_shamir(port, f, b"graph-triples", 7, N, t, n), N, "the captured deal")


@pytest.mark.parametrize("f,flags", [(O.MONT128, 0), (O.SECP256K1_SCALAR, 0), (O.SECP256K1_FIELD, 0), (O.M61, 1), (O.M127, 1), (O.GF2_128, 1)],
                         ids=["mont128", "secp_scalar", "secp_field", "m61-forced", "m127-forced", "gf128-forced"])
def test_two_passes_at_threshold_zero(env, f, flags):
    """t = 0 on the two-pass path: the first pass writes a, b, c alone (3 N elements of scratch) and the engine shares constant
    polynomials without coefficient rows; every party's share is the secret"""
    scl, mpc, prep, port = env
    for n, N in ((1, 3), (4, 67), (20, 257)):
        assert prep.triples_scratch_bytes(f, N, n, 0, flags) == 3 * N * 8 * O.LIMBS[f]
        got = prep.deal_triples_shamir(f, N, 0, n, SEED, flags=flags)
        same(got, reference(port, f, n, 0, N=N), N, f"{fname(f)} two-pass (n={n}, t=0) N={N}")
        for m in got:
            assert all(np.array_equal(host(m[i]), host(m[0])) for i in range(n))


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_largest_threshold_the_dealer_takes(env, f):
    """t = 48 (16 for the 32-byte fields): the last threshold at which the engine's share call stays asynchronous; one past it
    is refused"""
    scl, mpc, prep, port = env
    t = 16 if O.LIMBS[f] == 4 else 48
    n, N = t + 2, 67
    same(prep.deal_triples_shamir(f, N, t, n, SEED), reference(port, f, n, t, N=N), N, f"{fname(f)} Shamir ({n},{t})")
    with pytest.raises(scl.SclError) as ei:
        prep.deal_triples_shamir(f, N, t + 1, n + 1, SEED)
    assert ei.value.status == scl.ERR_BAD_ARG and "threshold" in str(ei.value)


def test_wrapper_refuses_what_the_header_refuses(env):
    scl, mpc, prep, port = env
    with pytest.raises(scl.SclError) as ei:
        prep.deal_triples_additive(O.M61, 8, 1, SEED)
    assert ei.value.status == scl.ERR_BAD_ARG and "n must be >= 2" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        prep.deal_triples_shamir(O.Z2K(64), 8, 1, 4, SEED)
    assert ei.value.status == scl.ERR_BAD_ARG
    with pytest.raises(scl.SclError) as ei:
        prep.deal_triples_shamir(O.M61, 8, 1, 4, SEED, flags=2)
    assert ei.value.status == scl.ERR_BAD_ARG and "flags" in str(ei.value)
    m = torch.zeros(4, 8, 1, dtype=torch.int64, device="cuda")
    with pytest.raises(scl.SclError) as ei:
        prep.deal_triples_shamir(O.M61, 8, 1, 4, SEED, out=(m, m, torch.zeros_like(m)))           # a is b
    assert ei.value.status == scl.ERR_BAD_ARG and "overlap" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        prep.deal_triples_shamir(O.M61, 8, 9, 4, SEED, scratch=torch.zeros(8, dtype=torch.int64, device="cuda"))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    assert not m.any()


def test_cxx_round_trips(env):
    """tests/cxx/test_triples_api.cc --gpu: hip::dealTriplesAdditive / dealTriplesShamir equal the per-secret calls on one PRG,
    and deal, mask, open, finish, recover multiplies"""
    r = subprocess.run([mirror_binary("triples"), "--gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
