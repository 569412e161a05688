"""Batch verification on the GPU (scl_amd.vf over libscl_hip_vf.so) against the Python model of tests/port_models.py, which
tests/test_vf_host.py pins to what the reference produced: device output equals the model byte for byte.  Each test's docstring names its
shapes.  One model run per field -- out[r][j] depends on row r and coefficient vector j alone, so every smaller row count and
repetition count is a slice of the largest -- and one upload; every layout is a device copy of it."""
import numpy as np
import pytest
import torch

import oracle_lib as O
from cxx_support import mirror_binary
from gpu_support import fname, gpu_env, host, only_the_view_was_written, placed, pm1, pool
from port_models import TAGS3 as TAGS
from port_models import coin_blocks, degree_entry, from_hex, golden, hex_rows, model_coins, model_combine, product_entry

pytestmark = pytest.mark.gpu

FIELDS = [O.M61, O.M127, O.MONT128, O.GF2_128, O.SECP256K1_SCALAR, O.SECP256K1_FIELD]
NS = [1, 2, 3, 63, 64, 65, 257, 1025]       # 3 and 257: the odd-N half block of Mersenne61; 63 .. 65: the wave edge
REPS = [1, 2, 4]
RMAX, JMAX = 11, 4
SEED, C0 = b"vf gpu coin", 5                # a non-zero block counter


@pytest.fixture(scope="module")
def env():
    return gpu_env("vf", "hm", "prep")


def row_counts(vf, f, reps, prg):
    """1, 2, R, R + 1 and 10: a full group of rows, a partial one, and more than one group"""
    R = vf.launch_shape(f, reps, prg)[0]
    return sorted({1, 2, R, R + 1, 10})


def second_trip_N(vf, f, reps, prg):
    """the smallest N at which a lane takes a second trip -- every workgroup the grid allows writes a partial, and the lanes of
    the first take another pack --, from the unit's own launch constants, plus 3 (odd: Mersenne61's half block)"""
    _, cols, groups, _ = vf.launch_shape(f, reps, prg)
    return cols * groups + 3


_REF = {}


def reference(scl, port, f):
    """x, y [RMAX][1025][L] on the device, and per N the coefficient rows rho [JMAX][N][L] (host and device) with the model's
    plain and product combinations [RMAX][JMAX][L]"""
    if f not in _REF:
        L, NMAX = O.LIMBS[f], max(NS)
        x = pool(port, f, RMAX * NMAX, b"vf-x").reshape(RMAX, NMAX, L)
        y = pool(port, f, RMAX * NMAX + 7, b"vf-y")[7:].reshape(RMAX, NMAX, L)
        per = {}
        for N in NS:
            rho = model_coins(port, f, SEED, C0, N, JMAX)
            per[N] = (rho, scl.to_device(rho), model_combine(port, f, x[:, :N], rho), model_combine(port, f, x[:, :N], rho, y[:, :N]))
        _REF[f] = (scl.to_device(x), scl.to_device(y), per)
    return _REF[f]


# ---- values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_both_forms_equal_the_model(env, f):
    """combine_prg and combine, plain and product: N 1, 2, 3, 63, 64, 65, 257, 1025 x reps 1, 2, 4 x rows 1, 2, R, R + 1, 10 at a
    row pitch above N (even and odd) and a pitched out; for the one-limb field also 8 bytes past a 16-byte boundary, the
    one-column path.  A non-zero counter0.  The inputs are unchanged, the gaps of out unwritten."""
    scl, vf, hm, prep, port = env
    xd, yd, per = reference(scl, port, f)
    for N in NS:
        rho, rho_d, w_plain, w_prod = per[N]
        layouts = [(N + 2 + (N % 2), 0), (N + 3 + (N % 2), 0)] + ([(N + 2 + (N % 2), 1)] if O.LIMBS[f] == 1 else [])
        for pitch, phase in layouts:
            _, xv = placed(xd[:, :N], (pitch,), phase)
            _, yv = placed(yd[:, :N], (pitch,), phase)
            _, rv = placed(rho_d, (pitch,), phase)
            for reps in REPS:
                for prg in (True, False):
                    for rows in row_counts(vf, f, reps, prg):
                        for y, want in ((None, w_plain), (yv, w_prod)):
                            note = f"{fname(f)} N={N} pitch={pitch} phase={phase} reps={reps} rows={rows} {'prg' if prg else 'rows'} {'plain' if y is None else 'product'}"
                            obuf, ov = placed(torch.zeros(rows, reps, O.LIMBS[f], dtype=torch.int64, device="cuda"), (reps + 3,), phase)
                            yy = None if y is None else y[:rows]
                            if prg:
                                got = vf.combine_prg(f, xv[:rows], yy, seed=SEED, counter0=C0, reps=reps, out=ov)
                            else:
                                got = vf.combine(f, xv[:rows], rv[:reps], yy, out=ov)
                            assert got.data_ptr() == ov.data_ptr()
                            assert np.array_equal(host(ov), want[:rows, :reps]), note
                            assert only_the_view_was_written(obuf, ov), note + ": a gap was written"
            assert torch.equal(xv, xd[:, :N]) and torch.equal(yv, yd[:, :N]) and torch.equal(rv, rho_d), f"{fname(f)} N={N}: an input changed"
    # dense operands, out allocated by the wrapper, x == y: sum rho x^2
    rho, rho_d, w_plain, _ = per[257]
    x = xd[:3, :257].contiguous()
    assert np.array_equal(host(vf.combine(f, x, rho_d[:2])), w_plain[:3, :2])
    assert np.array_equal(host(vf.combine(f, x, rho_d[:2], x)), model_combine(port, f, host(x), rho[:2], host(x)))
    assert np.array_equal(host(vf.combine_prg(f, x, x, seed=SEED, counter0=C0, reps=2)), model_combine(port, f, host(x), rho[:2], host(x)))


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_a_lane_takes_a_second_trip(env, f):
    """one N from the unit's own launch constants, cols_per_trip * max_groups + 3: every workgroup the grid allows writes a
    partial and some lanes take a second pack; one row (the model's cost over GF(2^128) is what sets it), reps 2, both forms,
    both calls (each at its own geometry)"""
    scl, vf, hm, prep, port = env
    L = O.LIMBS[f]
    model = {}
    for prg in (True, False):
        N = second_trip_N(vf, f, 2, prg)
        x = pool(port, f, N, b"vf-big-x").reshape(1, N, L)
        y = pool(port, f, N + 3, b"vf-big-y")[3:].reshape(1, N, L)
        rho = model_coins(port, f, SEED, C0, N, 2)
        xd, yd = scl.to_device(x), scl.to_device(y)
        for yy, yh in ((None, None), (yd, y)):
            if (N, yh is None) not in model:                    # the two calls of a two-pass field share one geometry: one model run
                model[N, yh is None] = model_combine(port, f, x, rho, yh)
            want = model[N, yh is None]
            got = vf.combine_prg(f, xd, yy, seed=SEED, counter0=C0, reps=2) if prg else vf.combine(f, xd, scl.to_device(rho), yy)
            assert np.array_equal(host(got), want), f"{fname(f)} N={N} {'prg' if prg else 'rows'} {'plain' if yy is None else 'product'}"


def test_the_empty_sum_is_zero(env):
    """N == 0 with rows > 0 writes zeros"""
    scl, vf, hm, prep, port = env
    for f in FIELDS:
        L = O.LIMBS[f]
        x = torch.zeros(3, 0, L, dtype=torch.int64, device="cuda")
        out = torch.full((3, 2, L), -1, dtype=torch.int64, device="cuda")
        vf.combine_prg(f, x, seed=SEED, reps=2, out=out)
        assert not out.any().item(), fname(f)
        out.fill_(-1)
        vf.combine(f, x, torch.zeros(2, 0, L, dtype=torch.int64, device="cuda"), x, out=out)
        assert not out.any().item(), fname(f)


# ---- the worst case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_worst_case_operands_through_combine(env, f):
    """x = y = rho = p - 1 everywhere (GF(2^128): all ones) at N 1 .. 1025 x reps 1, 4 x rows 1, R + 1, plain and product.  All
    three operands are views of ONE buffer from its start -- inputs may overlap."""
    scl, vf, hm, prep, port = env
    L, top = O.LIMBS[f], pm1(port, f)
    rows_max = max(vf.launch_shape(f, reps, False)[0] for reps in (1, 4)) + 1
    buf = scl.to_device(np.tile(top, (max(rows_max, JMAX) * max(NS), 1)))
    for N in NS:
        tops = np.tile(top, (1, N, 1))
        w_plain, w_prod = model_combine(port, f, tops, tops)[0, 0], model_combine(port, f, tops, tops, tops)[0, 0]
        for reps in (1, 4):
            R = vf.launch_shape(f, reps, False)[0]
            for rows in (1, R + 1):
                rho, x = buf[:reps * N].reshape(reps, N, L), buf[:rows * N].reshape(rows, N, L)
                note = f"{fname(f)} N={N} reps={reps} rows={rows}"
                assert np.array_equal(host(vf.combine(f, x, rho)), np.tile(w_plain, (rows, reps, 1))), note
                assert np.array_equal(host(vf.combine(f, x, rho, x)), np.tile(w_prod, (rows, reps, 1))), note + " product"


def test_mersenne61_passes_its_term_bound_in_a_lane_and_in_the_second_stage(env):
    """Mersenne61 promises 64 terms.  (a) N = 65 * cols_per_trip + 1: 66 workgroups, the second stage sums more than 64 partials.
    (b) N = 8 * cols_per_trip * max_groups + 5 of the streaming form (2^24 + 5 columns, 128 MiB): a lane's ninth trip brings
    its 65th .. 72nd term.  x = y = rho = p - 1 in one buffer: (p-1)^2 = 1 and (p-1)^3 = -1, so the plain form is N and the
    product form -N (mod p), which the model confirms at (a).  (c) the same N through the fused kernel with the PRG's coins."""
    scl, vf, hm, prep, port = env
    f, p = O.M61, (1 << 61) - 1
    _, cols, groups, _ = vf.launch_shape(f, 1, False)
    Na, Nb = 65 * cols + 1, 8 * cols * groups + 5
    assert Nb < 1 << 26
    buf = torch.full((2 * Nb, 1), p - 1, dtype=torch.int64, device="cuda")
    top = np.full((1, Na, 1), p - 1, dtype=np.uint64)
    assert O.to_ints(model_combine(port, f, top, top)[0]) == [Na % p] and O.to_ints(model_combine(port, f, top, top, top)[0]) == [p - Na]
    for N in (Na, Nb):
        x = buf[:N].reshape(1, N, 1)
        for reps in (1, 2):
            rho = torch.as_strided(buf, (reps, N, 1), (N, 1, 1))                                # rho_0 is x itself
            assert O.to_ints(host(vf.combine(f, x, rho)).reshape(reps, 1)) == [N % p] * reps, N
            assert O.to_ints(host(vf.combine(f, x, rho, x)).reshape(reps, 1)) == [p - N] * reps, N
    # the fused kernel past the bound: it cannot be fed the worst case, so at (b) its coins stand in -- combine_prg equals combine
    # on rows filled by scl_hip_vector_random, where a fused lane's 17th trip brings its 65th term (4 terms a trip at reps 1)
    _, fcols, fgroups, fused = vf.launch_shape(f, 1, True)
    assert fused and Nb > 16 * fcols * fgroups
    x, y = buf[:Nb].reshape(1, Nb, 1), buf[Nb:].reshape(1, Nb, 1)
    scl.vector_random(f, Nb, b"vf bound x", 0, out=buf[:Nb])
    rho = scl.vector_random(f, Nb, SEED, C0).reshape(1, Nb, 1)
    assert torch.equal(vf.combine_prg(f, x, seed=SEED, counter0=C0), vf.combine(f, x, rho))
    assert torch.equal(vf.combine_prg(f, x, y, seed=SEED, counter0=C0), vf.combine(f, x, rho, y))


# ---- the coin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_the_coin_is_vector_random_at_counter0_plus_j_blocks(env, f):
    """combine_prg == combine on rho rows filled by scl_hip_vector_random at counter0 + j B, B = coin_blocks; N 3, 257, 1025,
    reps 1 .. 4"""
    scl, vf, hm, prep, port = env
    xd, yd, per = reference(scl, port, f)
    for N in (3, 257, 1025):
        B = vf.coin_blocks(f, N)
        assert B == coin_blocks(f, N)
        for reps in (1, 2, 3, 4):
            rho = torch.stack([scl.vector_random(f, N, SEED, C0 + j * B) for j in range(reps)])
            assert np.array_equal(host(rho), per[N][0][:reps])
            x, y = xd[:10, :N].contiguous(), yd[:10, :N].contiguous()
            for yy in (None, y):
                assert torch.equal(vf.combine_prg(f, x, yy, seed=SEED, counter0=C0, reps=reps), vf.combine(f, x, rho, yy)), (fname(f), N, reps)


@pytest.mark.parametrize("f", FIELDS, ids=fname)
def test_equals_the_composition_of_existing_entry_points(env, f):
    """N = 1025, 10 rows, reps 2: scl_hip_vector_random + (scl_hip_ew MUL +) scl_hip_dot per row"""
    scl, vf, hm, prep, port = env
    xd, yd, per = reference(scl, port, f)
    N, rows, reps = 1025, 10, 2
    B = vf.coin_blocks(f, N)
    x, y = xd[:rows, :N].contiguous(), yd[:rows, :N].contiguous()
    plain = host(vf.combine_prg(f, x, seed=SEED, counter0=C0, reps=reps))
    prod = host(vf.combine_prg(f, x, y, seed=SEED, counter0=C0, reps=reps))
    for j in range(reps):
        rho = scl.vector_random(f, N, SEED, C0 + j * B)
        for r in range(rows):
            assert np.array_equal(plain[r, j], scl.dot(f, rho, x[r]).reshape(-1)), (fname(f), r, j)
            assert np.array_equal(prod[r, j], scl.dot(f, rho, scl.ew(f, O.MUL, x[r], y[r])).reshape(-1)), (fname(f), r, j)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_the_fixture_end_to_end_on_the_device(env):
    """the reference's combinations (the first N columns of rows 5 apart), its degree check -- check_degree passes on the good
    sharings, opens the reference's value and reports the altered one -- and its product check"""
    scl, vf, hm, prep, port = env
    g = golden("vf")
    for e in g["combine"]:
        f = TAGS[e["field"]]
        x, y = scl.to_device(hex_rows(port, f, e["x"])), scl.to_device(hex_rows(port, f, e["y"]))
        for r in e["runs"]:
            N = r["N"]
            for reps in (1, 2):
                assert np.array_equal(host(vf.combine_prg(f, x[:, :N], seed=b"vf coin", counter0=r["counter0"], reps=reps)),
                                      hex_rows(port, f, r["plain"])[:, :reps]), (e["field"], N, reps)
                assert np.array_equal(host(vf.combine_prg(f, x[:, :N], y[:, :N], seed=b"vf coin", counter0=r["counter0"], reps=reps)),
                                      hex_rows(port, f, r["product"])[:, :reps]), (e["field"], N, reps)
    for e in g["degree"]:
        f, n, t = TAGS[e["field"]], e["n"], e["t"]
        rows, _, _ = degree_entry(port, f, e)
        d = scl.to_device(rows)
        combined = vf.combine_prg(f, d, seed=b"vf coin", counter0=e["counter0"])
        assert np.array_equal(host(combined)[:, 0], from_hex(port, f, e["combined"]))
        assert np.array_equal(host(vf.check_degree(f, combined, n - t, t)), from_hex(port, f, [e["opened"]]))
        d[e["party"], e["column"]] = scl.ew(f, O.ADD, d[e["party"], e["column"]][None].contiguous(), scl.to_device(port.from_int(f, 1)[None]))[0]
        bad = vf.combine_prg(f, d, seed=b"vf coin", counter0=e["counter0"])
        assert np.array_equal(host(bad)[:, 0], from_hex(port, f, e["combined_bad"]))
        with pytest.raises(scl.SclError) as ei:
            vf.check_degree(f, bad, n - t, t)
        assert ei.value.status == scl.ERR_ERROR_DETECTED and ei.value.reference_message == "error detected during recovery"
    for e in g["product"]:
        f, n, t = TAGS[e["field"]], e["n"], e["t"]
        a, b, c, _ = [scl.to_device(v) for v in product_entry(port, f, e)]
        check = lambda cc: scl.ew(f, O.SUB, vf.combine_prg(f, a, b, seed=b"vf coin", counter0=e["counter0"])[:, 0].contiguous(),
                                  vf.combine_prg(f, cc, seed=b"vf coin", counter0=e["counter0"])[:, 0].contiguous())
        v = check(c)
        assert np.array_equal(host(v), from_hex(port, f, e["v"]))
        assert not vf.check_degree(f, v[:, None], n - 2 * t, 2 * t).any().item()
        delta = scl.to_device(np.repeat(from_hex(port, f, [e["delta"]]), n, axis=0))
        c[:, e["column"]] = scl.ew(f, O.ADD, c[:, e["column"]].contiguous(), delta)
        v_bad = check(c)
        assert np.array_equal(host(v_bad), from_hex(port, f, e["v_bad"]))
        assert np.array_equal(host(vf.check_degree(f, v_bad[:, None], n - 2 * t, 2 * t)), from_hex(port, f, [e["off"]]))


# ---- the protocol chains -------------------------------------------------------------------------------------------------------
CHAINS = [(O.M61, 2), (O.SECP256K1_SCALAR, 1)]


def double_chain(scl, vf, hm, f, n, t, N, reps, lo, hi, out_lo, out_hi, s_deal, s_lo, s_hi):
    """the launches of chain 1: deal N double sharings, combine both halves with ONE coin"""
    hm.double_share(f, N, t, n, b"vf dealer", out=(lo, hi), scratch=s_deal)
    vf.combine_prg(f, lo, seed=b"vf chain coin", counter0=C0, reps=reps, out=out_lo, scratch=s_lo)
    vf.combine_prg(f, hi, seed=b"vf chain coin", counter0=C0, reps=reps, out=out_hi, scratch=s_hi)


def chain_buffers(vf, hm, f, n, t, N, reps):
    L = O.LIMBS[f]
    z = lambda *shape: torch.zeros(*shape, L, dtype=torch.int64, device="cuda")
    need = hm.double_scratch_bytes(f, N, n, t, 0)
    sv = lambda: torch.zeros(vf.scratch_bytes(f, n, reps, N, vf.PRG) // 8, dtype=torch.int64, device="cuda")
    return dict(lo=z(n, N), hi=z(n, N), out_lo=z(n, reps), out_hi=z(n, reps),
                s_deal=torch.zeros(need // 8, dtype=torch.int64, device="cuda") if need else None, s_lo=sv(), s_hi=sv())


@pytest.mark.parametrize("f,reps", CHAINS, ids=["m61-reps2", "secp_scalar-reps1"])
def test_double_sharings_are_verified(env, f, reps):
    """(10, 3), N = 257: deal with scl_hm_double_share_prg, combine both halves with one coin, check degree t and degree 2t: both
    pass and open to the same value; a row of the degree-t half perturbed in one column is detected"""
    scl, vf, hm, prep, port = env
    n, t, N = 10, 3, 257
    B = chain_buffers(vf, hm, f, n, t, N, reps)
    double_chain(scl, vf, hm, f, n, t, N, reps, **B)
    v_lo = vf.check_degree(f, B["out_lo"], n - t, t)
    v_hi = vf.check_degree(f, B["out_hi"], n - 2 * t, 2 * t)
    assert torch.equal(v_lo, v_hi) and v_lo.any().item()
    rho = model_coins(port, f, b"vf chain coin", C0, N, reps)
    r = host(scl.shamir_recover(f, B["lo"][:t + 1].contiguous()))                                   # the N shared values
    assert np.array_equal(host(v_lo), model_combine(port, f, r[None], rho)[0])
    B["lo"][4, 17] = scl.ew(f, O.ADD, B["lo"][4, 17][None].contiguous(), scl.to_device(port.from_int(f, 1)[None]))[0]
    bad = vf.combine_prg(f, B["lo"], seed=b"vf chain coin", counter0=C0, reps=reps)
    with pytest.raises(scl.SclError) as ei:
        vf.check_degree(f, bad, n - t, t)
    assert ei.value.status == scl.ERR_ERROR_DETECTED


@pytest.mark.parametrize("f,reps", CHAINS, ids=["m61-reps2", "secp_scalar-reps1"])
def test_triples_are_verified(env, f, reps):
    """(10, 3), N = 257: deal with scl_prep_triples_shamir_prg; sum rho a b - sum rho c is a degree-2t sharing that opens to 0;
    with delta on all parties' shares of one column of c it opens to a non-zero value"""
    scl, vf, hm, prep, port = env
    n, t, N = 10, 3, 257
    a, b, c = prep.deal_triples_shamir(f, N, t, n, b"vf triples")
    check = lambda: scl.ew(f, O.SUB, vf.combine_prg(f, a, b, seed=b"vf chain coin", counter0=C0, reps=reps).reshape(n * reps, -1),
                           vf.combine_prg(f, c, seed=b"vf chain coin", counter0=C0, reps=reps).reshape(n * reps, -1)).reshape(n, reps, -1)
    assert not vf.check_degree(f, check(), n - 2 * t, 2 * t).any().item()
    delta = scl.to_device(np.repeat(port.from_int(f, 5)[None], n, axis=0))
    c[:, 9] = scl.ew(f, O.ADD, c[:, 9].contiguous(), delta)
    off = host(vf.check_degree(f, check(), n - 2 * t, 2 * t))
    rho = model_coins(port, f, b"vf chain coin", C0, N, reps)
    zero = port.from_int(f, 0)[None]
    for j in range(reps):
        assert off[j].any() and np.array_equal(off[j], port.ew(f, O.SUB, zero, port.ew(f, O.MUL, rho[j, 9][None], port.from_int(f, 5)[None]))[0])


@pytest.mark.parametrize("f,reps", CHAINS, ids=["m61-reps2", "secp_scalar-reps1"])
def test_the_first_chain_captured_into_one_graph(env, f, reps):
    """the launches of chain 1 -- the deal and the two combinations -- on one stream, captured as a linear chain and replayed once
    with every buffer cleared in between; the synchronous detect stays outside.  The result equals the eager result."""
    scl, vf, hm, prep, port = env
    n, t, N = 10, 3, 257
    B = chain_buffers(vf, hm, f, n, t, N, reps)
    chain = lambda: double_chain(scl, vf, hm, f, n, t, N, reps, **B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                   # every kernel has run once before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = {k: host(v).copy() for k, v in B.items() if k.startswith(("lo", "hi", "out"))}
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for v in B.values():
        if v is not None:
            v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, v in first.items():
        assert np.array_equal(host(B[k]), v), k
    assert torch.equal(vf.check_degree(f, B["out_lo"], n - t, t), vf.check_degree(f, B["out_hi"], n - 2 * t, 2 * t))


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_the_header_refuses(env):
    scl, vf, hm, prep, port = env
    x = torch.zeros(3, 8, 1, dtype=torch.int64, device="cuda")
    rho = torch.zeros(5, 8, 1, dtype=torch.int64, device="cuda")
    for reps in (0, 5):
        with pytest.raises(scl.SclError) as ei:
            vf.combine_prg(O.M61, x, seed=SEED, reps=reps)
        assert ei.value.status == scl.ERR_BAD_ARG and "reps" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        vf.combine(O.M61, x, rho)
    assert ei.value.status == scl.ERR_BAD_ARG and "reps" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.Z2K(64), x, seed=SEED)
    assert ei.value.status == scl.ERR_BAD_ARG
    with pytest.raises(scl.SclError) as ei:
        vf.combine(O.M61, x, rho[:2, :7])
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x, x[:2], seed=SEED)
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x, seed=SEED, out=torch.zeros(3, 2, 1, dtype=torch.int64, device="cuda"))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x, seed=SEED, scratch=torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert ei.value.status == scl.ERR_SIZE_MISMATCH and "scratch" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x.expand(3, 8, 1)[:, :, :].as_strided((3, 8, 1), (0, 1, 1)), seed=SEED)       # a row stride of 0 is below N
    assert ei.value.status == scl.ERR_SIZE_MISMATCH and "op_stride < N" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x, seed=SEED, out=x[:, :1])                                                    # out inside x
    assert ei.value.status == scl.ERR_BAD_ARG and "out_dev overlaps x_dev" in str(ei.value)
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x, seed=SEED, counter0=1 << 64)
    assert ei.value.status == scl.ERR_BAD_ARG
    with pytest.raises(scl.SclError) as ei:
        vf.combine_prg(O.M61, x.cpu(), seed=SEED)
    assert ei.value.status == scl.ERR_BAD_ARG


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_the_cxx_round_trip(env):
    """tests/cxx/test_vf_api --gpu: hip::combinePrg and hip::combine over the device containers equal the host form of ss/vf.h
    (which equals vf_combine_one), plain and product, for Mersenne61 (fused, past one trip), Mersenne127 and the secp256k1 order
    (two launches); share -> combinePrg -> shamirRecoverD opens sum rho secret and reports an altered share"""
    import subprocess
    r = subprocess.run([mirror_binary("vf"), "--gpu"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
