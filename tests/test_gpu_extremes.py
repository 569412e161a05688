"""Every accumulating kernel at worst-case operands and term counts.

The kernels sum products unreduced up to hand-derived term counts (F::ACC_TERMS, F::K_TERMS, MatAcc::TERMS), contract i8
digits into int32 (the Mersenne61 matrix-core kernels) and keep words positive with biases.  Uniform operands stay a factor of
about four below those bounds, so the suite's random-data tests cannot see a wrong one.  Here the operands are the pools of
tests/extremes.py -- p - 1, all-ones limbs, the digit-extreme Mersenne61 words X_NEG and X_POS -- and the term counts are
chosen to land on each kernel's flush.  Expected values come from the big-integer model's closed forms (constant operands) or,
for mixed arrays, from the oracle; tests/test_extremes_model.py shows on the CPU that the two agree at these operands.

Each test pins its kernel with the tuning knobs and restores the defaults after it."""
import contextlib

import numpy as np
import pytest

import extremes as X
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEFAULTS = {"max_blocks": 0, "force_scalar": 0, "force_table": 0, "prg_two_pass": 0, "inv_batch": 0, "inv_two_level": 0,
            "gemm_slab_mib": 0, "matmul_lds_min": 0, "mfma": 0, "gf_tiles": 1, "share_waves": 9, "share_waves128": 12}
FIELDS = [(O.M61, None), (O.M127, None)] + [(O.MONT128, p) for p in X.MONT128_PRIMES] + \
    [(O.GF2_128, None), (O.SECP256K1_SCALAR, None), (O.SECP256K1_FIELD, None)]
FIELD_IDS = ["M61", "M127", "Mont128-full", "Mont128-2^127-1", "Mont128-c381", "GF2_128", "secp-order", "secp-field"]
PRIME_FIELDS = [c for c in FIELDS if c[0] != O.GF2_128]
PRIME_IDS = [i for c, i in zip(FIELDS, FIELD_IDS) if c[0] != O.GF2_128]
RINGS = [O.Z2K(k) for k in X.RING_BITS]
BLOCK, RED_UNROLL = 256, 4     # kernels.hpp: workgroup size and packs per trip of k_sum / k_dot


@pytest.fixture(scope="module")
def scl():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    import scl_amd
    return scl_amd


@pytest.fixture(scope="module")
def port():
    return O.Port()


@contextlib.contextmanager
def knobs(scl, **kv):
    for k, v in kv.items():
        scl.set_tuning(k, v)
    try:
        yield
    finally:
        for k in kv:
            scl.set_tuning(k, DEFAULTS[k])


@pytest.fixture
def field(request, scl, port):
    """(model, pool) with the Mont128 modulus of the case on the library and the oracle, 2^128 - 159 again after it"""
    f, p = request.param
    if f == O.MONT128:
        scl.set_mont128_prime(p)
        port.mont128_set_prime(p)
    try:
        yield X.Model(f, p), X.pool(f, p)
    finally:
        if f == O.MONT128:
            scl.set_mont128_prime(X.MONT128_PRIMES[0])
            port.mont128_set_prime(X.MONT128_PRIMES[0])


def const(m, v, *shape):
    return np.ascontiguousarray(np.broadcast_to(m.arr([v])[0], shape + (m.limbs,)))


def ints(a):
    return O.to_ints(a)


def canon(m, vals):
    return [m.canon(v) for v in vals]


def all_equal(m, got, want):
    """every entry of the device result `got` is the raw word `want`"""
    a = got.cpu().numpy().view(np.uint64).reshape(-1, m.limbs) if isinstance(got, torch.Tensor) else np.asarray(got).reshape(-1, m.limbs)
    w = m.arr([want])[0]
    if m.kind == "ring":
        return set(canon(m, ints(np.unique(a, axis=0)))) == {want}
    return bool((a == w).all())


# ------------------------------------------------------------------------------------------------------ 1. element-wise
@pytest.mark.parametrize("field", FIELDS + [(r, None) for r in RINGS], ids=FIELD_IDS + [f"Z2k{k}" for k in X.RING_BITS],
                         indirect=True)
def test_elementwise_pool_cross_product_in_every_lane(scl, field):
    """k_ew* (ADD, SUB, MUL, NEG), k_ew_inv* / k_ew_gf128 (INV, DIV), k_scalar_mul, and the ew_status forms: the pool's full
    cross product, shifted by 0..3 elements so that every pair sits in every lane slot of a pack, against the model"""
    m, vals = field
    f = m.tag
    a = [x for x in vals for _ in vals]
    b = [y for _ in vals for y in vals]
    for shift in range(4):
        A, B = m.arr([vals[0]] * shift + a), m.arr([vals[-1]] * shift + b)
        da, db = scl.to_device(A), scl.to_device(B)
        for op in (O.ADD, O.SUB, O.MUL):
            got = canon(m, ints(scl.to_host(scl.ew(f, op, da, db))))[shift:]
            assert got == [m.op(op, x, y) for x, y in zip(a, b)], (op, shift)
            st = scl.ew_status_buffer()
            got2 = canon(m, ints(scl.to_host(scl.ew_status(f, op, da, db, st))))[shift:]
            assert got2 == got and st.item() == 0
        assert canon(m, ints(scl.to_host(scl.ew(f, O.NEG, da))))[shift:] == [m.neg(x) for x in a]
    nz = [v for v in vals if m.invertible(v)]
    an = [x for x in nz for _ in nz]
    bn = [y for _ in nz for y in nz]
    for shift in range(2):
        dn = scl.to_device(m.arr([nz[0]] * shift + an))
        dd = scl.to_device(m.arr([nz[-1]] * shift + bn))
        for ib in (0, -1):
            with knobs(scl, inv_batch=ib):
                assert canon(m, ints(scl.to_host(scl.ew(f, O.INV, dn))))[shift:] == [m.inv(x) for x in an], (shift, ib)
                assert canon(m, ints(scl.to_host(scl.ew(f, O.DIV, dd, dn))))[shift:] == [m.div(y, x) for x, y in zip(an, bn)]
        st = scl.ew_status_buffer()
        scl.ew_status(f, O.INV, dn, None, st)
        assert st.item() == 0
    if len(nz) < len(vals):   # a zero (an even ring element) among the operands raises the device flag
        st = scl.ew_status_buffer()
        scl.ew_status(f, O.INV, scl.to_device(m.arr(vals)), None, st)
        assert st.item() == 1
    da = scl.to_device(m.arr(vals * 3))
    for s in vals:
        got = canon(m, ints(scl.to_host(scl.scalar_mul(f, da, m.arr([s])[0]))))
        assert got == [m.mul(x, s) for x in vals * 3], s


# ------------------------------------------------------------------------------------------------------------ 2. sum / dot
def test_sum_and_dot_at_each_flush_of_mersenne61(scl):
    """k_sum / k_dot over Mersenne61 (VEC 2, RED_UNROLL 4, flush when terms + 8 > 64): constant p - 1, X_NEG and X_POS vectors
    whose length puts ACC_TERMS - VEC, ACC_TERMS, ACC_TERMS + VEC and 2 ACC_TERMS + 1 terms on a thread, with 1 and 7
    workgroups ("max_blocks")"""
    m = X.Model(O.M61)
    acc = 64
    for blocks in (1, 7):
        G = blocks * BLOCK
        for per_thread in (acc - 2, acc, acc + 2, 2 * acc + 1):
            n = G * per_thread
            for v in (X.M61_P - 1, X.X_NEG, X.X_POS):
                a = scl.to_device(const(m, v, n))
                with knobs(scl, max_blocks=blocks):
                    assert ints(scl.vsum(O.M61, a)) == [m.times(n, v)], (blocks, per_thread, v)
                    assert ints(scl.dot(O.M61, a, a)) == [m.times(n, m.mul(v, v))], (blocks, per_thread, v)


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS, indirect=True)
def test_sum_and_dot_of_maximal_vectors(scl, field):
    """k_sum / k_dot (and k_dot_gf128) at the largest raw word: one length per thread count around a flush with one workgroup,
    and a length whose partials take the second-level k_sum launch (more than 2048 first-stage workgroups)"""
    m, vals = field
    f = m.tag
    top = max(vals) if m.kind != "gf" else X.GF_MASK
    second = [v for v in vals if v != top][-1]
    long_n = 2 * 2048 * BLOCK * RED_UNROLL + 3
    for n, blocks in ((BLOCK * 9, 1), (BLOCK * 7 * 5 + 1, 7), (long_n, 0)):
        for v, w in ((top, top), (top, second)):
            a, b = scl.to_device(const(m, v, n)), scl.to_device(const(m, w, n))
            with knobs(scl, max_blocks=blocks):
                assert ints(scl.vsum(f, a)) == [m.times(n, v)], (n, v)
                assert ints(scl.dot(f, a, b)) == [m.times(n, m.mul(v, w))], (n, v, w)


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS, indirect=True)
def test_sum_and_dot_of_pool_mixtures_against_the_oracle(scl, port, field):
    m, vals = field
    f = m.tag
    a = X.mixed(f, 50_000, 1, m.p if f == O.MONT128 else None)
    b = X.mixed(f, 50_000, 2, m.p if f == O.MONT128 else None)
    A, B = m.arr(a), m.arr(b)
    for blocks in (0, 1, 7):
        with knobs(scl, max_blocks=blocks):
            assert np.array_equal(scl.dot(f, scl.to_device(A), scl.to_device(B)), port.dot(f, A, B))
            assert np.array_equal(scl.vsum(f, scl.to_device(A)), port.sum(f, A))


# ----------------------------------------------------------------------------------------------------------- 3. reconstruct
RECOVER_M = {O.M61: [1, 2, 7, 8, 15, 16] + list(range(56, 73)) + [129, 256, 300],
             O.M127: [1, 8, 16, 17, 63, 64, 65, 128, 129, 200],
             O.MONT128: [2, 5, 16, 17, 64, 128, 129], O.SECP256K1_SCALAR: [2, 5, 16, 17, 64, 65],
             O.SECP256K1_FIELD: [2, 5, 16, 17, 64, 65]}


@pytest.mark.parametrize("field", PRIME_FIELDS, ids=PRIME_IDS, indirect=True)
def test_recover_at_the_flush_with_maximal_shares_and_lambdas(scl, field):
    """k_recover_fixed (Mersenne fields, m <= 16), k_recover_table (larger m, and any m under "force_table": flush at terms + 8
    and terms + 1) at m from ACC_TERMS - 8 to ACC_TERMS + 8, 2 ACC_TERMS + 1 and beyond one lambda table (the `prev` chaining),
    each also at one element per lane ("force_scalar" forces vector width 1): every share and every lambda at the largest raw
    word.  Then the default Lagrange basis, whose small signed integers take k_recover_small for the Montgomery fields."""
    m, vals = field
    f = m.tag
    N = 515
    top = max(vals)
    for mm in RECOVER_M[f]:
        shares = scl.to_device(const(m, top, mm, N))
        lam = m.arr([top] * mm)
        want = m.const_recover(top, [top] * mm)
        for kv in ({}, {"force_scalar": 1}, {"force_table": 1}):
            with knobs(scl, **kv):
                assert all_equal(m, scl.shamir_recover(f, shares, lam), want), (mm, kv)
        if mm <= 64:   # the default basis (small signed integers for the Montgomery fields)
            lam0 = scl.lagrange_basis(f, mm)
            want0 = m.const_recover(top, ints(lam0))
            for kv in ({}, {"force_table": 1}):
                with knobs(scl, **kv):
                    assert all_equal(m, scl.shamir_recover(f, shares, lam0), want0), (mm, kv)


@pytest.mark.parametrize("field", PRIME_FIELDS, ids=PRIME_IDS, indirect=True)
def test_recover_of_pool_mixtures_against_the_oracle(scl, port, field):
    m, vals = field
    f = m.tag
    N = 130
    for mm in (5, 16, 17, 64, 65):
        sh = m.arr(X.mixed(f, mm * N, mm, m.p if f == O.MONT128 else None)).reshape(mm, N, m.limbs)
        lam = m.arr(X.mixed(f, mm, mm + 100, m.p if f == O.MONT128 else None))
        want = port.shamir_recover_lambda(f, np.ascontiguousarray(np.transpose(sh, (1, 0, 2))), lam)
        for kv in ({}, {"force_scalar": 1}, {"force_table": 1}):
            with knobs(scl, **kv):
                assert np.array_equal(scl.to_host(scl.shamir_recover(f, scl.to_device(sh), lam)), want), (mm, kv)


def test_recover_gf128_all_ones(scl):
    """k_recover_gf128_pos (position tables) and k_recover_gf128 ("force_table" 3) with all-ones shares and lambdas"""
    m = X.Model(O.GF2_128)
    N = 1000
    for mm in (5, 64, 65, 130):
        shares = scl.to_device(const(m, X.GF_MASK, mm, N))
        lam = m.arr([X.GF_MASK] * mm)
        want = m.const_recover(X.GF_MASK, [X.GF_MASK] * mm)
        for ft in (0, 3):
            with knobs(scl, force_table=ft):
                assert all_equal(m, scl.shamir_recover(O.GF2_128, shares, lam), want), (mm, ft)


@pytest.mark.parametrize("field", FIELDS + [(r, None) for r in RINGS], ids=FIELD_IDS + [f"Z2k{k}" for k in X.RING_BITS],
                         indirect=True)
def test_additive_recover_at_the_flush(scl, field):
    """k_additive_recover (flush at terms + 4 > ACC_TERMS): n parties of maximal shares around 64, and 129"""
    m, vals = field
    f = m.tag
    top = max(vals) if m.kind != "gf" else X.GF_MASK
    for n in (1, 4, 59, 60, 61, 63, 64, 65, 67, 68, 129):
        got = scl.additive_recover(f, scl.to_device(const(m, top, n, 333)))
        assert all_equal(m, got, m.times(n, top)), n


# ------------------------------------------------------------------------------------------------------------ 4. sharing
SHARE_NT = [(2, 1), (5, 2), (9, 4), (17, 7), (17, 8), (55, 5), (64, 15), (17, 16), (33, 16), (64, 17), (128, 31), (100, 48),
            (100, 49), (120, 63), (200, 100), (812, 3), (812, 16)]


@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS, indirect=True)
def test_share_with_maximal_secrets_and_coefficients(scl, field):
    """every share kernel the dispatcher picks -- k_share (Horner), k_share_small / _t / _pair, k_share_blocked (G = 4, 6, 8),
    k_share_vdm, k_share_chunk (t > 48), k_share_gf_tiles / k_share_gf_nodes, the matrix-core share -- with every secret and
    every coefficient at the largest raw word: the shares are the geometric sum of the node's powers times that word.  Node
    counts whose powers approach 2^29 (17^7, 55^5, 812^3) reach the small-node accumulators' bounds at the full-width moduli."""
    m, vals = field
    f = m.tag
    top = max(vals) if m.kind != "gf" else X.GF_MASK
    N = 300
    for n, t in SHARE_NT:
        if m.limbs == 4 and n > 128 and t > 3:
            continue
        secrets = scl.to_device(const(m, top, N))
        coeffs = scl.to_device(const(m, top, t, N))
        nodes = [m.from_int(i + 1) for i in range(n)]
        want = [m.const_share(top, t, x) for x in nodes]
        modes = [{}, {"force_table": 1}, {"share_waves": 0, "share_waves128": 0}]   # (the last: k_share_small at t <= 7)
        if f == O.M61:
            modes += [{"mfma": 1}, {"mfma": -1}]
        if f == O.GF2_128:
            modes += [{"gf_tiles": 0}]
        for kv in modes:
            with knobs(scl, **kv):
                got = scl.to_host(scl.shamir_share(f, secrets, coeffs, n))
            for i in sorted({0, 1, n // 2, n - 1}):
                assert all_equal(m, got[i], want[i]), (n, t, kv, i)
            assert np.array_equal(got[:, 0], got[:, N - 1])
            rows = canon(m, ints(got[:, 0]))
            assert rows == want, (n, t, kv)
        if n <= 128 and t <= 48:   # full-width nodes: p - 1 - i
            xs = [(m.p - 1 - i) if m.p else X.GF_MASK ^ i for i in range(n)]
            got = scl.to_host(scl.shamir_share(f, secrets, coeffs, n, alphas=m.arr(xs)))
            assert canon(m, ints(got[:, 0])) == [m.const_share(top, t, x) for x in xs], (n, t)


# ----------------------------------------------------------------------------------------------------- 5. matrix cores (M61)
def _digit_extreme_pairs():
    return ((X.X_NEG, X.X_NEG), (X.X_NEG, X.X_POS), (X.X_POS, X.X_POS), (X.M61_P - 1, X.X_NEG))


def _alternating_product(scl, m, M, K, N, a0, a1, b):
    """A's rows alternate a0 / a1, B constant b: row i of the product is K * a_i * b everywhere"""
    A = np.empty((M, K, 1), dtype=np.uint64)
    A[0::2] = a0
    A[1::2] = a1
    return scl.to_device(A), scl.to_device(const(m, b, K, N)), [m.const_matmul(K, a0 if i % 2 == 0 else a1, b) for i in range(M)]


@pytest.mark.parametrize("M,K,N", [(128, 64, 4096), (64, 64, 4096), (100, 43, 5000), (16, 64, 4500), (128, 64, 300)])
def test_matrix_core_share_kernels_at_digit_extremes(scl, M, K, N):
    """the small-left-factor matrix-core products (p16, pipe<1>, k_share_mfma_m61 -- "mfma" 1): X_NEG times X_NEG gives the
    largest positive digit contraction E_d, X_NEG times X_POS the largest negative one; and rows alternating X_NEG / X_POS"""
    m = X.Model(O.M61)
    for a, b in _digit_extreme_pairs():
        with knobs(scl, mfma=1):
            got = scl.matmul(O.M61, scl.to_device(const(m, a, M, K)), scl.to_device(const(m, b, K, N)))
        assert all_equal(m, got, m.const_matmul(K, a, b)), (M, K, N, hex(a), hex(b))
    dA, dB, rows = _alternating_product(scl, m, M, K, N, X.X_NEG, X.X_POS, X.X_NEG)
    with knobs(scl, mfma=1):
        got = scl.to_host(scl.matmul(O.M61, dA, dB))
    assert [ints(got[i, :1])[0] for i in range(M)] == rows and (got == got[:, :1]).all()


@pytest.mark.parametrize("K", [8191, 8192, 8193, 16384, 32769])
def test_general_gemm_across_the_super_step(scl, K):
    """the general matrix-core GEMM (k_gemm_mfma_m61, "mfma" 1) in ONE k-slice: a 1024 x 1024 product is 256 workgroups, so
    gemm_mfma_slab (capi.hip) does not split K and every wave runs the whole inner dimension through its super-steps of
    GEMM_SUPER = 256 k-steps (8192 columns).  |E_d| reaches about 6 * 2^14 per column with digit-extreme factors (X_NEG x X_NEG
    the largest positive, X_NEG x X_POS the largest negative), so K across 8192 and up to 32769: a super-step of 32768 columns
    would wrap the int32 diagonals.  Then rows alternating X_POS / X_NEG at the longest K."""
    m = X.Model(O.M61)
    M = N = 1024
    for a, b in ((X.X_NEG, X.X_NEG), (X.X_NEG, X.X_POS)):
        dA, dB = scl.to_device(const(m, a, M, K)), scl.to_device(const(m, b, K, N))
        with knobs(scl, mfma=1):
            assert all_equal(m, scl.matmul(O.M61, dA, dB), m.const_matmul(K, a, b)), (K, hex(a), hex(b))
        del dA, dB
    if K == 32769:
        dA, dB, rows = _alternating_product(scl, m, M, K, N, X.X_POS, X.X_NEG, X.X_NEG)
        with knobs(scl, mfma=1):
            got = scl.to_host(scl.matmul(O.M61, dA, dB))
        assert [ints(got[i, :1])[0] for i in range(M)] == rows and (got == got[:, :1]).all()


@pytest.mark.parametrize("K", [8191, 8193, 32769])
def test_general_gemm_split_k_slabs_and_chunks(scl, K):
    """the general matrix-core GEMM on a few output tiles (64 x 96: K split into slices of at least 16 k-steps, the slices'
    partial products summed by k_additive_recover), slab by slab ("gemm_slab_mib" 1), and the (row block, k-chunk) form on the
    sharing kernels ("mfma" 2), with digit-extreme factors"""
    m = X.Model(O.M61)
    M, N = 64, 96
    for a, b in _digit_extreme_pairs():
        dA, dB = scl.to_device(const(m, a, M, K)), scl.to_device(const(m, b, K, N))
        want = m.const_matmul(K, a, b)
        for kv in ({"mfma": 1}, {"mfma": 1, "gemm_slab_mib": 1}, {"mfma": 2}):
            if K > 8193 and kv.get("mfma") == 2 and a != b:
                continue
            with knobs(scl, **kv):
                assert all_equal(m, scl.matmul(O.M61, dA, dB), want), (K, hex(a), hex(b), kv)


def test_detect_on_matrix_cores_with_digit_extreme_shares(scl, port):
    """shamirRecoverD over Mersenne61 on the matrix cores at the shapes of test_recover_detect_on_matrix_cores: constant
    polynomials X_NEG / X_POS / p - 1 (every share digit-extreme, every check must pass), then one share per corrupted secret"""
    m = X.Model(O.M61)
    for t, d, extra, N in ((42, 42, 0, 5000), (23, 23, 1, 4100), (30, 20, 3, 4500), (63, 63, 0, 4200), (10, 60, 0, 4097)):
        mm = d + t + extra
        secrets = np.array([(X.X_NEG, X.X_POS, X.M61_P - 1)[s % 3] for s in range(N)], dtype=np.uint64)
        shares = np.ascontiguousarray(np.broadcast_to(secrets[None, :, None], (mm, N, 1)))
        bad = np.arange(0, N, 7)
        corrupt = shares.copy()
        corrupt[d + 1 if d + 1 < d + t else 0, bad] = X.X_POS ^ 1
        nodes = m.arr([i + 1 for i in range(mm)])
        res = {}
        for mode in (1, -1):
            with knobs(scl, mfma=mode):
                out, st, nb = scl.shamir_recover_detect(O.M61, scl.to_device(shares), t, d=d, alphas=nodes, x=m.arr([0])[0])
                assert nb == 0 and not st.cpu().numpy().any() and np.array_equal(scl.to_host(out)[:, 0], secrets), (t, d, mode)
                res[mode] = scl.shamir_recover_detect(O.M61, scl.to_device(corrupt), t, d=d, alphas=nodes, x=m.arr([0])[0])
        (o1, s1, b1), (o0, s0, b0) = res[1], res[-1]
        assert b1 == b0 == len(bad) and np.array_equal(s1.cpu().numpy(), s0.cpu().numpy())
        assert np.array_equal(np.flatnonzero(s1.cpu().numpy()), bad)
        assert np.array_equal(scl.to_host(o1), scl.to_host(o0))


# ------------------------------------------------------------------------------------------------------ 6. vector-ALU matmul
@pytest.mark.parametrize("field", FIELDS + [(r, None) for r in RINGS], ids=FIELD_IDS + [f"Z2k{k}" for k in X.RING_BITS],
                         indirect=True)
def test_valu_matmul_paths_at_the_maximum(scl, field):
    """k_matvec (N = 1), k_matmul_thin (K <= 16), k_matmul (left factor in LDS: MatAcc::TERMS flush), k_matmul_tiled and its
    split over K -- "mfma" -1 keeps Mersenne61 off the matrix cores -- with both factors at the largest raw word"""
    m, vals = field
    f = m.tag
    top = max(vals) if m.kind != "gf" else X.GF_MASK
    second = sorted(vals)[-2]
    Ks = [63, 64, 65, 129, 200] if f == O.M61 else [16, 65, 257]
    cases = [(33, K, 1, {}) for K in Ks]                                          # k_matvec
    cases += [(8, 16 if m.limbs < 4 else 8, 600, {"matmul_lds_min": 1})]        # k_matmul_thin
    cases += [(M, K, 700, {"matmul_lds_min": 1}) for K in Ks for M in (5,) if M * K * 8 * m.limbs <= 48 * 1024]   # k_matmul
    cases += [(40, K, 300, {}) for K in Ks]                                       # k_matmul_tiled
    cases += [(9, 4096 if m.limbs == 1 else 2048, 17, {})]                        # split over K
    if f != O.M61:
        cases += [(2, 1 << 16, 3, {})]                                            # the longest K in the budget
    for M, K, N, kv in cases:
        for a, b in ((top, top), (top, second)):
            dA, dB = scl.to_device(const(m, a, M, K)), scl.to_device(const(m, b, K, N))
            with knobs(scl, mfma=-1, **kv):
                assert all_equal(m, scl.matmul(f, dA, dB), m.const_matmul(K, a, b)), (M, K, N, kv, a, b)


def test_k_matmul_flush_with_digit_extreme_m61(scl):
    """k_matmul over Mersenne61 at the K that puts MatAcc<M61>::TERMS = 64 products and one more in a u128: 64 products of p - 1
    fit, 128 would not"""
    m = X.Model(O.M61)
    for K in (64, 65, 127, 128, 129, 192, 1000):
        for a, b in ((X.M61_P - 1, X.M61_P - 1), (X.M61_P - 1, X.M61_P - 2)):
            dA, dB = scl.to_device(const(m, a, 6, K)), scl.to_device(const(m, b, K, 4096))
            with knobs(scl, mfma=-1, matmul_lds_min=1):
                assert all_equal(m, scl.matmul(O.M61, dA, dB), m.const_matmul(K, a, b)), K


# ------------------------------------------------------------------------------------------------------ 7. detect and correct
@pytest.mark.parametrize("f,kt", [(O.M61, 1024), (O.M127, 256)])
def test_recover_detect_at_k_terms(scl, f, kt):
    """k_recover_detect sums each check row over the d + 1 interpolating shares (rows_times_shares, flush when
    terms + 1 > F::K_TERMS).  Here d + 1 = K_TERMS and K_TERMS + 1, t = 2 (one check row, m = d + 2 shares), every share at
    p - 1 (a constant polynomial: the check passes); then the checked share changed in every third secret"""
    m = X.Model(f)
    N, t = 700, 2
    for d1 in (kt, kt + 1):
        d = d1 - 1
        n = d + t
        shares = const(m, m.p - 1, n, N)
        nodes = m.arr([i + 1 for i in range(n)])
        with knobs(scl, mfma=-1):
            out, st, nb = scl.shamir_recover_detect(f, scl.to_device(shares), t, d=d, alphas=nodes, x=m.arr([0])[0])
            assert nb == 0 and not st.cpu().numpy().any() and all_equal(m, out, m.p - 1), d1
            bad = shares.copy()
            bad[d + 1, ::3] = m.arr([m.p - 2])[0]
            out, st, nb = scl.shamir_recover_detect(f, scl.to_device(bad), t, d=d, alphas=nodes, x=m.arr([0])[0])
            assert nb == len(range(0, N, 3)) and np.array_equal(np.flatnonzero(st.cpu().numpy()), np.arange(0, N, 3)), d1


@pytest.mark.parametrize("field", PRIME_FIELDS, ids=PRIME_IDS, indirect=True)
def test_berlekamp_welch_with_maximal_residues(scl, port, field):
    """k_bw_consistent / k_bw_solve at small n: constant polynomials at the largest raw word, one corrupted share (corrected),
    against the oracle's shamirRecoverC"""
    m, vals = field
    f = m.tag
    top = max(vals)
    for t in (1, 2, 4):
        n, N = 3 * t + 1, 40
        aos = const(m, top, N, n).copy()
        aos[::2, 0] = m.arr([vals[1]])[0]
        res = scl.shamir_recover_correct(f, scl.to_device(np.ascontiguousarray(np.transpose(aos, (1, 0, 2)))))
        f_, e_, st, nerr = port.shamir_recover_c(f, aos)
        assert np.array_equal(res["status"].cpu().numpy(), st)
        assert all_equal(m, res["f"][0], top) and np.array_equal(scl.to_host(res["f"]), np.transpose(f_, (1, 0, 2)))


# ------------------------------------------------------------------------------------------------------------------ 8. rings
@pytest.mark.parametrize("K", X.RING_BITS)
def test_rings_at_all_ones(scl, port, K):
    """Z2k<K>: k_sum / k_dot, the matmul kernels, additive share (explicit randomness) and k_additive_recover with every word
    at 2^K - 1, and pool mixtures against the oracle"""
    f = O.Z2K(K)
    m = X.Model(f)
    top = (1 << K) - 1
    for n in (BLOCK * 9, 2 * 2048 * BLOCK * RED_UNROLL + 1):
        a = scl.to_device(const(m, top, n))
        assert m.canon(ints(scl.vsum(f, a))[0]) == m.times(n, top)
        assert m.canon(ints(scl.dot(f, a, a))[0]) == m.times(n, m.mul(top, top))
    for M, Kk, N in ((33, 200, 1), (8, 16, 600), (40, 129, 300), (9, 4096, 17)):
        got = scl.matmul(f, scl.to_device(const(m, top, M, Kk)), scl.to_device(const(m, top, Kk, N)))
        assert all_equal(m, got, m.const_matmul(Kk, top, top)), (M, Kk, N)
    N = 333
    for n in (2, 64, 65):
        sec = scl.to_device(const(m, top, N))
        rnd = scl.to_device(const(m, top, n - 1, N))
        sh = scl.additive_share(f, sec, rnd, n)
        assert all_equal(m, scl.additive_recover(f, sh), top), n
    mix = m.arr(X.mixed(f, 4099, K))
    mix2 = m.arr(X.mixed(f, 4099, K + 1))
    assert np.array_equal(scl.dot(f, scl.to_device(mix), scl.to_device(mix2)), port.dot(f, mix, mix2))
    assert np.array_equal(scl.vsum(f, scl.to_device(mix)), port.sum(f, mix))
