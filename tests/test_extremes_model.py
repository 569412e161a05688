"""The CPU checker is right at the extremes: the oracle (oracle_lib.Port) against the big-integer model of tests/extremes.py
on every pool of extreme operands -- all pairs of the element-wise operations, sums and dot products of constant vectors,
polynomial evaluation, reconstruct with given coefficients and matrix products at small K.  The GPU tests of
tests/test_gpu_extremes.py trust either of the two; here both are shown to agree where the kernels' bounds are tight."""
import numpy as np
import pytest

import extremes as X
import oracle_lib as O

FIELDS = [(O.M61, None), (O.M127, None)] + [(O.MONT128, p) for p in X.MONT128_PRIMES] + \
    [(O.GF2_128, None), (O.SECP256K1_SCALAR, None), (O.SECP256K1_FIELD, None)] + [(O.Z2K(k), None) for k in X.RING_BITS]
IDS = [f"{f:#x}-{p:x}" if p else f"{f:#x}" for f, p in FIELDS]


@pytest.fixture(scope="module")
def port():
    return O.Port()


@pytest.fixture
def field(request, port):
    """(model, pool) with the oracle's Mont128 modulus set for the case and 2^128 - 159 again after it"""
    f, p = request.param
    if f == O.MONT128:
        port.mont128_set_prime(p)
    try:
        yield X.Model(f, p), X.pool(f, p)
    finally:
        if f == O.MONT128:
            port.mont128_set_prime(X.MONT128_PRIMES[0])


def _canon(m, vals):
    return [m.canon(v) for v in vals]


def test_pools_hold_what_the_bounds_need():
    assert X.X_NEG in X.pool(O.M61) and X.X_POS in X.pool(O.M61) and X.M61_P - 1 in X.pool(O.M61)
    assert any(a + b == X.M61_P for a in X.pool(O.M61) for b in X.pool(O.M61))
    # digits of the matrix-core recoding: seven signed 8-bit digits (carry into the next) and a top digit
    def digits(x):
        d = []
        for _ in range(7):
            lo = x & 0xFF
            s = lo - 256 if lo >= 128 else lo
            d.append(s)
            x = (x - s) >> 8
        return d + [x]
    assert digits(X.X_NEG) == [-128] * 7 + [1] and digits(X.X_POS) == [127] * 7 + [31]
    assert digits(X.M61_P - 1) == [-2, 0, 0, 0, 0, 0, 0, 32]
    for f, p in FIELDS:
        m, vals = X.Model(f, p), X.pool(f, p)
        assert all(0 <= v < (m.p if m.p else 1 << 128) for v in vals), (f, p)
        assert len(set(vals)) == len(vals) >= (2 if f == O.Z2K(1) else 5)


@pytest.mark.parametrize("field", FIELDS, ids=IDS, indirect=True)
def test_elementwise_all_pairs(port, field):
    m, vals = field
    f = m.tag
    a = [x for x in vals for _ in vals]
    b = [y for _ in vals for y in vals]
    A, B = m.arr(a), m.arr(b)
    for op in (O.ADD, O.SUB, O.MUL):
        got = _canon(m, O.to_ints(port.ew(f, op, A, B)))
        assert got == [m.op(op, x, y) for x, y in zip(a, b)], op
    assert _canon(m, O.to_ints(port.ew(f, O.NEG, m.arr(vals)))) == [m.neg(x) for x in vals]
    nz = [v for v in vals if m.invertible(v)]
    assert _canon(m, O.to_ints(port.ew(f, O.INV, m.arr(nz)))) == [m.inv(x) for x in nz]
    a = [x for x in vals for _ in nz]
    b = [y for _ in vals for y in nz]
    assert _canon(m, O.to_ints(port.ew(f, O.DIV, m.arr(a), m.arr(b)))) == [m.div(x, y) for x, y in zip(a, b)]


@pytest.mark.parametrize("field", FIELDS, ids=IDS, indirect=True)
def test_dot_and_sum_of_constant_vectors(port, field):
    m, vals = field
    f = m.tag
    for v in vals:
        for n in (1, 64, 65, 1025):
            a = m.arr([v] * n)
            assert m.canon(O.to_ints(port.sum(f, a))[0]) == m.times(n, v), (v, n)
            assert m.canon(O.to_ints(port.dot(f, a, a))[0]) == m.times(n, m.mul(v, v)), (v, n)
    mix = X.mixed(f, 500, 7, m.p if f == O.MONT128 else None)
    mix2 = X.mixed(f, 500, 8, m.p if f == O.MONT128 else None)
    assert m.canon(O.to_ints(port.dot(f, m.arr(mix), m.arr(mix2)))[0]) == m.dot(mix, mix2)
    assert m.canon(O.to_ints(port.sum(f, m.arr(mix)))[0]) == m.vsum(mix)


@pytest.mark.parametrize("field", [c for c in FIELDS if not O.is_ring(c[0])],
                         ids=[i for c, i in zip(FIELDS, IDS) if not O.is_ring(c[0])], indirect=True)
def test_poly_eval_and_recover_lambda(port, field):
    m, vals = field
    f = m.tag
    for t in (1, 3, 8):
        for c in vals:
            coeffs = m.arr([c] * (t + 1))
            got = _canon(m, O.to_ints(port.poly_eval(f, coeffs, m.arr(vals))))
            assert got == [m.const_share(c, t, x) for x in vals], (c, t)
    # reconstruct: identical shares and a constant lambda row, then the pool in every slot
    for n in (1, 5, 17):
        for s in vals:
            lam = [vals[-1]] * n
            sh = m.arr([s] * n).reshape(1, n, m.limbs)
            got = O.to_ints(port.shamir_recover_lambda(f, sh, m.arr(lam)))[0]
            assert got == m.const_recover(s, lam), (s, n)
    n = len(vals)
    lam = list(reversed(vals))
    shares = [[vals[(i + j) % n] for i in range(n)] for j in range(n)]
    got = O.to_ints(port.shamir_recover_lambda(f, m.arr([x for r in shares for x in r]).reshape(n, n, m.limbs), m.arr(lam)))
    assert got == [m.dot(r, lam) for r in shares]


@pytest.mark.parametrize("field", FIELDS, ids=IDS, indirect=True)
def test_matmul_at_small_k(port, field):
    m, vals = field
    f = m.tag
    for K in (1, 7, 64, 65):
        for a, b in ((vals[-1], vals[-1]), (vals[2 % len(vals)], vals[-1]), (vals[-2], vals[1])):
            A = m.arr([a] * (3 * K)).reshape(3, K, m.limbs)
            B = m.arr([b] * (K * 2)).reshape(K, 2, m.limbs)
            got = _canon(m, O.to_ints(port.matmul(f, A, B)))
            assert got == [m.const_matmul(K, a, b)] * 6, (K, a, b)
    n = len(vals)
    Av = [vals[(i * 3 + k) % n] for i in range(4) for k in range(n)]
    Bv = [vals[(k + 5 * j) % n] for k in range(n) for j in range(3)]
    got = _canon(m, O.to_ints(port.matmul(f, m.arr(Av).reshape(4, n, m.limbs), m.arr(Bv).reshape(n, 3, m.limbs))))
    want = [m.dot(Av[i * n:(i + 1) * n], [Bv[k * 3 + j] for k in range(n)]) for i in range(4) for j in range(3)]
    assert got == want
