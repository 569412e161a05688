"""Extreme operands and a big-integer model of every field and ring (TEST INFRASTRUCTURE, not a conftest).

Most kernels sum products unreduced up to a hand-derived term count, trust an i8 digit contraction to fit an int32, or
bias a word to keep it positive.  Uniform random operands sit far below those bounds (a product of two uniform residues
averages a quarter of the largest one), so a bound that is wrong by a factor of up to about four passes every test that
draws uniform data.  The pools below hold the operands that reach the bounds: the largest raw words, the digit-extreme
Mersenne61 words of the matrix-core recoding, words with all-ones limbs, pairs that sum to exactly p.

Elements are RAW words -- what the ABI takes: for the Montgomery fields (Mont128, secp256k1 order and field) the
residue x R mod p, not x.  The model below works on raw words too:

  Montgomery   mul(a, b) = a b R^-1 mod p,  inv(a) = R^2 a^-1 mod p,  add / sub / neg mod p
  Mersenne     plain arithmetic mod p
  GF(2^128)    a shift-xor multiplier, x^128 = x^7 + x^2 + x + 1
  Z2k          integers mod 2^K

and gives closed forms for constant operands (a K-term product of constants, a reconstruct of identical shares, a share
of constant coefficients), with which a kernel's output of millions of entries is checked against exact arithmetic
without an oracle call."""
from __future__ import annotations

import numpy as np

import oracle_lib as O

M61_P = (1 << 61) - 1
M127_P = (1 << 127) - 1
# digit-extreme Mersenne61 words of the matrix-core recoding (share_mfma.hpp, mf_recode): seven signed 8-bit digits and a
# top digit.  X_NEG = [-128 x 7, 1] and X_POS = [127 x 7, 31]; both are canonical.  p - 1 recodes to [-2, 0 x 6, 32].
X_NEG = 0x007F7F7F7F7F7F80
X_POS = 0x1F7F7F7F7F7F7F7F

MONT128_PRIMES = ((1 << 128) - 159,              # full width: the small-node Barrett path
                  (1 << 127) - 1,                # not full width
                  0xc381e88f38c0c8fd8712b8bc076f3787)   # the third fixture modulus (tests/golden/golden_mont128.json)
SECP_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SECP_FIELD = (1 << 256) - (1 << 32) - 977
RING_BITS = (1, 61, 63, 64, 65, 127, 128)

GF_MASK = (1 << 128) - 1


def gf_mul(a: int, b: int) -> int:
    """bit-serial: for each set bit of b add a * x^i, a * x reduced by x^128 = x^7 + x^2 + x + 1 (0x87)"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a >> 128:
            a = (a & GF_MASK) ^ 0x87
    return r


def refl(v: int) -> int:
    """a 128-bit block with its bits reversed: between GCM's blocks (bit 0 first) and this field's integers"""
    return int(format(v, "0128b")[::-1], 2)


def spec_mul(X: int, Y: int) -> int:
    """the multiplication of the GCM specification as it is written there (Algorithm 1: right shifts, R = e1 || 0^120) on
    blocks as big-endian integers"""
    Z, V = 0, X
    for i in range(128):
        if (Y >> (127 - i)) & 1:
            Z ^= V
        V = (V >> 1) ^ (0xe1 << 120) if V & 1 else V >> 1
    return Z


def gf_inv(a: int) -> int:
    """a^(2^128 - 2) by square-and-multiply on the bit-serial multiplier"""
    r, e, base = 1, (1 << 128) - 2, a
    while e:
        if e & 1:
            r = gf_mul(r, base)
        base = gf_mul(base, base)
        e >>= 1
    return r


def _dedup(vals):
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


class Model:
    """the arithmetic of one field or ring on raw words (Python ints); `modulus` is p (Mont128: the one it is built with)"""

    def __init__(self, tag: int, modulus: int | None = None):
        self.tag = tag
        self.limbs = O.LIMBS[tag]
        if O.is_ring(tag):
            self.kind, self.bits = "ring", tag - 0x100
            self.p = 1 << self.bits
        elif tag == O.GF2_128:
            self.kind, self.p = "gf", None
        elif tag in (O.M61, O.M127):
            self.kind, self.p = "plain", O.P[tag]
        else:
            self.kind = "mont"
            self.p = modulus if modulus is not None else {O.MONT128: MONT128_PRIMES[0], O.SECP256K1_SCALAR: SECP_ORDER,
                                                           O.SECP256K1_FIELD: SECP_FIELD}[tag]
            self.R = 1 << (64 * self.limbs)
            self.Rinv = pow(self.R, -1, self.p)

    # ---- element operations on raw words
    def add(self, a, b):
        return a ^ b if self.kind == "gf" else (a + b) % self.p

    def sub(self, a, b):
        return a ^ b if self.kind == "gf" else (a - b) % self.p

    def neg(self, a):
        return a if self.kind == "gf" else (-a) % self.p

    def mul(self, a, b):
        if self.kind == "gf":
            return gf_mul(a, b)
        if self.kind == "mont":
            return a * b * self.Rinv % self.p
        return a * b % self.p

    def invertible(self, a) -> bool:
        return a % 2 == 1 if self.kind == "ring" else a != 0

    def inv(self, a):
        assert self.invertible(a)
        if self.kind == "gf":
            return gf_inv(a)
        if self.kind == "mont":
            return self.R * self.R * pow(a, -1, self.p) % self.p
        return pow(a, -1, self.p)

    def div(self, a, b):
        return self.mul(a, self.inv(b))

    def op(self, op, a, b=None):
        return {O.ADD: self.add, O.SUB: self.sub, O.MUL: self.mul, O.DIV: self.div}[op](a, b) if b is not None else \
            {O.NEG: self.neg, O.INV: self.inv}[op](a)

    def from_int(self, v: int):
        """raw word of the integer v (the field's from_u64; GF(2^128): the polynomial with v's bits)"""
        if self.kind == "gf":
            return v
        if self.kind == "mont":
            return v * self.R % self.p
        return v % self.p

    def canon(self, a):
        """the value a raw word stands for, as the arithmetic sees it (Z2k: bits above K do not count)"""
        return a % self.p if self.kind == "ring" else a

    # ---- closed forms
    def times(self, k: int, a):
        """a + a + ... (k terms)"""
        if self.kind == "gf":
            return a if k % 2 else 0
        return k * a % self.p

    def dot(self, a, b):
        s = 0
        for x, y in zip(a, b):
            s = self.add(s, self.mul(x, y))
        return s

    def vsum(self, a):
        s = 0
        for x in a:
            s = self.add(s, x)
        return s

    def const_matmul(self, K: int, a, b):
        """every entry of (M x K of a) times (K x N of b)"""
        return self.times(K, self.mul(a, b))

    def const_recover(self, share, lam):
        """sum_i lam_i * share for identical shares"""
        return self.mul(share, self.vsum(lam))

    def power(self, x, e: int):
        r = self.from_int(1)
        for _ in range(e):
            r = self.mul(r, x)
        return r

    def const_share(self, c, t: int, node):
        """c + c x + ... + c x^t at the node x (raw word): a polynomial whose t + 1 coefficients are all c"""
        g, xp = 0, self.from_int(1)
        for _ in range(t + 1):
            g = self.add(g, xp)
            xp = self.mul(xp, node)
        return self.mul(c, g)

    # ---- numpy bridge
    def arr(self, vals):
        return O.from_ints([int(v) for v in vals], self.limbs)

    def ints(self, a):
        return O.to_ints(a)


def pool(tag: int, modulus: int | None = None) -> list[int]:
    """the extreme raw words of a field or ring (canonical: every one is a valid element); Mont128 at `modulus`"""
    if O.is_ring(tag):
        K = tag - 0x100
        return _dedup([0, 1, (1 << K) - 1, 1 << (K - 1), (1 << (K - 1)) - 1])
    if tag == O.GF2_128:
        top = [GF_MASK ^ ((1 << k) - 1) for k in (64, 96, 120, 127)]       # top-heavy masks: the high bits all set
        return _dedup([0, 1, 1 << 127, GF_MASK, (1 << 127) | 1, 0x87, GF_MASK ^ 1, 0xFF << 120] + top)
    if tag == O.M61:
        p = M61_P
        return _dedup([0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 32) - 1, (1 << 32) + 1, X_NEG, X_POS,
                       1 << 60, p - (1 << 60), X_NEG, p - X_NEG, X_POS, p - X_POS, 12345, p - 12345])
    if tag == O.M127:
        p = M127_P
        m61 = [v for v in pool(O.M61)]
        return _dedup(m61 + [p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 64) - 1, 1 << 64, 1 << 96, 1 << 126,
                             p - (1 << 126), p - ((1 << 64) - 1), (1 << 127) - (1 << 64)])
    m = Model(tag, modulus)
    p, R = m.p, m.R
    vals = [0, 1, p - 1, p - 2, R % p, (-R) % p, (1 << 64) - 1, 1 << 64, ((p >> 64) - 1) << 64 | ((1 << 64) - 1)]
    if tag in (O.SECP256K1_SCALAR, O.SECP256K1_FIELD):
        # as many all-ones limbs at the top as the modulus allows, below p: the field's top three limbs are all ones; the
        # order's third limb is FF..FE, so its word keeps the top two limbs of p and zero below
        vals += [((1 << 192) - 1) << 64, (((1 << 192) - 1) << 64) | 0xFFFFFFFE] if tag == O.SECP256K1_FIELD else \
            [(p >> 128) << 128, ((p >> 64) << 64) - 1]
        vals += [(1 << 128) - 1, 1 << 128, (1 << 192) - 1]
    return _dedup([v for v in vals if 0 <= v < p])


def nonzero(tag, vals):
    m = Model(tag)
    return [v for v in vals if m.invertible(v)]


def mixed(tag: int, n: int, seed: int, modulus: int | None = None) -> list[int]:
    """n raw words drawn from the pool (every pool value at least once where n allows), in a seeded order"""
    vals = pool(tag, modulus)
    rng = np.random.default_rng(seed)
    out = [vals[i % len(vals)] for i in range(n)]
    rng.shuffle(out)
    return out
