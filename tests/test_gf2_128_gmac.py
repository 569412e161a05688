"""GF(2^128) pinned by GMAC tags that OpenSSL computed (tests/golden/golden_gf2_128_gmac.json, tests/golden/make_golden_gmac.py).

GHASH is Horner evaluation at H = E_K(0^128) in this field once each block's bits are reversed (`_refl`).  For an AAD of m whole
blocks A_1..A_m, GHASH = tag xor E_K(J0) is the value at refl(H) of P(x) = c_1 x + .. + c_{m+1} x^{m+1} with c_1 = refl(L),
L = (8 len(A)) << 64, and c_{k+1} = refl(A_{m+1-k}); the constant term is 0.  So every tag is an external evaluation of a
polynomial whose coefficients are the AAD, at a node that is a full-width field element, and it pins products, Horner chains,
sharing, matrix products, inversion and reconstruction at once.

The CPU half checks the fixture against the GCM specification's own multiplication (Algorithm 1), against the Python
shift-xor model after reflection, against the C oracle and -- where the `openssl` tool exists -- against OpenSSL again.  The
`gpu` half sends the fixture through every GF(2^128) kernel family and compares bit-exactly with the fixture."""
import contextlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from extremes import gf_mul, spec_mul
from extremes import refl as _refl

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_gf2_128_gmac.json")) as fh:
    GOLD = json.load(fh)


class GmacSet:
    """one set of the fixture: keys j, AADs s, tags[j][s]; GCM blocks are big-endian integers, field elements reflected"""

    def __init__(self, d):
        self.H = [int(k["h"], 16) for k in d["keys"]]
        self.E = [int(k["ekj0"], 16) for k in d["keys"]]
        raw = [bytes.fromhex(a) for a in d["aads"]]
        self.aads = [[int.from_bytes(a[i:i + 16], "big") for i in range(0, len(a), 16)] for a in raw]
        self.tags = [[int(t, 16) for t in row] for row in d["tags"]]
        self.nodes = [_refl(h) for h in self.H]
        self.coeffs = []   # [s] -> [c_1 .. c_{m+1}] as field elements
        for blocks in self.aads:
            L = (128 * len(blocks)) << 64
            self.coeffs.append([_refl(L)] + [_refl(b) for b in reversed(blocks)])
        self.values = [[_refl(self.tags[j][s] ^ self.E[j]) for s in range(len(self.aads))] for j in range(len(self.H))]

    def ghash(self, j, s):
        return self.tags[j][s] ^ self.E[j]

    def degree(self, s):
        return len(self.coeffs[s])


SETS = {name: GmacSet(d) for name, d in GOLD["sets"].items()}
GRID, LONG, NODES = SETS["grid"], SETS["long"], SETS["nodes"]


def length_block(blocks):
    return (128 * len(blocks)) << 64


# ---- the fixture itself -------------------------------------------------------------------------------------------------------------
def test_the_fixture_has_the_documented_shape():
    assert GOLD["openssl_version"].startswith("OpenSSL ") and GOLD["seed"] == 0x6D4D4143
    assert (len(GRID.H), len(GRID.aads)) == (24, 64) and [len(a) for a in GRID.aads] == [s % 16 + 1 for s in range(64)]
    assert (len(LONG.H), [len(a) for a in LONG.aads]) == (4, [32, 47, 63, 64, 100, 127])
    assert (len(NODES.H), [len(a) for a in NODES.aads]) == (136, [1, 2, 3, 3])
    for st in SETS.values():
        assert len(st.tags) == len(st.H) and all(len(r) == len(st.aads) for r in st.tags)
        assert len(set(st.H)) == len(st.H)   # distinct nodes
    # the reflection's edges sit at the first and at the last block of some AAD: zero, all ones, only the first bit (x^0),
    # only the last bit (x^127), and a key's H
    edges = [0, (1 << 128) - 1, 1 << 127, 1, GRID.H[5]]
    assert all(any(a[0] == e for a in GRID.aads) and any(a[-1] == e for a in GRID.aads) for e in edges)
    assert os.path.getsize(os.path.join(HERE, "golden", "golden_gf2_128_gmac.json")) < 512 * 1024


@pytest.mark.parametrize("name", sorted(SETS))
def test_fixture_against_the_gcm_specification(name):
    """every tag: E_K(J0) xor GHASH with GHASH by the specification's Algorithm 1 (right shifts, R = e1 || 0^120) over the AAD
    blocks and the length block -- and the same chain on the Python shift-xor model after reflection"""
    st = SETS[name]
    for j, h in enumerate(st.H):
        hr = st.nodes[j]
        for s, blocks in enumerate(st.aads):
            x = xr = 0
            for b in blocks + [length_block(blocks)]:
                x = spec_mul(x ^ b, h)
                xr = gf_mul(xr ^ _refl(b), hr)
            assert x == st.ghash(j, s), (name, j, s)
            assert xr == st.values[j][s], (name, j, s)


@pytest.mark.parametrize("name", sorted(SETS))
def test_oracle_poly_eval_at_the_keys_gives_the_fixture(name):
    port = O.Port()
    st = SETS[name]
    xs = O.from_ints(st.nodes, 2)
    for s, c in enumerate(st.coeffs):
        got = O.to_ints(port.poly_eval(O.GF2_128, O.from_ints([0] + c, 2), xs))
        assert got == [st.values[j][s] for j in range(len(st.H))], (name, s)


def test_fixture_against_openssl_again():
    """re-derive 8 tags and 2 H values with the tool that made them (skipped where it is not installed)"""
    import shutil
    import subprocess
    import tempfile
    if not shutil.which("openssl"):
        pytest.skip("openssl is not on PATH")
    picks = [("grid", 0, 0), ("grid", 5, 20), ("grid", 23, 63), ("grid", 11, 31), ("long", 1, 5), ("long", 3, 2),
             ("nodes", 135, 3), ("nodes", 64, 0)]
    with tempfile.TemporaryDirectory() as d:
        for name, j, s in picks:
            key, iv = GOLD["sets"][name]["keys"][j]["key"], GOLD["sets"][name]["keys"][j]["iv"]
            path = os.path.join(d, "aad.bin")
            with open(path, "wb") as fh:
                fh.write(bytes.fromhex(GOLD["sets"][name]["aads"][s]))
            r = subprocess.run(["openssl", "mac", "-cipher", "AES-128-GCM", "-macopt", "hexkey:" + key, "-macopt", "hexiv:" + iv,
                                "-in", path, "GMAC"], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert int(r.stdout.strip(), 16) == SETS[name].tags[j][s], (name, j, s)
    for name, j in (("grid", 7), ("nodes", 100)):
        key = GOLD["sets"][name]["keys"][j]["key"]
        r = subprocess.run(["openssl", "enc", "-aes-128-ecb", "-K", key, "-nopad"], input=bytes(16), capture_output=True)
        assert r.returncode == 0 and int.from_bytes(r.stdout, "big") == SETS[name].H[j]


# ---- the HIP kernels ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scl():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    import scl_amd
    return scl_amd


def E(vals):
    """field elements -> [n][2] uint64"""
    return O.from_ints(list(vals), 2)


def ints_of(scl, t):
    return O.to_ints(scl.to_host(t))


def coeff_rows(st, aad_of_lane, t):
    """[t + 1][N] coefficient rows c_0 = 0, c_1 .. c_t of lane s's polynomial (zero above its degree)"""
    rows = [[0] * len(aad_of_lane)]
    for k in range(1, t + 1):
        rows.append([st.coeffs[s][k - 1] if k <= st.degree(s) else 0 for s in aad_of_lane])
    return rows


def lanes(aads, N):
    return [aads[i % len(aads)] for i in range(N)]


KNOB_DEFAULT = {"inv_batch": 0, "force_table": 0, "matmul_lds_min": 0}


@contextlib.contextmanager
def tuned(scl, key, value):
    scl.set_tuning(key, value)
    try:
        yield
    finally:
        scl.set_tuning(key, KNOB_DEFAULT[key])


@pytest.mark.gpu
@pytest.mark.parametrize("inv_batch", [0, -1], ids=["lds_window", "register"])
def test_gpu_ghash_as_a_chain_of_elementwise_products(scl, inv_batch):
    """GHASH itself over all 1 536 grid lanes at once: X = (X + block_i) * H, one ADD and one MUL launch per block, AADs
    shorter than 16 blocks led by zero blocks (which leave X = 0), the length block last.  On the LDS window-table product
    (k_ew_gf128_mul) and on the register product ("inv_batch" -1).  Nothing intermediate comes from a model."""
    f = scl.GF2_128
    pairs = [(j, s) for j in range(len(GRID.H)) for s in range(len(GRID.aads))]
    steps = max(len(a) for a in GRID.aads) + 1
    seq = []
    for j, s in pairs:
        blocks = GRID.aads[s]
        seq.append([0] * (steps - 1 - len(blocks)) + [_refl(b) for b in blocks] + [_refl(length_block(blocks))])
    H = scl.to_device(E(GRID.nodes[j] for j, s in pairs))
    x = scl.to_device(E([0] * len(pairs)))
    with tuned(scl, "inv_batch", inv_batch):
        for i in range(steps):
            x = scl.ew(f, scl.MUL, scl.ew(f, scl.ADD, x, scl.to_device(E(q[i] for q in seq))), H)
    assert ints_of(scl, x) == [GRID.values[j][s] for j, s in pairs]


@pytest.mark.gpu
def test_gpu_scalar_mul_and_dot_give_ghash(scl):
    """scalar_mul by refl(H) as the Horner step of one key over all 64 grid AADs; dot(c_1 .. c_{m+1}, [H, H^2, ..]) for every
    grid and long pair (the powers of H by the Python model, itself pinned by the CPU half)"""
    f = scl.GF2_128
    steps = max(len(a) for a in GRID.aads) + 1
    seq = [[0] * (steps - 1 - len(b)) + [_refl(x) for x in b] + [_refl(length_block(b))] for b in GRID.aads]
    for j, h in enumerate(GRID.nodes):
        x = scl.to_device(E([0] * len(seq)))
        for i in range(steps):
            x = scl.scalar_mul(f, scl.ew(f, scl.ADD, x, scl.to_device(E(q[i] for q in seq))), E([h])[0])
        assert ints_of(scl, x) == GRID.values[j], j
    for st in (GRID, LONG):
        for j, h in enumerate(st.nodes):
            pw = [h]
            while len(pw) < max(st.degree(s) for s in range(len(st.aads))):
                pw.append(gf_mul(pw[-1], h))
            for s, c in enumerate(st.coeffs):
                got = O.to_ints(scl.dot(f, scl.to_device(E(c)), scl.to_device(E(pw[:len(c)])))[None])
                assert got == [st.values[j][s]], (j, s)


@pytest.mark.gpu
@pytest.mark.parametrize("inv_batch", [0, 32, -1], ids=["chained", "chain32", "per_element"])
def test_gpu_inverse_and_divide_with_external_inputs(scl, inv_batch):
    """Two 1-block AADs a, a' under one key: GHASH(a) xor GHASH(a') = (a xor a') H^2 (the length blocks cancel), so
    (g xor g') / (a xor a') = H^2 and that divided by H is H.  Over a batch of 10 007 elements, so that the chained
    inversion (k_ew_inv_rolled on LDS-table products, chains of 8 by default and of 32 forced, with a partial last chain) and
    the per-element form ("inv_batch" -1) all run; INV then MUL too."""
    f = scl.GF2_128
    one = [s for s in range(len(GRID.aads)) if len(GRID.aads[s]) == 1]
    quads = []
    for j in range(len(GRID.H)):
        for s in one:
            for s2 in one:
                if GRID.aads[s][0] != GRID.aads[s2][0]:
                    quads.append((GRID.values[j][s] ^ GRID.values[j][s2],
                                  _refl(GRID.aads[s][0] ^ GRID.aads[s2][0]), GRID.nodes[j]))
    assert len(quads) >= 200
    N = 10007
    quads = [quads[i % len(quads)] for i in range(N)]
    num, den, h = (scl.to_device(E(q[i] for q in quads)) for i in range(3))
    with tuned(scl, "inv_batch", inv_batch):
        h2 = scl.ew(f, scl.DIV, num, den)
        assert ints_of(scl, scl.ew(f, scl.DIV, h2, h)) == [q[2] for q in quads]
        assert ints_of(scl, h2) == [gf_mul(q[2], q[2]) for q in quads]
        assert ints_of(scl, scl.ew(f, scl.MUL, num, scl.ew(f, scl.INV, den))) == ints_of(scl, h2)
        # and back: H^2 * (a xor a') is the GHASH difference
        assert ints_of(scl, scl.ew(f, scl.MUL, h2, den)) == [q[0] for q in quads]


# sharing at full-width nodes: (set, AADs of degree <= t, t, N) -- k_share<.., 4>, <.., 16>, <.., 48>, the chunked Horner kernel (t > 48)
SHARE_CASES = [
    ("grid", 4, 257),     # AADs of <= 3 blocks
    ("grid", 16, 263),    # <= 15 blocks
    ("grid", 17, 259),    # all
    ("long", 128, 261),   # up to 127 blocks
    ("nodes", 4, 257),    # 136 nodes: two launches of at most 128 parties
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,t,N", SHARE_CASES)
def test_gpu_shamir_share_at_the_keys_gives_ghash(scl, name, t, N):
    """shamir_share with secrets 0, coefficient rows c_1 .. c_t and alphas = refl(H_j): share row j is refl(GHASH_{K_j})"""
    import torch
    f = scl.GF2_128
    st = SETS[name]
    aads = [s for s in range(len(st.aads)) if st.degree(s) <= t]
    assert max(st.degree(s) for s in aads) == t   # the kernel instance runs at its full width
    per_lane = lanes(aads, N)
    rows = coeff_rows(st, per_lane, t)
    coeffs = torch.stack([scl.to_device(E(r)) for r in rows[1:]])
    n = len(st.H)
    shares = scl.shamir_share(f, scl.to_device(E(rows[0])), coeffs, n, alphas=E(st.nodes))
    got = scl.to_host(shares)
    for j in range(n):
        assert O.to_ints(got[j]) == [st.values[j][s] for s in per_lane], (name, t, j)


@pytest.mark.gpu
@pytest.mark.parametrize("name,t", [("grid", 4), ("grid", 17), ("long", 128)])
@pytest.mark.parametrize("knob", [None, ("matmul_lds_min", 1024)], ids=["default", "matmul_lds_min"])
def test_gpu_vandermonde_times_coefficients_gives_ghash(scl, name, t, knob):
    """vandermonde(n, t + 1, xs = refl(H)) times the [t + 1][N] coefficient matrix: the same shares.  Default path (the tiled
    kernel at these sizes) and "matmul_lds_min" 1024 (fuzz_abi.KNOBS): the thin kernel at t = 4, the one-column-per-thread kernel
    at t = 17."""
    f = scl.GF2_128
    st = SETS[name]
    aads = [s for s in range(len(st.aads)) if st.degree(s) <= t]
    N = 1031
    per_lane = lanes(aads, N)
    C = scl.to_device(np.stack([E(r) for r in coeff_rows(st, per_lane, t)]))
    V = scl.vandermonde(f, len(st.H), t + 1, xs=E(st.nodes))
    if knob:
        with tuned(scl, *knob):
            out = scl.matmul(f, V, C)
    else:
        out = scl.matmul(f, V, C)
    got = scl.to_host(out)
    for j in range(len(st.H)):
        assert O.to_ints(got[j]) == [st.values[j][s] for s in per_lane], (name, t, j)


@pytest.mark.gpu
@pytest.mark.parametrize("force_table", [0, 3])
@pytest.mark.parametrize("m", [5, 7, 40, 41, 80, 81, 128, 130])
def test_gpu_reconstruction_at_a_held_out_key(scl, m, force_table):
    """From the GHASH values of m keys of the nodes set (degree <= 4), the Lagrange basis at the m nodes for x = the held-out
    key's node: shamir_recover gives the held-out key's GHASH.  m <= 40: position tables at 512 threads, 41..80: at 1024
    threads, 81..128: the shared-shift kernel, > 128: a second launch that adds to the first one's sums; "force_table" 3: the
    shared-shift kernel at every m."""
    import torch
    f = scl.GF2_128
    N = 1025
    out_j = len(NODES.H) - 1
    per_lane = lanes(list(range(len(NODES.aads))), N)
    lam = scl.lagrange_basis(f, m, alphas=E(NODES.nodes[:m]), x=E([NODES.nodes[out_j]])[0])
    shares = torch.stack([scl.to_device(E(NODES.values[j][s] for s in per_lane)) for j in range(m)])
    with tuned(scl, "force_table", force_table):
        rec = scl.shamir_recover(f, shares, lam)
    assert ints_of(scl, rec) == [NODES.values[out_j][s] for s in per_lane]


@pytest.mark.gpu
def test_gpu_detect_and_correct_at_the_keys(scl):
    """shamir_recover_detect over the 24 grid keys with d = 17 (16 blocks + the length block; t = 7 checked shares): consistent
    shares pass, evaluate to 0 at x = 0 and to the fixture at a key's node, and one altered share per lane is reported wherever
    it sits.  shamir_recover_correct (t = 7: the AADs of <= 6 blocks) with 3 altered shares recovers secret 0, the AAD's
    coefficients, and the corrected polynomial evaluated at the keys is the fixture."""
    import torch
    f = scl.GF2_128
    N = 321
    per_lane = lanes(list(range(len(GRID.aads))), N)
    vals = [[GRID.values[j][s] for s in per_lane] for j in range(24)]
    shares = torch.stack([scl.to_device(E(v)) for v in vals])
    al = E(GRID.nodes)
    out, status, bad = scl.shamir_recover_detect(f, shares, 7, 17, alphas=al)
    assert bad == 0 and not status.cpu().numpy().any() and ints_of(scl, out) == [0] * N
    out, status, bad = scl.shamir_recover_detect(f, shares, 7, 17, alphas=al, x=al[23])
    assert bad == 0 and ints_of(scl, out) == vals[23]
    hit = {s: (s * 5) % 24 for s in range(0, N, 3)}          # lane -> the party whose share is altered
    alt = [list(v) for v in vals]
    for s, j in hit.items():
        alt[j][s] ^= 1 << (s % 128)
    out, status, bad = scl.shamir_recover_detect(f, torch.stack([scl.to_device(E(v)) for v in alt]), 7, 17, alphas=al)
    st = status.cpu().numpy()
    assert bad == len(hit) and sorted(np.nonzero(st)[0].tolist()) == sorted(hit)
    # Berlekamp-Welch: t = (24 - 1) // 3 = 7, the first 22 shares
    short = [s for s in range(len(GRID.aads)) if GRID.degree(s) <= 7]
    per_lane = lanes(short, 257)
    vals = [[GRID.values[j][s] for s in per_lane] for j in range(24)]
    for i, s in enumerate(per_lane):
        for j in ((i * 7) % 22, (i * 7 + 5) % 22, (i * 7 + 13) % 22):
            vals[j][i] ^= ((i + 1) * 0x9E3779B97F4A7C15 << (j % 64)) & ((1 << 128) - 1)
    r = scl.shamir_recover_correct(f, torch.stack([scl.to_device(E(v)) for v in vals]), alphas=al)
    assert r["failed"] == 0 and not r["status"].cpu().numpy().any()
    assert r["nerr"].cpu().tolist() == [3] * len(per_lane)
    fr = scl.to_host(r["f"])
    want = coeff_rows(GRID, per_lane, 21)
    for k in range(22):
        assert O.to_ints(fr[k]) == want[k], k
    sh = scl.shamir_share(f, r["f"][0].contiguous(), r["f"][1:8].contiguous(), 24, alphas=al)
    got = scl.to_host(sh)
    for j in range(24):
        assert O.to_ints(got[j]) == [GRID.values[j][s] for s in per_lane], j
