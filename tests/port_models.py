"""The Python models of the protocol units built from pieces of the CPU oracle only (oracle_lib.Port), and the readers of their
fixtures under tests/golden/: the triple dealer, honest-majority multiplication, inner and matrix products at one opening, batch
verification and the Beaver finish.  tests/test_{triples,hm,ip,vf}_host.py pin each model entry by entry to what the REFERENCE
produced; the GPU value tests (tests/test_gpu_*.py) compare the kernels against the same functions.  Everything is exact.

The PRG disciplines are those of include/scl_hip_prep.h, scl_hip_hm.h and scl_hip_vf.h: E = byteSize, BPE = ceil(E/16),
Bs(d) = ceil((d+1) E / 16); the docstrings of the host test files state each unit's block ranges."""
import json
import os

import numpy as np

import oracle_lib as O

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = {"m61": O.M61, "m127": O.M127, "secp256k1_scalar": O.SECP256K1_SCALAR, "secp256k1_field": O.SECP256K1_FIELD}
TAGS3 = {k: TAGS[k] for k in ("m61", "m127", "secp256k1_scalar")}          # the fields of the ip and vf fixtures, in their order


def golden_path(unit):
    return os.path.join(GOLDEN_DIR, "golden_%s.json" % unit)


def golden(unit):
    """the `data` of tests/golden/golden_<unit>.json"""
    with open(golden_path(unit)) as fh:
        return json.load(fh)["data"]


def from_hex(port, f, strings):
    """FF::write images -> [len][L], by FF::read"""
    return port.from_bytes(f, bytes.fromhex("".join(strings)))


def ew(port, f, op, a, b):
    """Port.ew over arrays of any leading shape"""
    L = O.LIMBS[f]
    return port.ew(f, op, np.ascontiguousarray(a).reshape(-1, L), np.ascontiguousarray(b).reshape(-1, L)).reshape(a.shape)


# ---- the triple dealer -------------------------------------------------------------------------------------------------------
def bpe(f):
    return (O.byte_size(f) + 15) // 16


def additive_blocks(f, n):
    return (2 + 3 * (n - 1)) * bpe(f)


def poly_blocks(f, t):
    return ((t + 1) * O.byte_size(f) + 15) // 16


def shamir_blocks(f, t):
    return 2 * bpe(f) + 3 * poly_blocks(f, t)


def stream(port, seed, counter0, N, B):
    """the blocks of N triples, [N][16 B] bytes; the 64-bit counter wraps like the PRG's"""
    first = counter0 % (1 << 64)
    total = N * B
    head = min(total, (1 << 64) - first)
    raw = port.prg_blocks(seed, first, head) + (port.prg_blocks(seed, 0, total - head) if total > head else b"")
    return np.frombuffer(raw, dtype=np.uint8).reshape(N, 16 * B)


def random_at(port, f, st, block):
    """one FF::random per triple at block `block` of its range: the first byteSize bytes of BPE whole blocks -> [N][L]"""
    E = O.byte_size(f)
    return port.from_bytes(f, np.ascontiguousarray(st[:, 16 * block:16 * block + E]).tobytes())


def model_additive(port, f, seed, counter0, N, n):
    """-> a, b, c as [n][N][L] (party-major, the device layout)"""
    B, P = additive_blocks(f, n), bpe(f)
    st = stream(port, seed, counter0, N, B)
    a, b = random_at(port, f, st, 0), random_at(port, f, st, P)
    out = []
    for m, secret in enumerate((a, b, port.ew(f, O.MUL, a, b))):
        rows, last = [], secret
        for i in range(n - 1):
            r = random_at(port, f, st, (2 + m * (n - 1) + i) * P)
            last = port.ew(f, O.SUB, last, r)
            rows.append(r)
        out.append(np.stack(rows + [last]))
    return out


def model_shamir(port, f, seed, counter0, N, t, n):
    """-> a, b, c as [n][N][L]"""
    B, P, Bs = shamir_blocks(f, t), bpe(f), poly_blocks(f, t)
    st = stream(port, seed, counter0, N, B)
    a, b = random_at(port, f, st, 0), random_at(port, f, st, P)
    return [share_draw(port, f, st, 2 * P + m * Bs, secret, t, n) for m, secret in enumerate((a, b, port.ew(f, O.MUL, a, b)))]


def horner_at_bit_patterns(port, f, secret, coeffs, n):
    """GF(2^128): the reference's walk over the nodes, x++ on one() (shamir.h:62-65), cycles 1, 0, 1, .. in characteristic 2 and
    shamir_share_coeffs walks with it; the engine -- every batch path and the mirror -- evaluates at the bit patterns of 1, 2, ..,
    n instead.  Horner by the oracle's element-wise calls.  -> [N][n][L]"""
    N, t = coeffs.shape[0], coeffs.shape[1]
    rows = []
    for i in range(n):
        x = np.repeat(port.from_int(f, i + 1)[None], N, axis=0)
        y = np.ascontiguousarray(coeffs[:, t - 1])
        for k in range(t - 1, -1, -1):
            y = port.ew(f, O.ADD, port.ew(f, O.MUL, y, x), secret if k == 0 else np.ascontiguousarray(coeffs[:, k - 1]))
        rows.append(y)
    return np.stack(rows, axis=1)


def triples_entry_matrices(port, f, entry):
    """the triples fixture's triples of one run as a, b, c [n][count][L]"""
    return [np.stack([from_hex(port, f, tr[k]) for tr in entry["triples"]], axis=1) for k in "abc"]


def protocol_from_model(port):
    """test_protocol.cc:36-41 from the model: PRG::create() is the all-zero key; xs draws block 0, ys block 1, the triple
    starts at block 2.  -> dict of [2][L] arrays (and x, y)"""
    f, seed = O.M61, b""
    r = stream(port, seed, 0, 1, 2)
    x, y = port.from_int(f, 42)[None], port.from_int(f, 11)[None]
    xs0, ys0 = random_at(port, f, r, 0), random_at(port, f, r, 1)
    a, b, c = model_additive(port, f, seed, 2, 1, 2)
    return {"x": x, "y": y, "xs": np.stack([xs0, port.ew(f, O.SUB, x, xs0)])[:, 0], "ys": np.stack([ys0, port.ew(f, O.SUB, y, ys0)])[:, 0],
            "a": a[:, 0], "b": b[:, 0], "c": c[:, 0]}


# ---- honest-majority multiplication ------------------------------------------------------------------------------------------
def double_blocks(f, t):
    return bpe(f) + poly_blocks(f, t) + poly_blocks(f, 2 * t)


def share_draw(port, f, st, block, secret, d, n):
    """shamirSecretShare(secret, d, n, prg) with the prg at block `block` of each row of the stream -> [n][N][L]"""
    N, E, L = st.shape[0], O.byte_size(f), O.LIMBS[f]
    draw = port.from_bytes(f, np.ascontiguousarray(st[:, 16 * block:16 * block + (d + 1) * E]).tobytes()).reshape(N, d + 1, L)
    if d == 0:
        shares = np.repeat(secret[:, None, :], n, axis=1)
    elif f == O.GF2_128:
        shares = horner_at_bit_patterns(port, f, secret, draw[:, 1:], n)
    else:
        shares = port.shamir_share_coeffs(f, secret, np.ascontiguousarray(draw[:, 1:]), n)     # element 0 is discarded
    return np.ascontiguousarray(np.transpose(shares, (1, 0, 2)))


def model_double(port, f, seed, counter0, N, t, n):
    """-> lo, hi as [n][N][L] (party-major, the device layout) and r [N][L]"""
    st = stream(port, seed, counter0, N, double_blocks(f, t))
    r = random_at(port, f, st, 0)
    return share_draw(port, f, st, bpe(f), r, t, n), share_draw(port, f, st, bpe(f) + poly_blocks(f, t), r, 2 * t, n), r


def model_inputs(port, f, seed, P, t, n):
    """P products' inputs off one PRG: x, y = FF::random, then the degree-t sharings of x and of y, product after product
    -> x, y [P][L], xs, ys [n][P][L]"""
    B = 2 * bpe(f) + 2 * poly_blocks(f, t)
    st = stream(port, seed, 0, P, B)
    x, y = random_at(port, f, st, 0), random_at(port, f, st, bpe(f))
    return x, y, share_draw(port, f, st, 2 * bpe(f), x, t, n), share_draw(port, f, st, 2 * bpe(f) + poly_blocks(f, t), y, t, n)


def nodes(port, f, n):
    return np.stack([port.from_int(f, i + 1) for i in range(n)])


def model_him(port, f, m, n, points=None):
    """row i = the Lagrange basis of the nodes 1..n at the point -i (GF(2^128): at the bit pattern n + 1 + i) -> [m][n][L]"""
    zero = port.from_int(f, 0)
    if points is None:
        points = [n + 1 + i for i in range(m)] if f == O.GF2_128 else [-i for i in range(m)]
    xs = [port.from_int(f, p) if p >= 0 else port.ew(f, O.SUB, zero[None], port.from_int(f, -p)[None])[0] for p in points]
    return np.stack([port.lagrange_basis(f, nodes(port, f, n), x) for x in xs])


def model_apply(port, f, M, x):
    """out[k] = sum_i M[k][i] x[i]: M [m][n][L], x [n][N][L] -> [m][N][L]"""
    return port.matmul(f, M, x)


def model_mask(port, f, x, y, r2):
    return port.ew(f, O.ADD, port.ew(f, O.MUL, x, y), r2)


def model_open(port, f, dsh, lam=None):
    """dsh [m][N][L] at the nodes 1..m -> [N][L]"""
    if lam is None:
        lam = port.lagrange_basis(f, nodes(port, f, dsh.shape[0]), port.from_int(f, 0))
    return port.shamir_recover_lambda(f, np.ascontiguousarray(np.transpose(dsh, (1, 0, 2))), lam)


def model_finish(port, f, opened, r):
    """r [rows][N][L] -> opened - r"""
    return np.stack([port.ew(f, O.SUB, opened, row) for row in r])


def model_protocol(port, f, n, t, S, dealer_seeds, input_seed):
    """n dealers, S double sharings each, extraction with hyperInvertible(n - t, n), product p = S k + s -> dict of arrays:
    lo, hi [dealer][party][S], M, R_lo, R_hi [party][(n-t) S], x, y, xs, ys, d_shares, d, z_shares, z"""
    m = n - t
    deals = [model_double(port, f, s, 0, S, t, n) for s in dealer_seeds]
    lo, hi = np.stack([d[0] for d in deals]), np.stack([d[1] for d in deals])
    M = model_him(port, f, m, n)
    L = O.LIMBS[f]
    R_lo = np.stack([model_apply(port, f, M, np.ascontiguousarray(lo[:, j])).reshape(m * S, L) for j in range(n)])
    R_hi = np.stack([model_apply(port, f, M, np.ascontiguousarray(hi[:, j])).reshape(m * S, L) for j in range(n)])
    x, y, xs, ys = model_inputs(port, f, input_seed, m * S, t, n)
    d_shares = model_mask(port, f, xs, ys, R_hi)
    d = model_open(port, f, d_shares)
    z_shares = model_finish(port, f, d, R_lo)
    return {"lo": lo, "hi": hi, "M": M, "R_lo": R_lo, "R_hi": R_hi, "x": x, "y": y, "xs": xs, "ys": ys, "d_shares": d_shares, "d": d,
            "z_shares": z_shares, "z": model_open(port, f, z_shares)}


def hm_protocol_entry(port, f, e):
    """one `protocol` run of the hm fixture in model_protocol's layout"""
    S = len(e["dealers"][0]["sharings"])
    col = lambda rows: np.stack([from_hex(port, f, r) for r in rows], axis=1)            # [p][party] -> [party][p]
    out = {"lo": np.stack([col([s["lo"] for s in d["sharings"]]) for d in e["dealers"]]),
           "hi": np.stack([col([s["hi"] for s in d["sharings"]]) for d in e["dealers"]]),
           "R_lo": col([s["v"] for k in e["R_lo"] for s in k]), "R_hi": col([s["v"] for k in e["R_hi"] for s in k])}
    for k in ("d_shares", "z_shares"):
        out[k] = col([p[k] for p in e["products"]])
    for k in ("x", "y", "d", "z"):
        out[k] = from_hex(port, f, e[k])
    return out, S


# ---- inner and matrix products at one opening --------------------------------------------------------------------------------
def model_dot_mask(port, f, x, y, r2=None):
    """x, y [terms][...][L], r2 [...][L] or None -> sum_k x[k] y[k] (+ r2), one reduced operation at a time"""
    acc = ew(port, f, O.MUL, x[0], y[0])
    for k in range(1, x.shape[0]):
        acc = ew(port, f, O.ADD, acc, ew(port, f, O.MUL, x[k], y[k]))
    return acc if r2 is None else ew(port, f, O.ADD, acc, r2)


def model_matmul_mask(port, f, X, Y, r2=None):
    """X [batch][a][K][N][L], Y [batch][K][b][N][L], r2 [batch][a][b][N][L] or None -> [batch][a][b][N][L]"""
    batch, a, K, N, L = X.shape
    b = Y.shape[2]
    out = np.zeros((batch, a, b, N, L), dtype=np.uint64)
    for i in range(a):
        for l in range(b):
            out[:, i, l] = model_dot_mask(port, f, np.moveaxis(X[:, i], 1, 0), np.moveaxis(Y[:, :, l], 1, 0), None if r2 is None else r2[:, i, l])
    return out


def inner_entry(port, f, e):
    """one `inner` entry of the ip fixture: the model's operands in the device layout and what the reference recorded
    -> xs, ys [K][n][1][L], lo, hi [n][1][L], want (dict)"""
    n, t, K = e["n"], e["t"], e["K"]
    x, y, xs, ys = model_inputs(port, f, b"ip inputs", K, t, n)              # xs [n][K][L]
    assert np.array_equal(x, from_hex(port, f, e["x"])) and np.array_equal(y, from_hex(port, f, e["y"])), (e["field"], n, K, "the inputs")
    lo, hi, _ = model_double(port, f, b"ip dealer", 0, 1, t, n)             # [n][1][L]
    want = {k: from_hex(port, f, e["out"][k])[:, None] for k in ("d_shares", "z_shares")}
    want.update({k: from_hex(port, f, [e["out"][k]]) for k in ("d", "z")})
    want["x"], want["y"] = x, y
    term_major = lambda s: np.ascontiguousarray(np.transpose(s, (1, 0, 2))[:, :, None])
    return term_major(xs), term_major(ys), lo, hi, want


def matrix_entry(port, f, e):
    """one `matrix` entry of the ip fixture -> X [n][a][K][1][L], Y [n][K][b][1][L], lo, hi [n][a][b][1][L], want"""
    n, t, a, K, b = e["n"], e["t"], e["a"], e["K"], e["b"]
    x, y, xs, ys = model_inputs(port, f, b"ip matrix", a * K, t, n)          # pair p: X's entry p, Y's entry p, row-major
    assert np.array_equal(x, from_hex(port, f, e["x"])) and np.array_equal(y, from_hex(port, f, e["y"])), (e["field"], n, a, K, b, "the inputs")
    lo, hi, _ = model_double(port, f, b"ip dealer", 0, a * b, t, n)         # [n][a b][L]
    L = O.LIMBS[f]
    want = {k: np.stack([from_hex(port, f, o[k]) for o in e["out"]], axis=1).reshape(n, a, b, 1, L) for k in ("d_shares", "z_shares")}
    want.update({k: from_hex(port, f, [o[k] for o in e["out"]]) for k in ("d", "z")})
    want["x"], want["y"] = x, y
    return xs.reshape(n, a, K, 1, L), ys.reshape(n, K, b, 1, L), lo.reshape(n, a, b, 1, L), hi.reshape(n, a, b, 1, L), want


# ---- batch verification ------------------------------------------------------------------------------------------------------
def coin_blocks(f, N):
    return -(-N * O.byte_size(f) // 16)


def model_coins(port, f, seed, counter0, N, reps):
    """-> rho [reps][N][L]: `reps` consecutive Vector::random(N) of a PRG on `seed` at block counter0"""
    bs, B = O.byte_size(f), coin_blocks(f, N)
    if N == 0:
        return np.zeros((reps, 0, O.LIMBS[f]), dtype=np.uint64)
    return np.stack([port.from_bytes(f, port.prg_blocks(seed, counter0 + j * B, B)[:N * bs]) for j in range(reps)])


def model_combine(port, f, x, rho, y=None):
    """x (y) [rows][N][L], rho [reps][N][L] -> [rows][reps][L]: Port.dot of rho_j with x_r (x_r .* y_r); the empty sum is zero"""
    rows, N, L = x.shape
    out = np.zeros((rows, rho.shape[0], L), dtype=np.uint64)
    if N == 0:
        return out
    for r in range(rows):
        m = np.ascontiguousarray(x[r]) if y is None else port.ew(f, O.MUL, np.ascontiguousarray(x[r]), np.ascontiguousarray(y[r]))
        for j in range(rho.shape[0]):
            out[r, j] = port.dot(f, np.ascontiguousarray(rho[j]), m)
    return out


def hex_rows(port, f, rows):
    return np.stack([from_hex(port, f, r) for r in rows])


def degree_entry(port, f, e):
    """one `degree` entry of the vf fixture -> rows [n][N][L] (party i's shares of the N secrets), rho [1][N][L], secrets"""
    secrets = port.vector_random(f, b"vf secrets", e["N"])
    assert np.array_equal(secrets, from_hex(port, f, e["secrets"])), (e["field"], "the secrets")
    shares = port.shamir_share(f, b"vf sharing", secrets, e["t"], e["n"])                  # [N][n][L], one PRG, secret after secret
    return np.ascontiguousarray(np.transpose(shares, (1, 0, 2))), model_coins(port, f, b"vf coin", e["counter0"], e["N"], 1), secrets


def product_entry(port, f, e):
    """one `product` entry of the vf fixture -> a, b, c rows [n][N][L], rho [1][N][L]"""
    a, b = port.vector_random(f, b"vf a", e["N"]), port.vector_random(f, b"vf b", e["N"])
    assert np.array_equal(a, from_hex(port, f, e["a"])) and np.array_equal(b, from_hex(port, f, e["b"])), (e["field"], "the factors")
    c = port.ew(f, O.MUL, a, b)
    sh = lambda seed, v: np.ascontiguousarray(np.transpose(port.shamir_share(f, seed, v, e["t"], e["n"]), (1, 0, 2)))
    return sh(b"vf share a", a), sh(b"vf share b", b), sh(b"vf share c", c), model_coins(port, f, b"vf coin", e["counter0"], e["N"], 1)


# ---- the Beaver finish -------------------------------------------------------------------------------------------------------
def oracle_finish(port, f, e, d, a, b, c, add_ed):
    """e b + d a + c (+ e d), one oracle element-wise call per operation; a, b, c [n][L] and e, d [n][L]"""
    z = port.ew(f, O.ADD, port.ew(f, O.ADD, port.ew(f, O.MUL, e, b), port.ew(f, O.MUL, d, a)), c)
    return port.ew(f, O.ADD, z, port.ew(f, O.MUL, e, d)) if add_ed else z
