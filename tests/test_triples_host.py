"""The triple dealer, the host half: a Python model that deals triples in the reference's PRG order from pieces of the CPU oracle
only (Port.prg_blocks, from_bytes, ew, shamir_share_coeffs), pinned entry by entry to what the REFERENCE dealt
(tests/golden/golden_triples.json); and the C++ mirror's ss::randomTripleAdditive / ss::randomTripleShamir
(tests/cxx/test_triples_api.cc) on the same entries, plain and -- as a stand-alone program -- under the address and
undefined-behaviour sanitizers.  The model also checks the kernels in tests/test_gpu_triples.py.  Everything is exact.

The discipline (include/scl_hip_prep.h): E = byteSize, BPE = ceil(E/16).  Additive: triple s owns the blocks
[counter0 + s B, counter0 + (s+1) B), B = (2 + 3 (n-1)) BPE: a, b, the n-1 random shares of a, of b, of c.  Shamir: B = 2 BPE + 3 Bs,
Bs = ceil((t+1) E / 16): a, b, one Vector::random(t+1) draw per polynomial whose first element is discarded."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_triples.json")
TAGS = {"m61": O.M61, "m127": O.M127, "secp256k1_scalar": O.SECP256K1_SCALAR, "secp256k1_field": O.SECP256K1_FIELD}


# ---- the model ---------------------------------------------------------------------------------------------------------------
def bpe(f):
    return (O.byte_size(f) + 15) // 16


def additive_blocks(f, n):
    return (2 + 3 * (n - 1)) * bpe(f)


def poly_blocks(f, t):
    return ((t + 1) * O.byte_size(f) + 15) // 16


def shamir_blocks(f, t):
    return 2 * bpe(f) + 3 * poly_blocks(f, t)


def _stream(port, seed, counter0, N, B):
    """the blocks of N triples, [N][16 B] bytes; the 64-bit counter wraps like the PRG's"""
    first = counter0 % (1 << 64)
    total = N * B
    head = min(total, (1 << 64) - first)
    raw = port.prg_blocks(seed, first, head) + (port.prg_blocks(seed, 0, total - head) if total > head else b"")
    return np.frombuffer(raw, dtype=np.uint8).reshape(N, 16 * B)


def _random(port, f, stream, block):
    """one FF::random per triple at block `block` of its range: the first byteSize bytes of BPE whole blocks -> [N][L]"""
    E = O.byte_size(f)
    return port.from_bytes(f, np.ascontiguousarray(stream[:, 16 * block:16 * block + E]).tobytes())


def model_additive(port, f, seed, counter0, N, n):
    """-> a, b, c as [n][N][L] (party-major, the device layout)"""
    B, P = additive_blocks(f, n), bpe(f)
    st = _stream(port, seed, counter0, N, B)
    a, b = _random(port, f, st, 0), _random(port, f, st, P)
    out = []
    for m, secret in enumerate((a, b, port.ew(f, O.MUL, a, b))):
        rows, last = [], secret
        for i in range(n - 1):
            r = _random(port, f, st, (2 + m * (n - 1) + i) * P)
            last = port.ew(f, O.SUB, last, r)
            rows.append(r)
        out.append(np.stack(rows + [last]))
    return out


def model_shamir(port, f, seed, counter0, N, t, n):
    """-> a, b, c as [n][N][L]"""
    B, P, Bs, E, L = shamir_blocks(f, t), bpe(f), poly_blocks(f, t), O.byte_size(f), O.LIMBS[f]
    st = _stream(port, seed, counter0, N, B)
    a, b = _random(port, f, st, 0), _random(port, f, st, P)
    out = []
    for m, secret in enumerate((a, b, port.ew(f, O.MUL, a, b))):
        lo = 16 * (2 * P + m * Bs)
        draw = port.from_bytes(f, np.ascontiguousarray(st[:, lo:lo + (t + 1) * E]).tobytes()).reshape(N, t + 1, L)
        if t == 0:
            shares = np.repeat(secret[:, None, :], n, axis=1)
        elif f == O.GF2_128:
            shares = _horner_at_bit_patterns(port, f, secret, draw[:, 1:], n)
        else:
            shares = port.shamir_share_coeffs(f, secret, np.ascontiguousarray(draw[:, 1:]), n)     # element 0 is discarded
        out.append(np.ascontiguousarray(np.transpose(shares, (1, 0, 2))))
    return out


def _horner_at_bit_patterns(port, f, secret, coeffs, n):
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


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["data"]


def from_hex(port, f, strings):
    """FF::write images -> [len][L], by FF::read"""
    return port.from_bytes(f, bytes.fromhex("".join(strings)))


def entry_matrices(port, f, entry):
    """the fixture's triples of one run as a, b, c [n][count][L]"""
    return [np.stack([from_hex(port, f, tr[k]) for tr in entry["triples"]], axis=1) for k in "abc"]


@pytest.fixture(scope="module")
def port():
    return O.Port()


def test_the_model_deals_the_fixtures_additive_triples(port):
    """every run: five consecutive triples, n in {2, 3, 5}, and the run after a three-block burn (counter0 = 3)"""
    runs = golden()["additive"]
    assert len(runs) == 16
    for e in runs:
        f = TAGS[e["field"]]
        got = model_additive(port, f, e["seed"].encode(), e["burn"], len(e["triples"]), e["n"])
        for g, w, k in zip(got, entry_matrices(port, f, e), "abc"):
            assert np.array_equal(g, w), (e["field"], e["n"], e["burn"], k)


def test_the_model_deals_the_fixtures_shamir_triples(port):
    runs = golden()["shamir"]
    assert len(runs) == 20 and {(e["n"], e["t"]) for e in runs} == {(4, 1), (10, 3), (16, 7), (20, 9)}
    for e in runs:
        f = TAGS[e["field"]]
        got = model_shamir(port, f, e["seed"].encode(), e["burn"], len(e["triples"]), e["t"], e["n"])
        for g, w, k in zip(got, entry_matrices(port, f, e), "abc"):
            assert np.array_equal(g, w), (e["field"], e["n"], e["t"], e["burn"], k)


def protocol_from_model(port):
    """test_protocol.cc:36-41 from the model: PRG::create() is the all-zero key; xs draws block 0, ys block 1, the triple
    starts at block 2.  -> dict of [2][L] arrays (and x, y)"""
    f, seed = O.M61, b""
    r = _stream(port, seed, 0, 1, 2)
    x, y = port.from_int(f, 42)[None], port.from_int(f, 11)[None]
    xs0, ys0 = _random(port, f, r, 0), _random(port, f, r, 1)
    a, b, c = model_additive(port, f, seed, 2, 1, 2)
    return {"x": x, "y": y, "xs": np.stack([xs0, port.ew(f, O.SUB, x, xs0)])[:, 0], "ys": np.stack([ys0, port.ew(f, O.SUB, y, ys0)])[:, 0],
            "a": a[:, 0], "b": b[:, 0], "c": c[:, 0]}


def test_the_model_restates_the_references_protocol_test(port):
    """the reference's "Beaver multiplication protocol": its xs, ys, ts, and both parties' e, d, z of beaver.h:40-61; z0 + z1 = 462"""
    f, g, m = O.M61, golden()["protocol"], protocol_from_model(port)
    for k in ("xs", "ys", "a", "b", "c"):
        assert np.array_equal(m[k], from_hex(port, f, g[k])), k
    e2, d2 = port.ew(f, O.SUB, m["xs"], m["a"]), port.ew(f, O.SUB, m["ys"], m["b"])
    e, d = port.ew(f, O.ADD, e2[:1], e2[1:]), port.ew(f, O.ADD, d2[:1], d2[1:])
    assert np.array_equal(np.concatenate([e2, e]), from_hex(port, f, g["e"]))
    assert np.array_equal(np.concatenate([d2, d]), from_hex(port, f, g["d"]))
    ee, dd = np.repeat(e, 2, axis=0), np.repeat(d, 2, axis=0)
    z = port.ew(f, O.ADD, port.ew(f, O.ADD, port.ew(f, O.MUL, ee, m["b"]), port.ew(f, O.MUL, dd, m["a"])), m["c"])
    z[0] = port.ew(f, O.ADD, z[:1], port.ew(f, O.MUL, e, d))[0]          # only party 0 adds constants
    total = port.ew(f, O.ADD, z[:1], z[1:])
    assert np.array_equal(np.concatenate([z, total]), from_hex(port, f, g["z"]))
    assert O.to_ints(total) == [462] and g["z"][2] == (462).to_bytes(8, "little").hex()


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------
def _newest_header():
    return max(os.path.getmtime(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs)


def triples_binary(name="test_triples_api", flags=("-O2",)):
    """tests/cxx/test_triples_api.cc compiled against the mirror and the libraries (build() leaves it in place; rebuilt here when
    stale)"""
    src, exe = os.path.join(CXX, "test_triples_api.cc"), os.path.join(CXX, "_build", name)
    lib = os.path.join(ROOT, "secure-computation-library_amd", "scl_amd")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(_newest_header(), os.path.getmtime(src)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        b = subprocess.run(["g++", "-std=c++20", *flags, "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{ROOT}/include", "-o", exe, src,
                            f"-L{lib}", "-lscl_hip_prep", "-lscl_hip_mpc", "-lscl_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
    return exe


def mirror_output(exe):
    r = subprocess.run([exe, "--host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_the_mirror_deals_the_fixture():
    """ss::randomTripleAdditive / ss::randomTripleShamir on the fixture's seeds, burns and shapes print the fixture, and the
    program's restatement of "Beaver multiplication protocol" holds (exit status 0)"""
    r = mirror_output(triples_binary())
    assert json.loads(r.stdout) == golden()
    needed = subprocess.run(["readelf", "-d", triples_binary()], capture_output=True, text=True, check=True).stdout
    assert "libscl_hip_prep.so" in needed and "libscl_hip.so" in needed


def test_the_mirror_under_the_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined: the same output, no report"""
    exe = triples_binary("test_triples_api_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                  "-fno-omit-frame-pointer"))
    r = mirror_output(exe)
    assert json.loads(r.stdout) == golden()
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
