"""The triple dealer, the host half: the Python model (tests/port_models.py) that deals triples in the reference's PRG order from pieces of the CPU oracle
only (Port.prg_blocks, from_bytes, ew, shamir_share_coeffs), pinned entry by entry to what the REFERENCE dealt
(tests/golden/golden_triples.json); and the C++ mirror's ss::randomTripleAdditive / ss::randomTripleShamir
(tests/cxx/test_triples_api.cc) on the same entries, plain and -- as a stand-alone program -- under the address and
undefined-behaviour sanitizers.  The model also checks the kernels in tests/test_gpu_triples.py.  Everything is exact.

The discipline (include/scl_hip_prep.h): E = byteSize, BPE = ceil(E/16).  Additive: triple s owns the blocks
[counter0 + s B, counter0 + (s+1) B), B = (2 + 3 (n-1)) BPE: a, b, the n-1 random shares of a, of b, of c.  Shamir: B = 2 BPE + 3 Bs,
Bs = ceil((t+1) E / 16): a, b, one Vector::random(t+1) draw per polynomial whose first element is discarded."""
import json

import numpy as np
import pytest

import oracle_lib as O
from cxx_support import SANITIZE, mirror_binary, mirror_host_output, needed
from port_models import TAGS, from_hex, golden, model_additive, model_shamir, protocol_from_model, triples_entry_matrices as entry_matrices


@pytest.fixture(scope="module")
def port():
    return O.Port()


def test_the_model_deals_the_fixtures_additive_triples(port):
    """every run: five consecutive triples, n in {2, 3, 5}, and the run after a three-block burn (counter0 = 3)"""
    runs = golden("triples")["additive"]
    assert len(runs) == 16
    for e in runs:
        f = TAGS[e["field"]]
        got = model_additive(port, f, e["seed"].encode(), e["burn"], len(e["triples"]), e["n"])
        for g, w, k in zip(got, entry_matrices(port, f, e), "abc"):
            assert np.array_equal(g, w), (e["field"], e["n"], e["burn"], k)


def test_the_model_deals_the_fixtures_shamir_triples(port):
    runs = golden("triples")["shamir"]
    assert len(runs) == 20 and {(e["n"], e["t"]) for e in runs} == {(4, 1), (10, 3), (16, 7), (20, 9)}
    for e in runs:
        f = TAGS[e["field"]]
        got = model_shamir(port, f, e["seed"].encode(), e["burn"], len(e["triples"]), e["t"], e["n"])
        for g, w, k in zip(got, entry_matrices(port, f, e), "abc"):
            assert np.array_equal(g, w), (e["field"], e["n"], e["t"], e["burn"], k)


def test_the_model_restates_the_references_protocol_test(port):
    """the reference's "Beaver multiplication protocol": its xs, ys, ts, and both parties' e, d, z of beaver.h:40-61; z0 + z1 = 462"""
    f, g, m = O.M61, golden("triples")["protocol"], protocol_from_model(port)
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
def test_the_mirror_deals_the_fixture():
    """ss::randomTripleAdditive / ss::randomTripleShamir on the fixture's seeds, burns and shapes print the fixture, and the
    program's restatement of "Beaver multiplication protocol" holds (exit status 0)"""
    r = mirror_host_output("triples")
    assert json.loads(r.stdout) == golden("triples")
    dynamic = needed(mirror_binary("triples"))
    assert "libscl_hip_prep.so" in dynamic and "libscl_hip.so" in dynamic


def test_the_mirror_under_the_sanitizers():
    """the same stand-alone program built with -fsanitize=address,undefined: the same output, no report"""
    r = mirror_host_output("triples", "test_triples_api_san", SANITIZE)
    assert json.loads(r.stdout) == golden("triples")
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
