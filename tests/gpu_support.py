"""What the GPU tests of the extension libraries share: the environment fixture's body, PRG-seeded operands, the references that
are computed once per run and read by more than one file, the helpers that place operands on the device, and the arena helpers of
the red-zone and aliasing tests (tests/redzone.py).  Every assert carries the values it compared: this is no test module, so
pytest does not rewrite them."""
import importlib

import numpy as np
import pytest
import torch

import oracle_lib as O
import redzone as R
from port_models import model_additive, model_double, model_shamir, oracle_finish
from secp256k1_model import P as SECP_P
from secp256k1_model import Q as SECP_Q
from secp256k1_model import ec_image

MONT_P = (1 << 128) - 159
OK = 0


def gpu_env(*extensions):
    """-> (scl_amd, scl_amd.<extension>.., port) with the Mont128 modulus of the tests set on both sides"""
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a GPU")
    import scl_amd
    modules = [importlib.import_module("scl_amd." + name) for name in extensions]
    port = O.Port()
    scl_amd.set_mont128_prime(MONT_P)
    port.mont128_set_prime(MONT_P)
    return (scl_amd, *modules, port)


def fname(f):
    return {O.M61: "m61", O.M127: "m127", O.MONT128: "mont128", O.GF2_128: "gf128", O.SECP256K1_SCALAR: "secp_scalar",
            O.SECP256K1_FIELD: "secp_field"}.get(f, "z2k%d" % (f - 0x100))


def host(t):
    return t.detach().cpu().numpy().view(np.uint64)


# ---- operands ------------------------------------------------------------------------------------------------------------------
def rnd(port, f, n, tag: bytes, prefix=b"beaver-"):
    """n uniform elements from the oracle's own read of PRG bytes on the seed prefix + tag (the prefix is the first user's: every
    reference of the extension tests was drawn under it)"""
    if O.is_ring(f):
        bs = O.byte_size(f)
        return port.from_bytes(f, port.prg(prefix + tag, [max(n, 1) * bs]))[:n]
    return port.vector_random(f, prefix + tag, n)


def pm1(port, f):
    """p - 1 (GF(2^128): all ones), the largest canonical element"""
    if f == O.GF2_128:
        return np.full(2, 2 ** 64 - 1, dtype=np.uint64)
    return port.ew(f, O.SUB, port.from_int(f, 0)[None], port.from_int(f, 1)[None])[0]


def pool(port, f, count, tag):
    """`count` elements that repeat a uniform pool of 4099 with an odd period (rows and batches all differ)"""
    base = rnd(port, f, 4099, tag)
    return base[np.arange(count) % 4099]


# ---- references computed once and shared between the value tests and the red-zone tests of a unit ---------------------------------
BEAVER_ROWS, BEAVER_N = 3, 4099           # the largest shape of tests/test_gpu_beaver.py; every other one is a prefix
HM_SEED, HM_N = b"gpu hm", 1025
TRIPLES_SEED, TRIPLES_N = b"gpu triples", 257
_REF = {}


def beaver_reference(port, f):
    """operands [BEAVER_ROWS][BEAVER_N][L], e, d [BEAVER_N][L] and the oracle's results, once per field"""
    if ("beaver", f) not in _REF:
        L, RMAX, NMAX = O.LIMBS[f], BEAVER_ROWS, BEAVER_N
        r = {k: rnd(port, f, RMAX * NMAX, k.encode()).reshape(RMAX, NMAX, L) for k in ("x", "y", "a", "b", "c")}
        r["e"], r["d"] = rnd(port, f, NMAX, b"e"), rnd(port, f, NMAX, b"d")
        flat = lambda k: r[k].reshape(RMAX * NMAX, L)
        r["mask_e"] = port.ew(f, O.SUB, flat("x"), flat("a")).reshape(RMAX, NMAX, L)
        r["mask_d"] = port.ew(f, O.SUB, flat("y"), flat("b")).reshape(RMAX, NMAX, L)
        tile = lambda k: np.ascontiguousarray(np.broadcast_to(r[k], (RMAX, NMAX, L))).reshape(RMAX * NMAX, L)
        for add_ed in (0, 1):
            r["z%d" % add_ed] = oracle_finish(port, f, tile("e"), tile("d"), flat("a"), flat("b"), flat("c"), add_ed).reshape(
                RMAX, NMAX, L)
        _REF["beaver", f] = r
    return _REF["beaver", f]


def hm_reference(port, f, n, t, counter0=0, N=HM_N):
    """the model's lo, hi [n][N][L] and r [N][L] on HM_SEED, once per case"""
    key = ("hm", f, n, t, counter0, N)
    if key not in _REF:
        _REF[key] = model_double(port, f, HM_SEED, counter0, N, t, n)
    return _REF[key]


def triples_reference(port, f, n, t=None, counter0=0, N=TRIPLES_N):
    """the model's a, b, c [n][N][L] on TRIPLES_SEED (t None: additive), once per case"""
    key = ("triples", f, n, t, counter0, N)
    if key not in _REF:
        _REF[key] = model_additive(port, f, TRIPLES_SEED, counter0, N, n) if t is None else model_shamir(port, f, TRIPLES_SEED, counter0, N, t, n)
    return _REF[key]


# ---- operands on the device ------------------------------------------------------------------------------------------------------
def placed(dense, strides, phase=0):
    """a device copy of `dense` [d0]..[dk][N][L] whose leading axes lie `strides` elements apart, `phase` elements into a zeroed
    buffer -> (buffer, view)"""
    lead, (N, L) = dense.shape[:-2], dense.shape[-2:]
    extent = sum((n - 1) * s for n, s in zip(lead, strides)) + N
    buf = torch.zeros((extent + phase + 2) * L, dtype=torch.int64, device="cuda")
    v = torch.as_strided(buf, tuple(dense.shape), tuple(s * L for s in strides) + (L, 1), phase * L)
    v.copy_(dense)
    return buf, v


def only_the_view_was_written(buf, view):
    rest = buf.clone()
    torch.as_strided(rest, tuple(view.shape), view.stride(), view.storage_offset() - buf.storage_offset()).zero_()
    return not rest.any().item()


def deal_all(hm, f, S, t, n, seeds, lo, hi, scratch=None, flags=0):
    """dealer i's S double sharings into lo[i], hi[i]: [dealer][party][S][L]"""
    for i, s in enumerate(seeds):
        hm.double_share(f, S, t, n, s, out=(lo[i], hi[i]), scratch=scratch, flags=flags)


def hm_chain_buffers(f, n, t, S):
    """the buffers of the honest-majority chain: n dealers, S double sharings each, (n - t) S products"""
    L, m = O.LIMBS[f], n - t
    z = lambda *shape: torch.zeros(*shape, L, dtype=torch.int64, device="cuda")
    return {"lo": z(n, n, S), "hi": z(n, n, S), "R_lo": z(n, m, S), "R_hi": z(n, m, S), "d": z(n, m * S), "z": z(n, m * S), "out": z(m * S)}


# ---- secp256k1 on the device: between the big-integer model's values and the engine's Montgomery limbs and Jacobian points ----------
SECP_R = 1 << 256


def limbs_of(v: int):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]


def scalars_dev(scl, values):
    """integers -> SECP256K1_SCALAR elements (Montgomery limbs) on the device"""
    return scl.to_device(np.array([limbs_of(v % SECP_Q * SECP_R % SECP_Q) for v in values], dtype=np.uint64).reshape(len(values), 4))


def scalars_host(scl, t):
    """SECP256K1_SCALAR elements -> integers"""
    rinv = pow(SECP_R, -1, SECP_Q)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % SECP_Q for row in scl.to_host(t).reshape(-1, 4)]


def points_dev(scl, pts):
    """model points -> device points (Z = 1, or infinity), through their images"""
    raw = torch.from_numpy(np.frombuffer(b"".join(ec_image(p) for p in pts), dtype=np.uint8).copy().reshape(len(pts), 65)).cuda()
    out, status = scl.ec_wire_unpack(raw)
    assert not status.any(), status
    return out


def images(scl, points):
    raw = scl.ec_wire_pack(points.reshape(-1, 12)).cpu().numpy()
    return [raw[i].tobytes() for i in range(raw.shape[0])]


def rescale(scl, points, seed: int):
    """(X, Y, Z) -> (zX, zY, zZ) with a random non-zero z per point: the same points under other coordinates"""
    n = points.shape[0]
    rng = np.random.default_rng(seed)
    z = [int.from_bytes(rng.bytes(32), "big") % (SECP_P - 1) + 1 for _ in range(n)]
    zl = np.array([limbs_of(v * SECP_R % SECP_P) for v in z for _ in range(3)], dtype=np.uint64).reshape(3 * n, 4)
    f = scl.SECP256K1_FIELD
    return scl.ew(f, scl.MUL, points.reshape(3 * n, 4).contiguous(), scl.to_device(zl)).reshape(n, 12)


# ---- arenas: share matrices as windows of a tests/redzone.py arena -----------------------------------------------------------------
def limbs(f):
    return O.LIMBS[f]


def esz(f):
    return 8 * limbs(f)


def placements(f, N, k):
    """(align, phase in bytes, pitch in elements): one limb -- both phases, the pitch even and odd in turn; wider -- two of the
    three phases in rotation at a pitch of N + 3"""
    if limbs(f) == 1:
        even = N + 2 + (N % 2)
        return [(16, 0, even), (16, 0, even + 1), (16, 8, even), (16, 8, even + 1)]
    return [(128, (0, 16, 48)[(k + i) % 3], N + 3) for i in (0, 1)]


def mat(A, name, f, rows, N, pitch, align, phase, kind="out", data=None):
    """a window of `rows` rows of N elements, `pitch` elements apart, filled from `data` when given"""
    w = A.window(name, N * esz(f), align, phase, rows=rows, pitch_bytes=pitch * esz(f), kind=kind)
    if data is not None:
        w.load(np.ascontiguousarray(data))
    return w


def el(w, f):
    """a window's elements, [rows][N][L]"""
    return w.read(np.uint64).reshape(w.rows, -1, limbs(f))


def settle(last_error, A, rc, note):
    """the call returned OK and wrote nothing outside its output windows; `last_error` is the library's scl_X_last_error"""
    assert rc == OK, f"{note}: status {rc} ({last_error().decode()})"
    try:
        A.check()
    except R.RedZoneError as e:
        raise R.RedZoneError(f"{note}\n{e}", e.strays, e.count) from None
