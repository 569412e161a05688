"""Generate golden_gf2_128_gmac.json: GMAC tags computed by the `openssl` command-line tool, the external pin of GF(2^128).

GHASH (McGrew & Viega, "The Galois/Counter Mode of Operation") is Horner evaluation at H = E_K(0^128) in GF(2)[x] / (x^128 +
x^7 + x^2 + x + 1), this project's GF(2^128), with each 16-byte block's bits reversed.  A GMAC tag over an AAD of m whole
blocks A_1..A_m under the 96-bit IV is tag = E_K(J0) xor GHASH_H(A_1, .., A_m, L), J0 = IV || 0^31 1, L = (8 len(A)) << 64.
So GHASH = tag xor E_K(J0) is the value at refl(H) of the polynomial c_1 x + .. + c_{m+1} x^{m+1}, c_1 = refl(L) and
c_{k+1} = refl(A_{m+1-k}): every tag is an externally computed evaluation of a polynomial whose coefficients are the AAD.

Run on a build machine with openssl (standard library only, nothing of the engine); no test runs it.  Every key, IV and AAD
comes from SEED, so a rerun with the same openssl writes the same file byte for byte.  Stored are the tools' raw outputs:
H and E_K(J0) from `openssl enc -aes-128-ecb -nopad`, each tag from `openssl mac ... GMAC`.

Sets:
  grid   24 keys x 64 AADs of 1..16 blocks in cycle (edge blocks: zero, all ones, only the first bit, only the last bit, a key's H)
  long    4 keys x AADs of 32, 47, 63, 64, 100, 127 blocks (deep Horner chains)
  nodes 136 keys x 4 AADs of 1..3 blocks (polynomials of degree <= 4: reconstruction from many external nodes)
"""
import json
import os
import random
import subprocess
import tempfile

SEED = 0x6D4D4143  # "mMAC"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_gf2_128_gmac.json")


def openssl(args, data=None):
    return subprocess.run(["openssl"] + args, input=data, capture_output=True, check=True).stdout


def aes_blocks(key: bytes, iv: bytes):
    """(H, E_K(J0)) from one two-block ECB encryption of 0^128 || IV || 0^31 1"""
    out = openssl(["enc", "-aes-128-ecb", "-K", key.hex(), "-nopad"], bytes(16) + iv + b"\x00\x00\x00\x01")
    assert len(out) == 32
    return out[:16], out[16:]


def gmac(key: bytes, iv: bytes, aad: bytes, tmp: str) -> bytes:
    with open(tmp, "wb") as fh:
        fh.write(aad)
    tag = openssl(["mac", "-cipher", "AES-128-GCM", "-macopt", "hexkey:" + key.hex(), "-macopt", "hexiv:" + iv.hex(),
                   "-in", tmp, "GMAC"]).decode().strip()
    assert len(tag) == 32
    return bytes.fromhex(tag)


def make_keys(rng, n):
    keys = []
    for _ in range(n):
        key, iv = rng.randbytes(16), rng.randbytes(12)
        h, ekj0 = aes_blocks(key, iv)
        keys.append({"key": key, "iv": iv, "h": h, "ekj0": ekj0})
    return keys


def make_set(keys, aads, tmp):
    return {
        "keys": [{k: v.hex() for k, v in key.items()} for key in keys],
        "aads": [a.hex() for a in aads],
        # tags[j][s]: key j, AAD s
        "tags": [[gmac(key["key"], key["iv"], a, tmp).hex() for a in aads] for key in keys],
    }


def main():
    rng = random.Random(SEED)
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "aad.bin")

        keys = make_keys(rng, 24)
        edges = [bytes(16), b"\xff" * 16, b"\x80" + bytes(15), bytes(15) + b"\x01", keys[5]["h"]]
        aads = []
        for s in range(64):
            blocks = []
            for b in range(s % 16 + 1):
                r = rng.random()
                blocks.append(edges[rng.randrange(len(edges))] if r < 0.3 else rng.randbytes(16))
            aads.append(b"".join(blocks))
        # every edge block at the first and at the last position of some AAD
        for i, e in enumerate(edges):
            aads[16 + i] = e + aads[16 + i][16:]
            aads[31 - i] = aads[31 - i][:-16] + e
        grid = make_set(keys, aads, tmp)

        keys = make_keys(rng, 4)
        long_ = make_set(keys, [rng.randbytes(16 * m) for m in (32, 47, 63, 64, 100, 127)], tmp)

        keys = make_keys(rng, 136)
        nodes = make_set(keys, [rng.randbytes(16 * m) for m in (1, 2, 3, 3)], tmp)

    doc = {
        "generator": "tests/golden/make_golden_gmac.py",
        "seed": SEED,
        "openssl_version": openssl(["version"]).decode().strip(),
        "sets": {"grid": grid, "long": long_, "nodes": nodes},
    }
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
