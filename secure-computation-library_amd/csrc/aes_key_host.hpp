// csrc/aes_key_host.hpp -- the AES-128 key schedule of the reference's PRG on the host: the one piece of host code on which
// bit-exactness against the reference rests, defined once for the engine (capi.hip) and every extension unit
// (unit_host.hpp), and checked without a GPU by tests/cxx/aes_key_check.hip.  Host code only, in an anonymous namespace: the
// header is included once per translation unit.
#pragma once

#include <cstring>

#include "kernels.hpp"  // AesKey, aes_key_round1

namespace {

// The S-box from its definition (FIPS-197): the inverse in GF(2^8) through the logarithms to the generator 3, then the affine
// map.
struct Sbox {
  unsigned char s[256];
  Sbox() {
    auto xt = [](unsigned a) { return ((a << 1) ^ ((a & 0x80) ? 0x11b : 0)) & 0xff; };
    unsigned char ex[256], lg[256] = {0};
    unsigned v = 1;
    for (int i = 0; i < 255; ++i) {
      ex[i] = (unsigned char)v;
      lg[v] = (unsigned char)i;
      v ^= xt(v);  // v * 3
    }
    for (int x = 0; x < 256; ++x) {
      const unsigned inv = x ? ex[(255 - lg[x]) % 255] : 0;
      unsigned r = inv, rot = inv;
      for (int i = 0; i < 4; ++i) {
        rot = ((rot << 1) | (rot >> 7)) & 0xff;
        r ^= rot;
      }
      s[x] = (unsigned char)(r ^ 0x63);
    }
  }
};

// The round keys (prg.cc:88-101: key = the seed zero-padded or truncated to 16 bytes) and the T-table the kernels replicate in
// LDS: te0[x] = (2S, S, S, 3S) from byte 0 up, S = sbox[x].
void make_aes_key(const unsigned char* seed, size_t seed_len, sclhip::AesKey& k) {
  using sclhip::u32;
  static const Sbox sb;
  unsigned char rk[176] = {0};
  if (seed) std::memcpy(rk, seed, seed_len > 16 ? 16 : seed_len);
  unsigned rcon = 1;
  for (int i = 16; i < 176; i += 4) {
    unsigned char w[4] = {rk[i - 4], rk[i - 3], rk[i - 2], rk[i - 1]};
    if (i % 16 == 0) {
      const unsigned char w0 = w[0];
      w[0] = (unsigned char)(sb.s[w[1]] ^ rcon);
      w[1] = sb.s[w[2]];
      w[2] = sb.s[w[3]];
      w[3] = sb.s[w0];
      rcon = ((rcon << 1) ^ ((rcon & 0x80) ? 0x11b : 0)) & 0xff;
    }
    for (int j = 0; j < 4; ++j) rk[i + j] = (unsigned char)(rk[i - 16 + j] ^ w[j]);
  }
  for (int w = 0; w < 44; ++w)
    k.rk[w] = (u32)rk[4 * w] | ((u32)rk[4 * w + 1] << 8) | ((u32)rk[4 * w + 2] << 16) | ((u32)rk[4 * w + 3] << 24);
  for (int x = 0; x < 256; ++x) {
    const unsigned s = sb.s[x], s2 = ((s << 1) ^ ((s & 0x80) ? 0x11b : 0)) & 0xff, s3 = s2 ^ s;
    k.te0[x] = s2 | (s << 8) | (s << 16) | (s3 << 24);
  }
  sclhip::aes_key_round1(k);
}

}  // namespace
