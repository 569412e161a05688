// include/scl_hip/util/sha256.h -- scl::util::Sha256 (include/scl/util/sha256.h:33-67, src/scl/util/sha256.cc): SHA-256 with
// the IUF interface, on the host, per call -- as the reference runs it.  Written from FIPS 180-4; header only.  Batches of
// messages and whole trees are hashed on the device by scl_hip_sha256 / scl_hip_merkle_* (csrc/sha256.hpp).
#ifndef SCL_HIP_UTIL_SHA256_H
#define SCL_HIP_UTIL_SHA256_H

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "digest.h"
#include "iuf_hash.h"

namespace scl::util {

class Sha256 final : public IUFHash<Sha256> {
 public:
  using DigestType = Digest<256>;

  /// absorb n bytes
  void hash(const unsigned char* bytes, std::size_t n) {
    m_length += n;
    while (n) {
      const std::size_t take = n < 64 - m_fill ? n : 64 - m_fill;
      std::memcpy(m_block.data() + m_fill, bytes, take);
      m_fill += take, bytes += take, n -= take;
      if (m_fill == 64) {
        compress();
        m_fill = 0;
      }
    }
  }

  /// pad (0x80, zeros, the bit length as 64 big-endian bits) and emit the state, big-endian
  DigestType write() {
    const std::uint64_t bits = static_cast<std::uint64_t>(m_length) * 8;
    m_block[m_fill++] = 0x80;
    if (m_fill > 56) {
      std::memset(m_block.data() + m_fill, 0, 64 - m_fill);
      compress();
      m_fill = 0;
    }
    std::memset(m_block.data() + m_fill, 0, 56 - m_fill);
    for (int i = 0; i < 8; ++i) m_block[56 + i] = static_cast<unsigned char>(bits >> (56 - 8 * i));
    compress();
    m_fill = 0;
    DigestType out;
    for (int i = 0; i < 8; ++i)
      for (int b = 0; b < 4; ++b) out[4 * i + b] = static_cast<unsigned char>(m_state[i] >> (24 - 8 * b));
    return out;
  }

 private:
  static std::uint32_t rotr(std::uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

  void compress() {
    static constexpr std::uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    std::uint32_t w[64];
    for (int t = 0; t < 16; ++t)
      w[t] = (std::uint32_t(m_block[4 * t]) << 24) | (std::uint32_t(m_block[4 * t + 1]) << 16) |
             (std::uint32_t(m_block[4 * t + 2]) << 8) | std::uint32_t(m_block[4 * t + 3]);
    for (int t = 16; t < 64; ++t) {
      const std::uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
      const std::uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
      w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    std::uint32_t v[8];
    for (int i = 0; i < 8; ++i) v[i] = m_state[i];
    for (int t = 0; t < 64; ++t) {
      const std::uint32_t S1 = rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25), ch = (v[4] & v[5]) ^ (~v[4] & v[6]);
      const std::uint32_t S0 = rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22), mj = (v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]);
      const std::uint32_t t1 = v[7] + S1 + ch + K[t] + w[t], t2 = S0 + mj;
      for (int i = 7; i > 0; --i) v[i] = v[i - 1];
      v[4] += t1;
      v[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) m_state[i] += v[i];
  }

  std::array<unsigned char, 64> m_block{};
  std::size_t m_fill = 0;
  std::size_t m_length = 0;
  std::array<std::uint32_t, 8> m_state = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                          0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
};

}  // namespace scl::util

#endif  // SCL_HIP_UTIL_SHA256_H
