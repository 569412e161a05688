// include/scl_hip/util/bitmap.h -- scl::util::Bitmap (include/scl/util/bitmap.h:36-214): bits packed into bytes, bit i in
// byte i / 8 at position i % 8; a bitmap of no bits still owns one byte, as there.  Its wire image is that of its byte vector.
// A Merkle proof's directions are one: the low `depth` bits of the leaf index, little-endian (scl_hip_merkle_paths).
#ifndef SCL_HIP_UTIL_BITMAP_H
#define SCL_HIP_UTIL_BITMAP_H

#include <bitset>
#include <cstddef>
#include <ostream>
#include <stdexcept>
#include <vector>

#include "../serialization/serializer.h"

namespace scl {
namespace util {

class Bitmap {
 public:
  using BlockType = unsigned char;
  static constexpr std::size_t BITS_PER_BLOCK = 8 * sizeof(BlockType);

  static Bitmap fromStdVecBool(const std::vector<bool>& bits) {
    Bitmap bm(bits.size());
    for (std::size_t i = 0; i < bits.size(); ++i) bm.set(i, bits[i]);
    return bm;
  }
  /// the low `nbits` bits of an integer, bit i of the value = bit i of the map
  static Bitmap fromIndex(std::size_t value, std::size_t nbits) {
    Bitmap bm(nbits);
    for (std::size_t i = 0; i < nbits; ++i) bm.set(i, i < 8 * sizeof(value) && ((value >> i) & 1));
    return bm;
  }

  Bitmap(std::size_t nbits) : m_blocks(nbits == 0 ? 1 : (nbits + BITS_PER_BLOCK - 1) / BITS_PER_BLOCK, 0) {}
  Bitmap() : Bitmap(0) {}

  bool at(std::size_t i) const { return (m_blocks[i / BITS_PER_BLOCK] >> (i % BITS_PER_BLOCK)) & 1; }
  void set(std::size_t i, bool b) {
    const BlockType mask = static_cast<BlockType>(1u << (i % BITS_PER_BLOCK));
    BlockType& blk = m_blocks[i / BITS_PER_BLOCK];
    blk = static_cast<BlockType>(b ? (blk | mask) : (blk & ~mask));
  }
  std::size_t count() const {
    std::size_t ones = 0;
    for (BlockType b : m_blocks) ones += std::bitset<BITS_PER_BLOCK>(b).count();
    return ones;
  }
  std::size_t numberOfBlocks() const { return m_blocks.size(); }

  friend bool operator==(const Bitmap& a, const Bitmap& b) { return a.m_blocks == b.m_blocks; }
  friend bool operator!=(const Bitmap& a, const Bitmap& b) { return !(a == b); }
  friend std::ostream& operator<<(std::ostream& os, const Bitmap& bm) {
    for (BlockType b : bm.m_blocks) os << std::bitset<BITS_PER_BLOCK>(b);
    return os;
  }
  friend Bitmap operator^(const Bitmap& a, const Bitmap& b) {
    return combine(a, b, [](BlockType x, BlockType y) { return static_cast<BlockType>(x ^ y); });
  }
  friend Bitmap operator&(const Bitmap& a, const Bitmap& b) {
    return combine(a, b, [](BlockType x, BlockType y) { return static_cast<BlockType>(x & y); });
  }
  friend Bitmap operator|(const Bitmap& a, const Bitmap& b) {
    return combine(a, b, [](BlockType x, BlockType y) { return static_cast<BlockType>(x | y); });
  }
  friend Bitmap operator~(const Bitmap& a) {
    Bitmap out = a;
    for (BlockType& b : out.m_blocks) b = static_cast<BlockType>(~b);
    return out;
  }

 private:
  template <typename OP>
  static Bitmap combine(const Bitmap& a, const Bitmap& b, OP op) {
    if (a.numberOfBlocks() != b.numberOfBlocks()) throw std::logic_error("bitmaps are different sizes");
    Bitmap out = a;
    for (std::size_t i = 0; i < out.m_blocks.size(); ++i) out.m_blocks[i] = op(a.m_blocks[i], b.m_blocks[i]);
    return out;
  }
  std::vector<BlockType> m_blocks;
  friend struct seri::Serializer<Bitmap, void>;
};

}  // namespace util

namespace seri {
template <>
struct Serializer<util::Bitmap, void> {
  using Blocks = Serializer<std::vector<util::Bitmap::BlockType>>;
  static std::size_t sizeOf(const util::Bitmap& bm) { return Blocks::sizeOf(bm.m_blocks); }
  static std::size_t write(const util::Bitmap& bm, unsigned char* buf) { return Blocks::write(bm.m_blocks, buf); }
  static std::size_t read(util::Bitmap& bm, const unsigned char* buf) { return Blocks::read(bm.m_blocks, buf); }
};
}  // namespace seri
}  // namespace scl

#endif  // SCL_HIP_UTIL_BITMAP_H
