// tests/cxx/launch_rules_check.cc -- csrc/launch_rules.hpp as a host program: grid_cap against the four grid rules it replaced
// (written out here as they stood), mfma_shape against the expression the three matrix-core dispatchers repeated, dispatch_int /
// dispatch_of on every value and on the misses around them, residency_pad at the triples the launchers pass (values recorded
// from the function before it moved).  Prints "<n> checks, <k> mismatches"; tests/test_launch_rules.py builds and runs it plain
// and under -fsanitize=address,undefined.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../secure-computation-library_amd/csrc/launch_rules.hpp"

using namespace sclhip;

namespace {
long checks = 0, mismatches = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    ++checks;                                               \
    if (!(cond)) {                                          \
      ++mismatches;                                         \
      std::printf("line %d: %s\n", __LINE__, #cond);        \
    }                                                       \
  } while (0)

// kernels.hpp's constants, as numbers
constexpr int BLOCK = 256, ABLOCK = 1024, AES_GRID_CAP = 256 * 4, AES4_GRID_CAP = 256;

// the four rules as capi.hip spelled them; `knob` is "max_blocks" for the first two and "aes_blocks" for the others
unsigned old_grid_for(size_t work_items, long knob) {
  size_t blocks = (work_items + BLOCK - 1) / BLOCK;
  long cap = knob;
  if (cap <= 0) cap = 0x7fffffff;
  if (blocks > (size_t)cap) blocks = (size_t)cap;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}
unsigned old_grid_for_block(size_t work_items, int block, long knob) {
  size_t blocks = (work_items + block - 1) / block;
  long cap = knob;
  if (cap <= 0) cap = 0x7fffffff;
  if (blocks > (size_t)cap) blocks = (size_t)cap;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}
unsigned old_grid_aes(size_t work_items, long knob) {
  size_t blocks = (work_items + BLOCK - 1) / BLOCK;
  long cap = knob;
  if (cap <= 0) cap = AES_GRID_CAP;
  if (blocks > (size_t)cap) blocks = (size_t)cap;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}
unsigned old_grid_aes4(size_t work_items, long knob) {
  size_t blocks = (work_items + ABLOCK - 1) / ABLOCK;
  long cap = knob;
  if (cap <= 0) cap = AES4_GRID_CAP;
  if (blocks > (size_t)cap) blocks = (size_t)cap;
  if (blocks == 0) blocks = 1;
  return (unsigned)blocks;
}

std::vector<size_t> works(size_t block) { return {0, 1, block - 1, block, block + 1, ((size_t)1 << 31) * block + 1}; }

void check_grids() {
  // knobs: 0 (not set: the rule's default), 1, the default itself, and -1 (not set either)
  for (long knob : {0L, 1L, 0x7fffffffL, -1L}) {
    for (size_t w : works(BLOCK)) EXPECT(grid_cap(w, BLOCK, knob) == old_grid_for(w, knob));
    for (int block : {1, 64})
      for (size_t w : works((size_t)block)) EXPECT(grid_cap(w, block, knob) == old_grid_for_block(w, block, knob));
  }
  // (as capi.hip's grid_aes / grid_aes4 call it: the knob where it is set, their own default elsewhere)
  for (long knob : {0L, 1L, (long)AES_GRID_CAP, -1L})
    for (size_t w : works(BLOCK)) EXPECT(grid_cap(w, BLOCK, knob > 0 ? knob : AES_GRID_CAP) == old_grid_aes(w, knob));
  for (long knob : {0L, 1L, (long)AES4_GRID_CAP, -1L})
    for (size_t w : works(ABLOCK)) EXPECT(grid_cap(w, ABLOCK, knob > 0 ? knob : AES4_GRID_CAP) == old_grid_aes4(w, knob));
  // the defaults as numbers: no cap below 2^31 - 1 blocks, 1024 and 256 blocks for the PRG kernels, never an empty grid
  EXPECT(grid_cap(((size_t)1 << 31) * BLOCK + 1, BLOCK, 0) == 0x7fffffffu);
  EXPECT(grid_cap((size_t)1 << 40, BLOCK, AES_GRID_CAP) == 1024u);
  EXPECT(grid_cap((size_t)1 << 40, ABLOCK, AES4_GRID_CAP) == 256u);
  EXPECT(grid_cap(0, BLOCK, 0) == 1u);
}

void check_mfma_shape() {
  for (size_t rows = 1; rows <= 128; ++rows)
    for (size_t k = 1; k <= 64; ++k) {
      const int KS = k <= 32 ? 1 : 2;
      const int MT = (rows <= 32 && KS == 1) ? 1 : rows <= 64 ? 2 : 4;
      const MfmaShape s = mfma_shape(rows, k);
      EXPECT(s.KS == KS && s.MT == MT);
      const int pair = s.KS * 10 + s.MT;
      EXPECT(pair == 11 || pair == 12 || pair == 14 || pair == 22 || pair == 24);
    }
}

// every value of `hits` calls fn once with that value and returns true; every value of `misses` calls nothing and returns false
template <class Dispatch>
void check_dispatch(Dispatch&& dispatch, std::initializer_list<int> hits, std::initializer_list<int> misses) {
  for (int v : hits) {
    int calls = 0, got = -1;
    const bool found = dispatch(v, [&](int V) { ++calls, got = V; });
    EXPECT(found && calls == 1 && got == v);
  }
  for (int v : misses) {
    int calls = 0;
    const bool found = dispatch(v, [&](int) { ++calls; });
    EXPECT(!found && calls == 0);
  }
}

void check_dispatches() {
  // the value reaches fn as a compile-time constant: the lambdas hand it on as decltype(c)::value
  check_dispatch([](int v, auto&& fn) { return dispatch_int<1, 7>(v, [&](auto c) { fn(decltype(c)::value); }); }, {1, 2, 3, 4, 5, 6, 7},
                 {0, 8, -1, 1 << 20});
  check_dispatch([](int v, auto&& fn) { return dispatch_int<5, 16>(v, [&](auto c) { fn(decltype(c)::value); }); },
                 {5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, {4, 17, 0});
  check_dispatch([](int v, auto&& fn) { return dispatch_of<8, 16, 32, 64, 128>(v, [&](auto c) { fn(decltype(c)::value); }); },
                 {8, 16, 32, 64, 128}, {7, 129, 24, 48, 0, 256});
  check_dispatch([](int v, auto&& fn) { return dispatch_of<1, 2, 4>(v, [&](auto c) { fn(decltype(c)::value); }); }, {1, 2, 4}, {0, 3, 5});
}

void check_residency_pad() {
  // (waves, block, static LDS, dynamic LDS): k_recover_fixed / k_recover_small pass 10 and 12 with no static LDS, the small-node
  // share kernels 9, 12 and 16 (and 14 under "share_waves128") beside sizeof(u32) * SmallVdm::CAP = 2048 bytes of their own
  static const struct {
    long waves;
    int block;
    size_t static_lds, pad;
  } rows[] = {{9, 64, 0, 17920},  {9, 64, 2048, 15872},  {10, 64, 0, 15360}, {10, 64, 2048, 13312}, {12, 64, 0, 12800},
              {12, 64, 2048, 10752}, {14, 64, 0, 11264}, {14, 64, 2048, 9216}, {16, 64, 0, 10240}, {16, 64, 2048, 8192}};
  for (const auto& r : rows) EXPECT(residency_pad(r.waves, r.block, r.static_lds) == r.pad);
  EXPECT(residency_pad(0, 64, 0) == 0 && residency_pad(-1, 64, 0) == 0);  // no cap asked for
}
}  // namespace

int main() {
  check_grids();
  check_mfma_shape();
  check_dispatches();
  check_residency_pad();
  std::printf("%ld checks, %ld mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
