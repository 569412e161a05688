// tests/cxx/cmp_host_check.cc -- the host forms of detail/cmp.hpp (cmp_levels, cmp_planes, cmp_open_col, cmp_leaf, cmp_combine_lt,
// cmp_combine_eq, cmp_make_finish, cmp_finish_one) over the five prime fields, Mont128 at 2^128 - 159 and at 2^127 - 1, against
// the cases of the file named on the command line, written by tests/test_cmp_host.py from the Python model, one per line
// (integers in hex, counts decimal):
//   pair   <field> <w> <B> <opened> <cmod> <status> <j> <has_hi> <b_lo> <b_hi> <r_lt> <r_eq> <d_lt> <d_eq>
//       the opening's column part, then pair j of the first level: the leaves of the bits 2j and 2j + 1 from the shares b_lo and
//       b_hi (no partner: the identity), combined, + r2
//   level  <field> <has_hi> <lt_lo> <eq_lo> <lt_hi> <eq_hi> <r_lt> <r_eq> <d_lt> <d_eq>
//   finish <field> <w> <what> <cmod> <status> <lt> <rlow> <x> <y>
//   count  <w> <levels> <planes>
// Every word must be the line's.  Host only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "scl_hip/detail/cmp.hpp"
using namespace sclhip;

#define CHECK_SEED 0x13198A2E03707344ull
#include "check.hpp"

struct Int256 {
  u64 w[4];
};

static Int256 parse_hex(const std::string& s) {
  Int256 v = {{0, 0, 0, 0}};
  int bit = 0;
  for (std::size_t i = s.size(); i-- > 0 && bit < 256; bit += 4) {
    const char ch = s[i];
    const u64 d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : ch - 'A' + 10;
    v.w[bit >> 6] |= d << (bit & 63);
  }
  return v;
}

template <class F>
static typename F::E from_int(const typename F::Ctx& c, const Int256& v) {
  u64 w[F::LIMBS];
  for (int i = 0; i < (int)F::LIMBS; ++i) w[i] = v.w[i];
  return fx_from_limbs<F>(c, w);
}
template <class F>
static Int256 to_int(const typename F::Ctx& c, const typename F::E& e) {
  Int256 v = {{0, 0, 0, 0}};
  u64 w[F::LIMBS];
  fx_limbs<F>(c, e, w);
  for (int i = 0; i < (int)F::LIMBS; ++i) v.w[i] = w[i];
  return v;
}
static bool same(const Int256& a, const Int256& b) { return !std::memcmp(a.w, b.w, sizeof a.w); }

struct Line {
  std::string kind, field;
  std::vector<std::string> words;
};

template <class F>
static void run_field(const typename F::Ctx& c, const char* name, const std::vector<Line>& lines) {
  typedef typename F::E E;
  long at = 0, pairs = 0, levels = 0, finishes = 0;
  for (const Line& ln : lines) {
    if (ln.field != name) continue;
    const std::vector<std::string>& a = ln.words;
    auto num = [&](int i) { return std::atoi(a[i].c_str()); };
    auto el = [&](int i) { return from_int<F>(c, parse_hex(a[i])); };
    if (ln.kind == "pair" && a.size() == 13) {
      const int w = num(0), B = num(1), j = num(5), has_hi = num(6);
      u64 cw[F::LIMBS];
      int st = -1;
      const E cmod = cmp_open_col<F>(c, fx_make_finish<F>(c, w, B), el(2), cw, st);
      check(st == num(4), name, "status against the model", at);
      check(same(to_int<F>(c, cmod), parse_hex(a[3])), name, "cmod against the model", at);
      E lt_lo, eq_lo, lt_hi = F::zero(), eq_hi = F::one(c);
      cmp_leaf<F>(c, cmp_bit_mask(cw[(2 * j) >> 6], 2 * j), el(7), lt_lo, eq_lo);
      if (has_hi) cmp_leaf<F>(c, cmp_bit_mask(cw[(2 * j + 1) >> 6], 2 * j + 1), el(8), lt_hi, eq_hi);
      check(same(to_int<F>(c, cmp_combine_lt<F>(c, lt_hi, eq_hi, lt_lo, el(9))), parse_hex(a[11])), name, "first level lt against the model", at);
      check(same(to_int<F>(c, cmp_combine_eq<F>(c, eq_hi, eq_lo, el(10))), parse_hex(a[12])), name, "first level eq against the model", at);
      ++pairs;
    } else if (ln.kind == "level" && a.size() == 9) {
      const int has_hi = num(0);
      const E lt_hi = has_hi ? el(3) : F::zero(), eq_hi = has_hi ? el(4) : F::one(c);
      check(same(to_int<F>(c, cmp_combine_lt<F>(c, lt_hi, eq_hi, el(1), el(5))), parse_hex(a[7])), name, "level lt against the model", at);
      check(same(to_int<F>(c, cmp_combine_eq<F>(c, eq_hi, el(2), el(6))), parse_hex(a[8])), name, "level eq against the model", at);
      ++levels;
    } else if (ln.kind == "finish" && a.size() == 8) {
      const E y = cmp_finish_one<F>(c, cmp_make_finish<F>(c, num(0), num(1)), el(2), num(3), el(4), el(5), el(6));
      check(same(to_int<F>(c, y), parse_hex(a[7])), name, "finish against the model", at);
      ++finishes;
    } else {
      check(false, name, "a line this program does not know", at);
    }
    ++at;
  }
  check(pairs >= 20 && levels >= 4 && finishes >= 12, name, "the file holds this field's cases", at);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: cmp_host_check <cases>\n");
    return 2;
  }
  std::vector<Line> lines;
  std::ifstream in(argv[1]);
  long counts = 0;
  for (std::string line; std::getline(in, line);) {
    std::istringstream ls(line);
    Line ln;
    if (!(ls >> ln.kind)) continue;
    if (ln.kind == "count") {
      std::size_t w = 0, levels = 0, planes = 0;
      ls >> w >> levels >> planes;
      check(cmp_levels(w) == levels && cmp_planes(w) == planes, "counts", "levels and planes against the model", (long)w);
      ++counts;
      continue;
    }
    ls >> ln.field;
    for (std::string word; ls >> word;) ln.words.push_back(word);
    lines.push_back(ln);
  }
  check(counts >= 20, "counts", "the file holds the counts", counts);
  static_assert(cmp_planes(59) == 119 && cmp_levels(59) == 6 && cmp_planes(1) == 1 && cmp_levels(1) == 1, "the counts of the header");
  run_field<M61>(M61::Ctx{}, "m61", lines);
  run_field<M127>(M127::Ctx{}, "m127", lines);
  run_field<Mont128>(Mont128::make_ctx(~(u128)0 - 158), "mont128_p0", lines);
  run_field<Mont128>(Mont128::make_ctx(((u128)1 << 127) - 1), "mont128_p1", lines);
  run_field<Secp256k1Scalar>(Secp256k1Scalar::Ctx{}, "secp_scalar", lines);
  run_field<Secp256k1Field>(Secp256k1Field::Ctx{}, "secp_field", lines);
  return summary();
}
