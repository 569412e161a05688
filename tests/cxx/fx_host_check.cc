// tests/cxx/fx_host_check.cc -- the host forms of detail/fx.hpp (fx_step, fx_canon, fx_compose_host, fx_mask_one, fx_finish_col,
// fx_finish_one, fx_make_mask, fx_make_finish) over the five prime fields, Mont128 at 2^128 - 159 and at 2^127 - 1.  Two sources:
//   * the cases of the file named on the command line, one per line, written by tests/test_fx_host.py from the Python model:
//       <field> <B> <k> <shift> <x> <c> <rlow> <opened> <y> <status> <plane 0> .. <plane B-1>      integers in hex, counts decimal
//     c and rlow are the mask of x under the planes (which are elements, not only bits: p - 1 in every plane is among them); y and
//     the status are the finish of x and rlow under the value `opened` (which need not be c: values at and beyond 2^(B+1) are
//     among them).  Every word must be the line's.
//   * identities on this program's own operands: the lazy sum of B planes equals the sum of plane i times 2^i through the
//     field's own mul and add; finishing the c of true bits and an in-range x gives floor(x / 2^shift) or that plus one.
// Host only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "scl_hip/detail/fx.hpp"
using namespace sclhip;

#define CHECK_SEED 0x243F6A8885A308D3ull
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

// between an integer below p and the field's element
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

struct Case {
  std::string field;
  int B, k, shift, status;
  Int256 x, c, rlow, opened, y;
  std::vector<Int256> planes;
};

// one copy of the finish per field (everything below it is forced inline)
template <class F>
__attribute__((noinline)) static typename F::E finish(const typename F::Ctx& c, const FxFinish<F>& prm, const typename F::E& opened, const typename F::E& x,
                                                      const typename F::E& rlow, int& status) {
  const typename F::E cp = fx_finish_col<F>(c, prm, opened, status);
  return fx_finish_one<F>(c, prm, cp, status, x, rlow);
}

template <class F>
static void identities(const typename F::Ctx& c, const char* name, int top, long at) {
  typedef typename F::E E;
  const int B = 2 + (int)(next64() % (u64)(top - 1)), k = 2 + (int)(next64() % (u64)(B - 1)), shift = 1 + (int)(next64() % (u64)(k - 1));
  // the lazy sum against mul and add
  std::vector<E> planes;
  for (int i = 0; i < B; ++i) planes.push_back(i % 5 == 4 ? Gen<F>::top(c) : Gen<F>::rnd(c));
  E want = F::zero(), weight = F::one(c);
  for (int i = 0; i < B; ++i) {
    want = F::add(c, want, F::mul(c, planes[i], weight));
    weight = F::add(c, weight, weight);
  }
  check(F::eq(fx_compose_host<F>(c, planes.data(), 1, B), want), name, "the lazy sum is the weighted sum", at);
  // true bits and an in-range x: y is floor(x / 2^shift) or that plus one.  x = 2^(k-1) - 1 - (a small value), both signs
  const E one = F::one(c);
  std::vector<E> bits;
  for (int i = 0; i < B; ++i) bits.push_back((next64() & 1) ? one : F::zero());
  const u64 small = next64() % 1000;
  E pos = F::zero();
  for (u64 i = 0; i < small; ++i) pos = F::add(c, pos, one);       // `small`
  for (int sign = 0; sign < 2; ++sign) {
    const E x = sign ? F::sub(c, F::zero(), pos) : pos;             // small or -small: in range for k >= 11
    if (k < 11) break;
    const FxMask<F> mprm = fx_make_mask<F>(c, k);
    const FxFinish<F> fprm = fx_make_finish<F>(c, shift, B);
    const E r = fx_compose_host<F>(c, bits.data(), 1, B), rlow = fx_compose_host<F>(c, bits.data(), 1, shift);
    int st = -1;
    const E y = finish<F>(c, fprm, fx_mask_one<F>(c, mprm, x, r), x, rlow, st);
    check(st == FX_OK, name, "an honest c is in range", at);
    // floor(+-small / 2^shift) as an element
    const long long xs = sign ? -(long long)small : (long long)small;
    const long long fl = shift >= 62 ? (xs < 0 ? -1 : 0) : (xs >> shift);
    E lo = F::zero();
    for (long long i = 0; i < (fl < 0 ? -fl : fl); ++i) lo = F::add(c, lo, one);
    if (fl < 0) lo = F::sub(c, F::zero(), lo);
    check(F::eq(y, lo) || F::eq(y, F::add(c, lo, one)), name, "floor or floor + 1", at);
  }
}

template <class F>
static void run_field(const typename F::Ctx& c, const char* name, const std::vector<Case>& cases, int want_top) {
  typedef typename F::E E;
  const int top = fx_prime_bits<F>(c) - 2;
  check(top == want_top, name, "|p| - 2", top);
  long at = 0, mine = 0;
  for (const Case& k : cases) {
    if (k.field != name) continue;
    ++mine;
    std::vector<E> planes;
    for (const Int256& v : k.planes) planes.push_back(from_int<F>(c, v));
    const E x = from_int<F>(c, k.x);
    const E r = fx_compose_host<F>(c, planes.data(), 1, k.B), rlow = fx_compose_host<F>(c, planes.data(), 1, k.shift);
    check(same(to_int<F>(c, fx_mask_one<F>(c, fx_make_mask<F>(c, k.k), x, r)), k.c), name, "c against the model", at);
    check(same(to_int<F>(c, rlow), k.rlow), name, "rlow against the model", at);
    int st = -1;
    const E y = finish<F>(c, fx_make_finish<F>(c, k.shift, k.B), from_int<F>(c, k.opened), x, rlow, st);
    check(st == k.status, name, "status against the model", at);
    check(same(to_int<F>(c, y), k.y), name, "y against the model", at);
    ++at;
  }
  check(mine >= 20, name, "the file holds this field's cases", mine);
  for (int i = 0; i < 200; ++i) identities<F>(c, name, top, at++);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: fx_host_check <cases>\n");
    return 2;
  }
  std::vector<Case> cases;
  std::ifstream in(argv[1]);
  for (std::string line; std::getline(in, line);) {
    std::istringstream ls(line);
    Case k;
    std::string x, c, rlow, opened, y, plane;
    if (!(ls >> k.field >> k.B >> k.k >> k.shift >> x >> c >> rlow >> opened >> y >> k.status)) continue;
    k.x = parse_hex(x), k.c = parse_hex(c), k.rlow = parse_hex(rlow), k.opened = parse_hex(opened), k.y = parse_hex(y);
    while (ls >> plane) k.planes.push_back(parse_hex(plane));
    if ((int)k.planes.size() != k.B) {
      std::printf("a line with %zu planes for B = %d\n", k.planes.size(), k.B);
      return 2;
    }
    cases.push_back(k);
  }
  run_field<M61>(M61::Ctx{}, "m61", cases, 59);
  run_field<M127>(M127::Ctx{}, "m127", cases, 125);
  run_field<Mont128>(Mont128::make_ctx(~(u128)0 - 158), "mont128_p0", cases, 126);
  run_field<Mont128>(Mont128::make_ctx(((u128)1 << 127) - 1), "mont128_p1", cases, 125);
  run_field<Secp256k1Scalar>(Secp256k1Scalar::Ctx{}, "secp_scalar", cases, 254);
  run_field<Secp256k1Field>(Secp256k1Field::Ctx{}, "secp_field", cases, 254);
  return summary();
}
