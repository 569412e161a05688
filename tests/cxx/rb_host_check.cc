// tests/cxx/rb_host_check.cc -- the host forms of detail/rb.hpp (rb_sqrt_one, rb_bit_factor, rb_bit_one, rb_make_params) over the
// five prime fields, Mont128 at 2^128 - 159 (s = 5) and at 2^127 - 1 (s = 1).  Two sources:
//   * the cases of the file named on the command line, one per line, written by tests/test_rb_host.py from the fixture
//     (tests/golden/golden_rb.json) and the Python model:  <field> <a> <status> <even root> <its inverse>, integers in hex.  The
//     status must be the line's on every case (Euler's criterion on the model's side), the root and the inverse word for word.
//   * identities on every case and on this program's own uniform elements: root^2 == a, root inv == 1, the root's integer value
//     even (odd on request, the two roots negatives of each other), the root of 0 is 0 with status 1, a non-residue yields 0 and
//     status 2, a^((p-1)/2) decides the status; the bit finish (v r + 1) / 2 is 1 for r the even root of u and 0 for the odd one.
// Host only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "scl_hip/detail/rb.hpp"
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

// between an integer below p and the field's element
template <class F>
static typename F::E from_int(const typename F::Ctx& c, const Int256& v) {
  if constexpr (F::TAG == M61::TAG) return v.w[0];
  else if constexpr (F::TAG == M127::TAG) return ((u128)v.w[1] << 64) | v.w[0];
  else if constexpr (F::TAG == Mont128::TAG) return F::to_mont(c, ((u128)v.w[1] << 64) | v.w[0]);
  else return F::to_mont(c, F::make(v.w[0], v.w[1], v.w[2], v.w[3]));
}
template <class F>
static Int256 to_int(const typename F::Ctx& c, const typename F::E& e) {
  Int256 v = {{0, 0, 0, 0}};
  if constexpr (F::TAG == M61::TAG) {
    v.w[0] = e;
  } else if constexpr (F::TAG == M127::TAG) {
    v.w[0] = (u64)e, v.w[1] = (u64)(e >> 64);
  } else if constexpr (F::TAG == Mont128::TAG) {
    const u128 x = F::from_mont(c, e);
    v.w[0] = (u64)x, v.w[1] = (u64)(x >> 64);
  } else {
    const typename F::E x = F::from_mont(c, e);
    for (int i = 0; i < 4; ++i) v.w[i] = x.w[i];
  }
  return v;
}
static bool same(const Int256& a, const Int256& b) { return !std::memcmp(a.w, b.w, sizeof a.w); }

// one copy of each chain per field (everything below them is forced inline)
template <class F>
__attribute__((noinline)) static RbRoot<F> root_of(const typename F::Ctx& c, const RbParams<F>& prm, const typename F::E& a, bool odd) {
  return rb_sqrt_one<F>(c, prm, a, odd);
}
template <class F>
__attribute__((noinline)) static typename F::E factor_of(const typename F::Ctx& c, const RbParams<F>& prm, const typename F::E& u, int& status) {
  return rb_bit_factor<F>(c, prm, u, status);
}

template <class F>
static void identities(const typename F::Ctx& c, const RbParams<F>& prm, const char* name, const typename F::E& a, long at) {
  typedef typename F::E E;
  const E one = F::one(c);
  u64 p[4], euler[4];
  rb_prime<F>(c, p);
  p[0] &= ~(u64)1;
  for (int i = 0; i < 4; ++i) euler[i] = p[i];
  rb_shr1(euler);
  const RbRoot<F> even = root_of<F>(c, prm, a, false), odd = root_of<F>(c, prm, a, true);
  check(even.status == odd.status, name, "one status for both roots", at);
  if (F::is_zero(a)) {
    check(even.status == RB_ZERO && F::is_zero(even.root) && F::is_zero(even.inv) && F::is_zero(odd.root), name, "the root of zero", at);
    return;
  }
  const bool residue = F::eq(rb_pow_host<F>(c, a, euler), one);
  check(even.status == (residue ? RB_OK : RB_NONRESIDUE), name, "the status is Euler's criterion", at);
  int st = -1;
  const E h = factor_of<F>(c, prm, a, st);
  check(st == even.status, name, "the bit factor's status", at);
  if (!residue) {
    check(F::is_zero(even.root) && F::is_zero(even.inv) && F::is_zero(odd.root) && F::is_zero(odd.inv), name, "a non-residue yields zero", at);
    check(F::is_zero(rb_bit_one<F>(c, prm, h, st, a)), name, "a flagged column is zero", at);
    return;
  }
  check(F::eq(F::sqr(c, even.root), a) && F::eq(F::sqr(c, odd.root), a), name, "root^2 == a", at);
  check(F::eq(F::mul(c, even.root, even.inv), one) && F::eq(F::mul(c, odd.root, odd.inv), one), name, "root inv == 1", at);
  check(!(to_int<F>(c, even.root).w[0] & 1) && (to_int<F>(c, odd.root).w[0] & 1), name, "the parity of the roots", at);
  check(F::eq(F::neg(c, even.root), odd.root) && F::eq(F::neg(c, even.inv), odd.inv), name, "the roots are negatives", at);
  // the bit of r = the even root of u = a is 1, that of the odd root 0
  check(F::eq(rb_bit_one<F>(c, prm, h, st, even.root), one) && F::is_zero(rb_bit_one<F>(c, prm, h, st, odd.root)), name, "the bit finish", at);
}

struct Case {
  std::string field;
  Int256 a, root, inv;
  int status;
};

template <class F>
static void run_field(const typename F::Ctx& c, const char* name, const std::vector<Case>& cases, int want_s) {
  typedef typename F::E E;
  const RbParams<F> prm = rb_make_params<F>(c);
  check(prm.s == want_s && rb_s<F>(prm) == want_s, name, "s", prm.s);
  check(F::eq(F::add(c, prm.half, prm.half), F::one(c)), name, "2^-1", 0);
  long at = 0, mine = 0;
  for (const Case& k : cases) {
    if (k.field != name) continue;
    ++mine;
    const E a = from_int<F>(c, k.a);
    const RbRoot<F> r = root_of<F>(c, prm, a, false);
    check(r.status == k.status, name, "status against the model", at);
    check(same(to_int<F>(c, r.root), k.root), name, "root against the model", at);
    check(same(to_int<F>(c, r.inv), k.inv), name, "inverse root against the model", at);
    identities<F>(c, prm, name, a, at++);
  }
  check(mine >= 69, name, "the file holds this field's cases", mine);
  for (const E& a : Gen<F>::pool(c)) identities<F>(c, prm, name, a, at++);
  for (int i = 0; i < 64; ++i) identities<F>(c, prm, name, Gen<F>::rnd(c), at++);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: rb_host_check <cases>\n");
    return 2;
  }
  std::vector<Case> cases;
  std::ifstream in(argv[1]);
  std::string field, a, root, inv;
  int status;
  while (in >> field >> a >> status >> root >> inv) cases.push_back({field, parse_hex(a), parse_hex(root), parse_hex(inv), status});
  run_field<M61>(M61::Ctx{}, "m61", cases, 1);
  run_field<M127>(M127::Ctx{}, "m127", cases, 1);
  run_field<Mont128>(Mont128::make_ctx(~(u128)0 - 158), "mont128_p0", cases, 5);
  run_field<Mont128>(Mont128::make_ctx(((u128)1 << 127) - 1), "mont128_p1", cases, 1);
  run_field<Secp256k1Scalar>(Secp256k1Scalar::Ctx{}, "secp_scalar", cases, 6);
  run_field<Secp256k1Field>(Secp256k1Field::Ctx{}, "secp_field", cases, 1);
  return summary();
}
