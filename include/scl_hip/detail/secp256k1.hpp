// include/scl_hip/detail/secp256k1.hpp -- the group of secp256k1 (y^2 = x^3 + 7 over Secp256k1Field), host and device.
//
// Replaces the point functions of math::EC<Secp256k1> (include/scl/math/ec.h, src/scl/math/curves/secp256k1_curve.cc:41-431):
// a point is (X : Y : Z) in homogeneous projective coordinates over Mont256<SecpFieldParams>, each coordinate four limbs in
// Montgomery form -- the reference's in-memory point --, infinity is (0 : 1 : 0).  Addition, mixed addition and doubling are
// the complete formulas for a = 0 of Renes, Costello and Batina, "Complete addition formulas for prime order elliptic
// curves" (EUROCRYPT 2016), algorithms 7, 8 and 9, written here from the paper's closed forms: with b3 = 3 b = 21 and
//     xx = X1 X2, yy = Y1 Y2, zz = Z1 Z2, xy = X1 Y2 + X2 Y1, yz = Y1 Z2 + Y2 Z1, xz = X1 Z2 + X2 Z1,
//     m = 3 xx, s = yy + b3 zz, d = yy - b3 zz, u = b3 xz:
//     X3 = xy d - yz u,   Y3 = d s + u m,   Z3 = s yz + m xy.
// They have no exceptional inputs (P = Q, P = -Q and infinity on either side included), so no lane branches on its data.
// Multiplication counts (field products M, products by the constant 21 as `c`, which are eight 32-bit multiply-adds and a fold,
// not a Montgomery product): add 12 M + 2 c, mixed add (Z2 = 1) 11 M + 2 c, dbl 8 M + 1 c (squares counted as M:
// Mont256::sqr is mul), equality 4 M, to affine 1 inversion (270 M: 255 squares, 15 products) + 2 M.
//
// This header is new with the Feldman entry points and is deliberately not part of field.hpp.  Its last section is what ECDSA
// adds: the scalar field's inversion, the conversion function and the per-lane window ladder (csrc/ecdsa_unit.hip).
#pragma once
#include "field.hpp"

namespace sclhip {
namespace secp {

typedef Secp256k1Field FQ;   // coordinates
typedef Secp256k1Scalar FR;  // scalars (the group order)
typedef U256 Fe;

struct Point {
  Fe X, Y, Z;
};
struct Affine {
  Fe x, y;
};
enum { POINT_LIMBS = 12, AFFINE_LIMBS = 8, WIRE_BYTES = 65, WINDOWS = 64, WINDOW_ENTRIES = 15, MUL_TABLE_ENTRIES = 16 };
// ec::toBytes / fromBytes flag bits (secp256k1_curve.cc:328-339)
enum { FLAG_FULL_POINT = 0x04, FLAG_INFINITY = 0x02 };

SCL_HD Fe fadd(const Fe& a, const Fe& b) { return FQ::add(FQ::Ctx{}, a, b); }
SCL_HD Fe fsub(const Fe& a, const Fe& b) { return FQ::sub(FQ::Ctx{}, a, b); }
SCL_HD Fe fmul(const Fe& a, const Fe& b) { return FQ::mul(FQ::Ctx{}, a, b); }
SCL_HD Fe fsqr(const Fe& a) { return FQ::mul(FQ::Ctx{}, a, a); }
SCL_HD Fe fone() { return FQ::one(FQ::Ctx{}); }
// a * 21: a residue in Montgomery form times a plain integer stays in Montgomery form (Mont256::muladd_small)
SCL_HD Fe fmul_b3(const Fe& a) { return FQ::muladd_small(FQ::Ctx{}, a, 21u, FQ::zero()); }
SCL_HD Fe fselect(bool take, const Fe& a, const Fe& b) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.w[i] = take ? a.w[i] : b.w[i];
  return r;
}

SCL_HD Point pt_infinity() { return Point{FQ::zero(), fone(), FQ::zero()}; }
SCL_HD Point pt_generator() {  // secp256k1_curve.cc:105-117, in Montgomery form
  return Point{FQ::make(0xD7362E5A487E2097ull, 0x231E295329BC66DBull, 0x979F48C033FD129Cull, 0x9981E643E9089F48ull),
               FQ::make(0xB15EA6D2D3DBABE2ull, 0x8DFC5D5D1F1DC64Dull, 0x70B6B59AAC19C136ull, 0xCF3F851FD4A582D6ull), fone()};
}
SCL_HD bool pt_is_infinity(const Point& p) { return FQ::is_zero(p.Z); }
SCL_HD Point pt_select(bool take, const Point& a, const Point& b) {
  return Point{fselect(take, a.X, b.X), fselect(take, a.Y, b.Y), fselect(take, a.Z, b.Z)};
}
SCL_HD Point pt_load(const u64* p) { return Point{FQ::ld(p), FQ::ld(p + 4), FQ::ld(p + 8)}; }
SCL_HD void pt_store(u64* p, const Point& v) {
  FQ::st(p, v.X);
  FQ::st(p + 4, v.Y);
  FQ::st(p + 8, v.Z);
}

// the common tail of add and mixed add
SCL_HD Point pt_add_finish(const Fe& xx, const Fe& yy, const Fe& zz, const Fe& xy, const Fe& yz, const Fe& xz) {
  const Fe m = fadd(fadd(xx, xx), xx);
  const Fe bz = fmul_b3(zz);
  const Fe s = fadd(yy, bz);
  const Fe d = fsub(yy, bz);
  const Fe u = fmul_b3(xz);
  Point r;
  r.X = fsub(fmul(xy, d), fmul(yz, u));
  r.Y = fadd(fmul(d, s), fmul(u, m));
  r.Z = fadd(fmul(s, yz), fmul(m, xy));
  return r;
}

// P + Q, any P and Q (algorithm 7): the three cross sums by (a + b)(c + d) - ac - bd
SCL_HD Point pt_add(const Point& p, const Point& q) {
  const Fe xx = fmul(p.X, q.X), yy = fmul(p.Y, q.Y), zz = fmul(p.Z, q.Z);
  const Fe xy = fsub(fmul(fadd(p.X, p.Y), fadd(q.X, q.Y)), fadd(xx, yy));
  const Fe yz = fsub(fmul(fadd(p.Y, p.Z), fadd(q.Y, q.Z)), fadd(yy, zz));
  const Fe xz = fsub(fmul(fadd(p.X, p.Z), fadd(q.X, q.Z)), fadd(xx, zz));
  return pt_add_finish(xx, yy, zz, xy, yz, xz);
}

// P + (x, y, 1), any P, a finite affine Q (algorithm 8): zz = Z1, yz = Y1 + y Z1, xz = X1 + x Z1
SCL_HD Point pt_add_affine(const Point& p, const Affine& q) {
  const Fe xx = fmul(p.X, q.x), yy = fmul(p.Y, q.y);
  const Fe xy = fsub(fmul(fadd(p.X, p.Y), fadd(q.x, q.y)), fadd(xx, yy));
  const Fe yz = fadd(fmul(q.y, p.Z), p.Y);
  const Fe xz = fadd(fmul(q.x, p.Z), p.X);
  return pt_add_finish(xx, yy, p.Z, xy, yz, xz);
}

// 2 P (algorithm 9): with yy = Y^2, bz = b3 Z^2, e = yy - 3 bz:  X3 = 2 XY e,  Y3 = e (yy + bz) + 8 yy bz,  Z3 = 8 yy YZ
SCL_HD Point pt_dbl(const Point& p) {
  const Fe yy = fsqr(p.Y);
  const Fe bz = fmul_b3(fsqr(p.Z));
  Fe y8 = fadd(yy, yy);
  y8 = fadd(y8, y8);
  y8 = fadd(y8, y8);
  const Fe e = fsub(yy, fadd(fadd(bz, bz), bz));
  const Fe xe = fmul(fmul(p.X, p.Y), e);
  Point r;
  r.X = fadd(xe, xe);
  r.Y = fadd(fmul(e, fadd(yy, bz)), fmul(y8, bz));
  r.Z = fmul(y8, fmul(p.Y, p.Z));
  return r;
}

// ec::negate (secp256k1_curve.cc:276-283): Y = 0 becomes infinity, as there
SCL_HD Point pt_neg(const Point& p) {
  return pt_select(FQ::is_zero(p.Y), pt_infinity(), Point{p.X, FQ::neg(FQ::Ctx{}, p.Y), p.Z});
}
SCL_HD Point pt_sub(const Point& p, const Point& q) { return pt_add(p, pt_neg(q)); }

// ec::equal (secp256k1_curve.cc:77-84): X1 Z2 == X2 Z1 and Y1 Z2 == Y2 Z1
SCL_HD bool pt_equal(const Point& p, const Point& q) {
  const bool ex = FQ::eq(fmul(p.X, q.Z), fmul(q.X, p.Z));
  const bool ey = FQ::eq(fmul(p.Y, q.Z), fmul(q.Y, p.Z));
  return ex & ey;
}

SCL_HD Fe fsqn(Fe a, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < n; ++i) a = fsqr(a);
  return a;
}
// a^(p - 2); inv(0) = 0.  p - 2 in binary is 223 ones, a zero, 22 ones, then 0000101101: runs of ones are built by doubling
// their length (x_k = a^(2^k - 1)), 255 squares and 15 products, no table and so no indexed array in registers.
SCL_HD Fe finv(const Fe& a) {
  const Fe x2 = fmul(fsqn(a, 1), a);
  const Fe x3 = fmul(fsqn(x2, 1), a);
  const Fe x6 = fmul(fsqn(x3, 3), x3);
  const Fe x9 = fmul(fsqn(x6, 3), x3);
  const Fe x11 = fmul(fsqn(x9, 2), x2);
  const Fe x22 = fmul(fsqn(x11, 11), x11);
  const Fe x44 = fmul(fsqn(x22, 22), x22);
  const Fe x88 = fmul(fsqn(x44, 44), x44);
  const Fe x176 = fmul(fsqn(x88, 88), x88);
  const Fe x220 = fmul(fsqn(x176, 44), x44);
  const Fe x223 = fmul(fsqn(x220, 3), x3);
  Fe t = fmul(fsqn(x223, 23), x22);
  t = fmul(fsqn(t, 5), a);
  t = fmul(fsqn(t, 3), x2);
  t = fmul(fsqn(t, 2), a);
  return t;
}

// ec::toAffine (secp256k1_curve.cc:68-75); of infinity: (0, 0)
SCL_HD Affine pt_to_affine(const Point& p) {
  const Fe zi = finv(p.Z);
  return Affine{fmul(p.X, zi), fmul(p.Y, zi)};
}

SCL_HD void fe_write_be(unsigned char* dst, const Fe& a) {  // Field::write: out of Montgomery form, big-endian
  const Fe v = FQ::from_mont(FQ::Ctx{}, a);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 w = v.w[3 - i];
#pragma unroll
    for (int b = 0; b < 8; ++b) dst[8 * i + b] = (unsigned char)(w >> (56 - 8 * b));
  }
}
SCL_HD Fe fe_read_be(const unsigned char* src) {  // Field::read
  Fe v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u64 w = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) w = (w << 8) | src[8 * i + b];
    v.w[3 - i] = w;
  }
  return FQ::to_mont(FQ::Ctx{}, v);
}

// ec::toBytes(dest, in, false) (secp256k1_curve.cc:395-431): 0x04 | x | y, infinity 0x06 and 64 zero bytes
SCL_HD void pt_write(unsigned char* dst, const Point& p) {
  const bool inf = pt_is_infinity(p);
  const Affine a = pt_to_affine(p);  // (0, 0) for infinity: the zero bytes
  dst[0] = (unsigned char)(inf ? (FLAG_FULL_POINT | FLAG_INFINITY) : FLAG_FULL_POINT);
  fe_write_be(dst + 1, a.x);
  fe_write_be(dst + 33, a.y);
}
// ec::fromBytes (secp256k1_curve.cc:357-389) for the uncompressed form: the infinity flag wins, a full point is taken as it is.
// Returns 0, or 1 for an image that is neither (a compressed point: not built here); the point is then infinity.
SCL_HD int pt_read(Point& out, const unsigned char* src) {
  const unsigned flags = src[0];
  out = pt_infinity();
  if (flags & FLAG_INFINITY) return 0;  // nothing behind the flag byte is read, as in the reference
  if (!(flags & FLAG_FULL_POINT)) return 1;
  out = Point{fe_read_be(src + 1), fe_read_be(src + 33), fone()};
  return 0;
}

// digit w (4 bits) of a scalar taken out of Montgomery form
SCL_HD unsigned scalar_digit(const Fe& plain, int w) { return (unsigned)(plain.w[w >> 4] >> (4 * (w & 15))) & 15u; }
SCL_HD Fe scalar_plain(const Fe& mont) { return FR::from_mont(FR::Ctx{}, mont); }

// s * P by double-and-add from the top bit (the host mirror's operator*, and the device table's small multiples)
SCL_HD Point pt_mul(const Point& p, const Fe& scalar_mont) {
  const Fe k = scalar_plain(scalar_mont);
  Point r = pt_infinity();
  for (int i = 255; i >= 0; --i) {
    r = pt_dbl(r);
    if ((k.w[i >> 6] >> (i & 63)) & 1) r = pt_add(r, p);
  }
  return r;
}

// ---- ECDSA (util::ECDSA, include/scl/util/sign.h:87-178): what signing and verification need beyond the group law -----------
SCL_HD Fe rmul(const Fe& a, const Fe& b) { return FR::mul(FR::Ctx{}, a, b); }
SCL_HD Fe rsqn(Fe a, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < n; ++i) a = rmul(a, a);
  return a;
}
// a^(q - 2) in the scalar field; rinv(0) = 0.  q - 2 is 127 ones, a zero, and 128 bits without structure (69 of them set): the
// run is built by doubling its length as in finv (x_k = a^(2^k - 1); 126 squares, 12 products), the rest is a rolled
// square-and-multiply over the constant -- the bit is the same in every lane, so the branch is uniform.  255 squares and
// 81 products; no table, so no indexed array in registers.
SCL_HD Fe rinv(const Fe& a) {
  Fe x = a;  // x_1
  int k = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int step = 0; step < 6; ++step) {  // x_k -> x_2k -> x_(2k + 1): 1, 3, 7, 15, 31, 63, 127
    x = rmul(rsqn(x, k), x);
    x = rmul(rsqn(x, 1), a);
    k = 2 * k + 1;
  }
  x = rsqn(x, 1);  // the zero that ends the run
  const u64 lo = FR::P(0) - 2, hi = FR::P(1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 127; i >= 0; --i) {
    x = rsqn(x, 1);
    if (((i >= 64 ? hi : lo) >> (i & 63)) & 1) x = rmul(x, a);
  }
  return x;
}

// the integer 32 big-endian bytes spell (not reduced, not in Montgomery form)
SCL_HD Fe u256_read_be(const unsigned char* src) {
  Fe v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u64 w = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) w = (w << 8) | src[8 * i + b];
    v.w[3 - i] = w;
  }
  return v;
}
// FF<Secp256k1Scalar>::read (montyFromBytes -> montyIn, ff_ops_gmp.h:280-290): 32 big-endian bytes, any value below 2^256,
// reduced mod q by the Montgomery product with R^2 (valid for a first operand below 2^256)
SCL_HD Fe scalar_from_be32(const unsigned char* src) { return FR::to_mont(FR::Ctx{}, u256_read_be(src)); }

// ECDSA::conversionFunc (sign.h:157-162): the affine x written big-endian and read back mod q.  x < p < 2^256 goes into the
// scalar field's Montgomery form as any 256-bit integer does.  Of infinity: finv(0) = 0, so x = 0 and the result is 0.
SCL_HD Fe ecdsa_conversion(const Point& p) {
  const Fe x = FQ::from_mont(FQ::Ctx{}, fmul(p.X, finv(p.Z)));
  return FR::to_mont(FR::Ctx{}, x);
}

// "R is not infinity and x(R) mod q == r" for a plain integer r < q, without the inversion: x(R) < p < 2 q, so x mod q == r
// iff x == r or x == r + q, the second only when r + q < p; and x == v iff X == v Z.  q in the coordinate field's
// Montgomery form is a constant, so v = r + q costs an addition: three products (r into Montgomery form, r Z, (r + q) Z).
SCL_HD bool pt_x_is(const Point& p, const Fe& r_plain) {
  const Fe q_mont = FQ::make(0xE21120489F1D95E1ull, 0x24A1AC9EB3FDE294ull, 0xFFFFFFFEBAAED80Dull, 0xFFFFFFFFFFFFFFFFull);  // q 2^256 mod p
  const Fe r = FQ::to_mont(FQ::Ctx{}, r_plain);
  Fe sum;
  const u64 carry = FQ::add_n(sum, r_plain, FR::prime());
  const bool second = !carry && !FQ::geq_p(sum);  // r + q < p
  const bool e0 = FQ::eq(p.X, fmul(r, p.Z));
  const bool e1 = FQ::eq(p.X, fmul(fadd(r, q_mont), p.Z));
  return (!pt_is_infinity(p)) & (e0 | (second & e1));
}

// acc + k * B from B's window table (k_ec_base_table's layout: entry (w, d - 1) is the affine d 16^w B): 64 mixed additions.
// A zero digit has no affine operand; the lane adds entry 1 of the window like the others and keeps its old sum.
SCL_HD Point pt_add_mul_table(Point acc, const u64* table, const Fe& k_plain) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int w = 0; w < WINDOWS; ++w) {
    const unsigned d = scalar_digit(k_plain, w);
    const u64* ent = table + ((size_t)w * WINDOW_ENTRIES + (d ? d - 1 : 0)) * AFFINE_LIMBS;
    const Affine q{FQ::ld(ent), FQ::ld(ent + 4)};
    acc = pt_select(d != 0, pt_add_affine(acc, q), acc);
  }
  return acc;
}

// k * P for a point and a scalar of the lane's own, in 4-bit windows.  The lane writes its table of d P, d = 0..15 (entry 0 is
// infinity: the formulas are complete, so a zero digit needs neither a branch nor a select), to memory it was given -- entry d
// at table + d * pitch limbs -- by 7 doublings and 7 additions, then runs 64 windows of 4 doublings and one table addition
// from the top digit down.  The digit only picks an address.
SCL_HD Point pt_mul_window(const Point& p, const Fe& k_plain, u64* table, size_t pitch) {
  pt_store(table, pt_infinity());
  pt_store(table + pitch, p);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int j = 1; j < 8; ++j) {
    const Point even = pt_dbl(pt_load(table + (size_t)j * pitch));
    pt_store(table + (size_t)(2 * j) * pitch, even);
    pt_store(table + (size_t)(2 * j + 1) * pitch, pt_add(even, p));
  }
  Point acc = pt_infinity();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int w = WINDOWS - 1; w >= 0; --w) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < 4; ++i) acc = pt_dbl(acc);
    acc = pt_add(acc, pt_load(table + (size_t)scalar_digit(k_plain, w) * pitch));
  }
  return acc;
}

}  // namespace secp
}  // namespace sclhip
