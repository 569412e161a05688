// include/scl_hip/math/ec.h -- math::EC<ec::Secp256k1> on the host (include/scl/math/ec.h:42-339 over
// src/scl/math/curves/secp256k1_curve.cc), on the point functions the kernels run (detail/secp256k1.hpp).
//
// Built: generator, zero, fromAffine (throws on a point off the curve), + - negate doublePoint, * ScalarField, == !=,
// isPointAtInfinity, toAffine, normalize, write(dest, false), read (uncompressed and infinity-flagged images), Serializer<EC>.
// Not built, and a compile error rather than something else: scalars that are math::Number (there is no such operator*) and the
// compressed image (write's second parameter only converts from the constant `false`).
#ifndef SCL_HIP_MATH_EC_H
#define SCL_HIP_MATH_EC_H

#include <array>
#include <cstddef>
#include <ostream>
#include <stdexcept>
#include <string>

#include "../detail/secp256k1.hpp"
#include "../serialization/serializer.h"
#include "curves/secp256k1.h"
#include "ff.h"

namespace scl::math {

template <typename CURVE>
class EC;  // one curve is built

template <>
class EC<ec::Secp256k1> final {
  using P = sclhip::secp::Point;

 public:
  using Field = FF<ec::Secp256k1::Field>;
  using ScalarField = FF<ec::Secp256k1::Scalar>;

  /// the `compress` argument of write: converts from the constant false only
  struct Uncompressed {
    consteval Uncompressed(bool compress) {
      if (compress) throw "the compressed point image is not built";
    }
  };

  constexpr static std::size_t byteSize() { return sclhip::secp::WIRE_BYTES; }  ///< ec.h:58-60 for compressed = false
  constexpr static const char* name() { return ec::Secp256k1::NAME; }

  static EC generator() { return EC(sclhip::secp::pt_generator()); }
  static EC zero() { return EC(); }
  /// ec.h:97-101 / setAffine (secp256k1_curve.cc:59-66)
  static EC fromAffine(const Field& x, const Field& y) {
    if (y * y != x * x * x + Field(7)) throw std::invalid_argument("provided (x, y) not on curve");
    return EC(P{limbs(x), limbs(y), sclhip::secp::fone()});
  }
  /// ec.h:88-92: an uncompressed or an infinity-flagged image
  static EC read(const unsigned char* src) {
    EC e;
    if (sclhip::secp::pt_read(e.m_p, src)) throw std::invalid_argument("compressed point images are not supported");
    return e;
  }
  /// the C ABI's point: 12 limbs
  static EC fromLimbs(const std::uint64_t* src) { return EC(sclhip::secp::pt_load(src)); }
  void toLimbs(std::uint64_t* dest) const { sclhip::secp::pt_store(dest, m_p); }

  EC() : m_p(sclhip::secp::pt_infinity()) {}

  EC& operator+=(const EC& o) { m_p = sclhip::secp::pt_add(m_p, o.m_p); return *this; }
  friend EC operator+(EC a, const EC& b) { return a += b; }
  EC& doublePointInPlace() { m_p = sclhip::secp::pt_dbl(m_p); return *this; }
  EC doublePoint() const { EC c(*this); return c.doublePointInPlace(); }
  EC& operator-=(const EC& o) { m_p = sclhip::secp::pt_sub(m_p, o.m_p); return *this; }
  friend EC operator-(EC a, const EC& b) { return a -= b; }
  EC& operator*=(const ScalarField& s) { m_p = sclhip::secp::pt_mul(m_p, limbs(s)); return *this; }
  friend EC operator*(EC p, const ScalarField& s) { return p *= s; }
  friend EC operator*(const ScalarField& s, EC p) { return p *= s; }
  EC& negate() { m_p = sclhip::secp::pt_neg(m_p); return *this; }
  friend EC operator-(EC p) { return p.negate(); }

  bool equal(const EC& o) const { return sclhip::secp::pt_equal(m_p, o.m_p); }
  friend bool operator==(const EC& a, const EC& b) { return a.equal(b); }
  friend bool operator!=(const EC& a, const EC& b) { return !a.equal(b); }
  bool isPointAtInfinity() const { return sclhip::secp::pt_is_infinity(m_p); }

  /// ec.h:265-267 / toAffine (secp256k1_curve.cc:68-75); of infinity: (0, 0)
  std::array<Field, 2> toAffine() const {
    const auto a = sclhip::secp::pt_to_affine(m_p);
    return {Field::fromLimbs(a.x.w), Field::fromLimbs(a.y.w)};
  }
  /// ec.h:272-281: Z = 1 unless the point is infinity
  void normalize() {
    if (isPointAtInfinity()) return;
    const auto a = sclhip::secp::pt_to_affine(m_p);
    m_p = P{a.x, a.y, sclhip::secp::fone()};
  }

  std::string toString() const {
    if (isPointAtInfinity()) return "EC{POINT_AT_INFINITY}";
    const auto a = toAffine();
    return "EC{" + a[0].toString() + ", " + a[1].toString() + "}";
  }
  friend std::ostream& operator<<(std::ostream& os, const EC& e) { return os << e.toString(); }

  /// ec.h:298-300 with compress = false: 65 bytes
  void write(unsigned char* dest, Uncompressed) const { sclhip::secp::pt_write(dest, m_p); }

 private:
  explicit EC(const P& p) : m_p(p) {}
  template <typename F>
  static sclhip::U256 limbs(const FF<F>& v) {
    sclhip::U256 r;
    v.toLimbs(r.w);
    return r;
  }
  P m_p;
};

}  // namespace scl::math

namespace scl::seri {

/// Serializer<EC> (ec.h:315-339): always the uncompressed image
template <>
struct Serializer<math::EC<math::ec::Secp256k1>, void> {
  using Point = math::EC<math::ec::Secp256k1>;
  static constexpr std::size_t sizeOf(const Point&) { return Point::byteSize(); }
  static std::size_t write(const Point& p, unsigned char* buf) {
    p.write(buf, false);
    return Point::byteSize();
  }
  static std::size_t read(Point& p, const unsigned char* buf) {
    p = Point::read(buf);
    return Point::byteSize();
  }
};

}  // namespace scl::seri

#endif
