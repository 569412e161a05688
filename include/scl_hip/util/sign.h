// include/scl_hip/util/sign.h -- scl::util::ECDSA and util::Signature<ECDSA> (include/scl/util/sign.h:33-178) on the host, one
// signature per call, on the point and scalar functions the kernels run (detail/secp256k1.hpp: rinv, ecdsa_conversion,
// pt_mul_window, pt_x_is).  Batches are signed and verified on the device by hip::Ecdsa (hip/ecdsa.h).
//
// What differs from the reference is cost, not results: verify compares x(R) with r by cross-multiplication instead of
// normalising R, and inverts s by the addition chain of rinv.  s == 0 throws what FF::inverse throws.
#ifndef SCL_HIP_UTIL_SIGN_H
#define SCL_HIP_UTIL_SIGN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../detail/secp256k1.hpp"
#include "../math/curves/secp256k1.h"
#include "../math/ec.h"
#include "../math/ff.h"
#include "prg.h"

namespace scl::util {

template <typename SIGNATURE_SCHEME>
struct Signature;

class ECDSA;

/// (r, s); the image is r then s, 32 big-endian bytes each (sign.h:41-82)
template <>
struct Signature<ECDSA> {
 private:
  using ElementType = math::FF<math::ec::Secp256k1::Scalar>;

 public:
  constexpr static std::size_t byteSize() { return ElementType::byteSize() * 2; }
  static Signature<ECDSA> read(const unsigned char* buf) {
    return {ElementType::read(buf), ElementType::read(buf + ElementType::byteSize())};
  }
  void write(unsigned char* buf) const {
    r.write(buf);
    s.write(buf + ElementType::byteSize());
  }
  ElementType r;
  ElementType s;
};

class ECDSA {
 public:
  using PublicKey = math::EC<math::ec::Secp256k1>;
  using SecretKey = PublicKey::ScalarField;

  /// sign.h:104-106
  static PublicKey derive(const SecretKey& secret_key) { return secret_key * PublicKey::generator(); }

  /// sign.h:116-126: the nonce is the first thing drawn from prg
  template <typename DIGEST>
  static Signature<ECDSA> Sign(const SecretKey& secret_key, const DIGEST& digest, PRG& prg) {
    const SecretKey k = SecretKey::random(prg);
    const SecretKey rx = conversionFunc(k * PublicKey::generator());
    const SecretKey h = digestToElement(digest);
    return {rx, k.inverse() * (h + secret_key * rx)};
  }

  /// sign.h:135-146.  s == 0: FF::inverse throws std::logic_error
  template <typename DIGEST>
  static bool verify(const PublicKey& public_key, const Signature<ECDSA>& signature, const DIGEST& digest) {
    namespace secp = sclhip::secp;
    const SecretKey h = digestToElement(digest);
    if (signature.s == SecretKey::zero()) (void)signature.s.inverse();
    const secp::Fe si = secp::rinv(limbs(signature.s));
    const secp::Fe u1 = secp::rmul(limbs(h), si);
    const secp::Fe u2 = secp::rmul(limbs(signature.r), si);
    std::uint64_t pk[secp::POINT_LIMBS], table[secp::MUL_TABLE_ENTRIES * secp::POINT_LIMBS];
    public_key.toLimbs(pk);
    secp::Point R = secp::pt_mul_window(secp::pt_load(pk), secp::scalar_plain(u2), table, secp::POINT_LIMBS);
    // u1 G: the host has no window table of the generator, so the bit ladder of EC::operator*
    R = secp::pt_add(R, secp::pt_mul(secp::pt_generator(), u1));
    return secp::pt_x_is(R, secp::scalar_plain(limbs(signature.r)));
  }

  /// sign.h:157-162: the affine x of R as an integer, mod the group order (0 for infinity)
  static SecretKey conversionFunc(const PublicKey& R) {
    std::uint64_t p[sclhip::secp::POINT_LIMBS];
    R.toLimbs(p);
    return SecretKey::fromLimbs(sclhip::secp::ecdsa_conversion(sclhip::secp::pt_load(p)).w);
  }

  /// sign.h:169-177: a digest shorter than 32 bytes fills the FRONT of a zeroed buffer, a longer one gives its first 32 bytes
  template <typename DIGEST>
  static SecretKey digestToElement(const DIGEST& digest) {
    unsigned char buf[SecretKey::byteSize()] = {0};
    std::copy(digest.begin(), digest.begin() + std::min<std::size_t>(digest.size(), SecretKey::byteSize()), buf);
    return SecretKey::fromLimbs(sclhip::secp::scalar_from_be32(buf).w);
  }

 private:
  static sclhip::U256 limbs(const SecretKey& v) {
    sclhip::U256 r;
    v.toLimbs(r.w);
    return r;
  }
};

}  // namespace scl::util

#endif  // SCL_HIP_UTIL_SIGN_H
