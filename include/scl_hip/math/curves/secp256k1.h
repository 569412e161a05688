// include/scl_hip/math/curves/secp256k1.h -- the curve tag of math::EC (include/scl/math/curves/secp256k1.h:30-60).
#ifndef SCL_HIP_MATH_CURVES_SECP256K1_H
#define SCL_HIP_MATH_CURVES_SECP256K1_H

#include "../ff.h"

namespace scl::math::ec {

struct Secp256k1 {
  using Field = ff::Secp256k1Field;    ///< the field the curve is defined over
  using Scalar = ff::Secp256k1Scalar;  ///< the field of its large prime-order group
  constexpr static const char* NAME = "secp256k1";
};

}  // namespace scl::math::ec

#endif
