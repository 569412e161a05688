// include/scl_hip/scl.h -- umbrella header: the hot-path surface of <scl/scl.h> on the MI355X engine.
#ifndef SCL_HIP_SCL_H
#define SCL_HIP_SCL_H

#include "hip/device.h"
#include "hip/elementwise.h"
#include "hip/feldman.h"
#include "hip/merkle.h"
#include "hip/open.h"
#include "math/fields/ff_ops.h"
#include "math/ff.h"
#include "math/array.h"
#include "math/curves/secp256k1.h"
#include "math/ec.h"
#include "math/lagrange.h"
#include "math/matrix.h"
#include "math/poly.h"
#include "math/vector.h"
#include "math/z2k.h"
#include "serialization/serializer.h"
#include "ss/additive.h"
#include "ss/feldman.h"
#include "ss/shamir.h"
#include "util/bitmap.h"
#include "util/digest.h"
#include "util/iuf_hash.h"
#include "util/merkle.h"
#include "util/merkle_proof.h"
#include "util/prg.h"
#include "util/sha256.h"
#include "names.h"

#endif
