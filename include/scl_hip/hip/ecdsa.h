// include/scl_hip/hip/ecdsa.h -- ECDSA over device-resident batches: the batch form of util::ECDSA (include/scl/util/sign.h:87-178)
// over hip::DeviceVector (secret keys, nonces, signatures), hip::DevicePoints (public keys) and a device buffer of 32-byte
// digests (a row of scl_hip_sha256's output each).  Signatures are a DeviceVector of 2 n scalars, r then s per signature -- the
// C ABI's [n][8] limbs, and element for element what Signature<ECDSA>::write emits.  hip::Ecdsa owns the generator's window
// table (built once, at construction) and allocates the scratch of the per-lane multiplication itself.  Thin calls into the C
// ABI (scl_hip_ec_mul, scl_hip_ecdsa_*); the per-signature forms are util::ECDSA (util/sign.h).
#ifndef SCL_HIP_HIP_ECDSA_H
#define SCL_HIP_HIP_ECDSA_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../util/digest.h"
#include "../util/sign.h"
#include "device.h"
#include "feldman.h"

namespace scl::hip {

class Ecdsa {
 public:
  using F = util::ECDSA::SecretKey;
  using PublicKey = util::ECDSA::PublicKey;
  using Digest = util::Digest<256>;

  explicit Ecdsa(void* stream = nullptr) : m_table(scl_hip_ec_base_table_bytes()) {
    std::uint64_t g[DevicePoints::LIMBS];
    check(scl_hip_ec_generator(g));
    check(scl_hip_ec_base_table(m_table.get(), g, stream));
  }
  const void* table() const { return m_table.get(); }

  /// n digests, 32 bytes each, uploaded
  static DeviceBuffer digests(const std::vector<Digest>& host) {
    DeviceBuffer d(host.size() * 32);
    if (!host.empty()) check(scl_hip_memcpy_h2d(d.get(), host.data(), host.size() * 32, nullptr));
    check(scl_hip_stream_sync(nullptr));
    return d;
  }
  /// the window table of a public key, for verifyOneSigner
  static DeviceBuffer tableOf(const PublicKey& pk, void* stream = nullptr) {
    DeviceBuffer t(scl_hip_ec_base_table_bytes());
    std::uint64_t limbs[DevicePoints::LIMBS];
    pk.toLimbs(limbs);
    check(scl_hip_ec_base_table(t.get(), limbs, stream));
    return t;
  }

  /// ECDSA::derive per key: sk[i] * G
  DevicePoints derive(const DeviceVector<F>& sk, void* stream = nullptr) const {
    DevicePoints out(1, sk.size());
    check(scl_hip_ec_mul_base(out.data(), table(), sk.data(), sk.size(), stream));
    return out;
  }

  /// scalars[i] * points[i]
  DevicePoints mul(const DeviceVector<F>& scalars, const DevicePoints& points, void* stream = nullptr) const {
    const std::size_t n = scalars.size();
    if (points.rows() * points.cols() != n) check(SCL_ERR_SIZE_MISMATCH);
    DevicePoints out(1, n);
    DeviceBuffer scratch(scl_hip_ec_mul_scratch_bytes(n));
    check(scl_hip_ec_mul(out.data(), points.data(), scalars.data(), scratch.get(), n, stream));
    check(scl_hip_stream_sync(stream));  // `scratch` ends with this call
    return out;
  }

  /// ECDSA::conversionFunc per point
  DeviceVector<F> conversion(const DevicePoints& points, void* stream = nullptr) const {
    const std::size_t n = points.rows() * points.cols();
    DeviceVector<F> out(n);
    check(scl_hip_ecdsa_conversion(out.data(), points.data(), n, stream));
    return out;
  }

  /// ECDSA::Sign per digest with nonces[i] in the place of SecretKey::random(prg); sk holds one key for all or one per
  /// signature.  Returns 2 n scalars (r, s, r, s, ..).  *zero_nonce (if given) tells whether any nonce was zero, where the
  /// reference throws and this writes (0, 0).
  DeviceVector<F> sign(const DeviceVector<F>& sk, const DeviceVector<F>& nonces, const DeviceBuffer& digests32,
                       bool* zero_nonce = nullptr, void* stream = nullptr) const {
    const std::size_t n = nonces.size();
    if ((sk.size() != 1 && sk.size() != n) || digests32.bytes() != n * 32) check(SCL_ERR_SIZE_MISMATCH);
    DeviceVector<F> sig(2 * n);
    DeviceBuffer status(4);
    check(scl_hip_memset(status.get(), 0, 4, stream));
    check(scl_hip_ecdsa_sign(sig.data(), table(), sk.data(), sk.size() == 1 ? 0 : 1, nonces.data(),
                             static_cast<const unsigned char*>(digests32.get()), static_cast<unsigned*>(status.get()), n, stream));
    unsigned flag = 0;
    check(scl_hip_memcpy_d2h(&flag, status.get(), 4, stream));
    check(scl_hip_stream_sync(stream));
    if (zero_nonce) *zero_nonce = flag != 0;
    return sig;
  }

  /// ECDSA::verify per signature: 1 accepted, 0 rejected, 2 where s == 0 (the per-signature form throws there).  pk holds one
  /// key for all or one per signature.
  std::vector<unsigned char> verify(const DevicePoints& pk, const DeviceVector<F>& sig, const DeviceBuffer& digests32,
                                    void* stream = nullptr) const {
    const std::size_t n = sig.size() / 2, keys = pk.rows() * pk.cols();
    if (sig.size() % 2 || (keys != 1 && keys != n) || digests32.bytes() != n * 32) check(SCL_ERR_SIZE_MISMATCH);
    DeviceBuffer ok(n), scratch(scl_hip_ec_mul_scratch_bytes(n));
    check(scl_hip_ecdsa_verify(static_cast<unsigned char*>(ok.get()), sig.data(), static_cast<const unsigned char*>(digests32.get()),
                               pk.data(), keys == 1 ? 0 : 1, table(), scratch.get(), n, stream));
    return toHost(ok, n, stream);
  }

  /// the same verdicts for one signer's signatures, from the window table of the signer's key (tableOf)
  std::vector<unsigned char> verifyOneSigner(const DeviceBuffer& qtable, const DeviceVector<F>& sig, const DeviceBuffer& digests32,
                                             void* stream = nullptr) const {
    const std::size_t n = sig.size() / 2;
    if (sig.size() % 2 || digests32.bytes() != n * 32 || qtable.bytes() != scl_hip_ec_base_table_bytes()) check(SCL_ERR_SIZE_MISMATCH);
    DeviceBuffer ok(n);
    check(scl_hip_ecdsa_verify_base(static_cast<unsigned char*>(ok.get()), sig.data(),
                                    static_cast<const unsigned char*>(digests32.get()), qtable.get(), table(), n, stream));
    return toHost(ok, n, stream);
  }
  std::vector<unsigned char> verifyOneSigner(const PublicKey& pk, const DeviceVector<F>& sig, const DeviceBuffer& digests32,
                                             void* stream = nullptr) const {
    const DeviceBuffer qtable = tableOf(pk, stream);
    return verifyOneSigner(qtable, sig, digests32, stream);
  }

 private:
  static std::vector<unsigned char> toHost(const DeviceBuffer& ok, std::size_t n, void* stream) {
    std::vector<unsigned char> v(n);
    if (n) check(scl_hip_memcpy_d2h(v.data(), ok.get(), n, stream));
    check(scl_hip_stream_sync(stream));  // the call's scratch ends with it
    return v;
  }
  DeviceBuffer m_table;
};

}  // namespace scl::hip

#endif  // SCL_HIP_HIP_ECDSA_H
