// include/scl_hip/hip/feldman.h -- Feldman VSS over device-resident secrets: the batch form of ss::feldmanSecretShare /
// feldmanVerify (include/scl/ss/feldman.h:107-163) over hip::DeviceVector (the secrets, or one party's shares) and
// hip::ShareMatrix (the shares as ss::shamirSecretShare deals them, [party][secret], no transpose).  Commitments stay in HBM
// as points ([k][secret], k = 0..t); one secret's column comes back as the math::Vector<EC> the per-secret forms use, so the
// two sides are interchangeable.  hip::Feldman owns the generator's window table (built once, at construction), computes the
// Lagrange basis of an index with the library and uploads it.  Thin calls into the C ABI (scl_hip_ec_*, scl_hip_feldman_*).
#ifndef SCL_HIP_HIP_FELDMAN_H
#define SCL_HIP_HIP_FELDMAN_H

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../math/ec.h"
#include "../math/lagrange.h"
#include "../math/vector.h"
#include "../ss/shamir.h"
#include "../util/prg.h"
#include "device.h"

namespace scl::hip {

using FeldmanGroup = math::EC<math::ec::Secp256k1>;
using FeldmanField = FeldmanGroup::ScalarField;

/// rows x cols points in HBM, row-major, 12 limbs each (the C ABI's point)
class DevicePoints {
 public:
  static constexpr std::size_t LIMBS = SCL_EC_POINT_LIMBS;

  DevicePoints() = default;
  DevicePoints(std::size_t rows, std::size_t cols) : m_buf(rows * cols * LIMBS * 8), m_rows(rows), m_cols(cols) {}
  /// upload one row
  explicit DevicePoints(const std::vector<FeldmanGroup>& host) : DevicePoints(1, host.size()) {
    std::vector<std::uint64_t> limbs(host.size() * LIMBS);
    for (std::size_t i = 0; i < host.size(); ++i) host[i].toLimbs(limbs.data() + i * LIMBS);
    if (!host.empty()) check(scl_hip_memcpy_h2d(m_buf.get(), limbs.data(), limbs.size() * 8, nullptr));
    check(scl_hip_stream_sync(nullptr));
  }

  std::size_t rows() const { return m_rows; }
  std::size_t cols() const { return m_cols; }
  std::size_t stride() const { return m_cols; }
  std::uint64_t* data() { return static_cast<std::uint64_t*>(m_buf.get()); }
  const std::uint64_t* data() const { return static_cast<const std::uint64_t*>(m_buf.get()); }
  const std::uint64_t* row(std::size_t k) const { return data() + k * m_cols * LIMBS; }

  /// column s: the commitments of secret s as feldmanSecretShare returns them
  math::Vector<FeldmanGroup> column(std::size_t s, void* stream = nullptr) const {
    if (s >= m_cols) check(SCL_ERR_INVALID_RANGE);
    std::vector<std::uint64_t> limbs(m_rows * LIMBS);
    for (std::size_t k = 0; k < m_rows; ++k)
      check(scl_hip_memcpy_d2h(limbs.data() + k * LIMBS, row(k) + s * LIMBS, LIMBS * 8, stream));
    check(scl_hip_stream_sync(stream));
    std::vector<FeldmanGroup> out;
    out.reserve(m_rows);
    for (std::size_t k = 0; k < m_rows; ++k) out.emplace_back(FeldmanGroup::fromLimbs(limbs.data() + k * LIMBS));
    return math::Vector<FeldmanGroup>(std::move(out));
  }
  /// every point, row-major
  std::vector<FeldmanGroup> toHost(void* stream = nullptr) const {
    std::vector<std::uint64_t> limbs(m_rows * m_cols * LIMBS);
    if (!limbs.empty()) check(scl_hip_memcpy_d2h(limbs.data(), m_buf.get(), limbs.size() * 8, stream));
    check(scl_hip_stream_sync(stream));
    std::vector<FeldmanGroup> out;
    out.reserve(m_rows * m_cols);
    for (std::size_t i = 0; i < m_rows * m_cols; ++i) out.emplace_back(FeldmanGroup::fromLimbs(limbs.data() + i * LIMBS));
    return out;
  }

 private:
  DeviceBuffer m_buf;
  std::size_t m_rows = 0, m_cols = 0;
};

/// what feldmanSecretShare returns for a batch: the share matrix and the commitments [t + 1][secret]
struct DeviceFeldmanSharing {
  ShareMatrix<FeldmanField> shares;
  DevicePoints commitments;
  /// secret s as the per-secret form has it (ss::FeldmanSharing)
  math::Vector<FeldmanField> sharesOf(std::size_t s) const { return math::Vector<FeldmanField>(shares.sharesOf(s)); }
  math::Vector<FeldmanGroup> commitmentsOf(std::size_t s) const { return commitments.column(s); }
};

/// The generator's window table and the calls that read it.  Construction launches the one kernel that fills the table.
class Feldman {
 public:
  using F = FeldmanField;

  explicit Feldman(void* stream = nullptr) : m_table(scl_hip_ec_base_table_bytes()) {
    std::uint64_t g[DevicePoints::LIMBS];
    check(scl_hip_ec_generator(g));
    check(scl_hip_ec_base_table(m_table.get(), g, stream));
  }
  const void* table() const { return m_table.get(); }

  /// s[i] * G
  DevicePoints mulGenerator(const DeviceVector<F>& s, void* stream = nullptr) const {
    DevicePoints out(1, s.size());
    check(scl_hip_ec_mul_base(out.data(), table(), s.data(), s.size(), stream));
    return out;
  }

  /// the commitments of feldmanSecretShare for every secret: row 0 = secret * G, row k = (party k - 1's share) * G
  DevicePoints commit(const DeviceVector<F>& secrets, const ShareMatrix<F>& shares, std::size_t t, void* stream = nullptr) const {
    if (shares.secrets() != secrets.size() || shares.parties() < t) check(SCL_ERR_SIZE_MISMATCH);
    DevicePoints c(t + 1, secrets.size());
    check(scl_hip_feldman_commit(c.data(), c.stride(), table(), secrets.data(), shares.data(), shares.stride(), t, secrets.size(),
                                 stream));
    return c;
  }

  /// feldmanSecretShare for a batch: secret s is shared and committed to exactly as the reference would on this PRG, in order
  DeviceFeldmanSharing share(const DeviceVector<F>& secrets, std::size_t t, std::size_t n, util::PRG& prg) const {
    ShareMatrix<F> shares = ss::shamirSecretShare(secrets, t, n, prg);
    DevicePoints c = commit(secrets, shares, t, nullptr);
    return DeviceFeldmanSharing{std::move(shares), std::move(c)};
  }

  /// feldmanVerify for every secret at one index: share_dev[s] against column s of the commitments; the verdict bytes stay in
  /// HBM (1 = accepted).  Asynchronous on `stream` but for the upload of the basis, which is waited for.
  DeviceBuffer verifyOnDevice(const std::uint64_t* share_dev, const DevicePoints& commitments, std::size_t share_index,
                              void* stream = nullptr) const {
    const std::size_t N = commitments.cols(), m = commitments.rows();
    if (m == 0) check(SCL_ERR_SIZE_MISMATCH);
    const auto lb = math::computeLagrangeBasis(math::Vector<F>::range(m), static_cast<int>(share_index));
    std::vector<std::uint64_t> limbs(m * 4);
    for (std::size_t k = 0; k < m; ++k) lb[k].toLimbs(limbs.data() + k * 4);
    DeviceBuffer lambda(limbs.size() * 8), scratch(2 * N * DevicePoints::LIMBS * 8), ok(N);
    check(scl_hip_memcpy_h2d(lambda.get(), limbs.data(), limbs.size() * 8, stream));
    check(scl_hip_feldman_verify(static_cast<unsigned char*>(ok.get()), share_dev, commitments.data(), commitments.stride(), m - 1,
                                 static_cast<const std::uint64_t*>(lambda.get()), table(), static_cast<std::uint64_t*>(scratch.get()), N,
                                 stream));
    check(scl_hip_stream_sync(stream));  // `limbs`, `lambda` and `scratch` end with this call
    return ok;
  }

  /// a vector of shares (one per secret) at `share_index`: index 0 verifies the secrets themselves
  std::vector<bool> verify(const DeviceVector<F>& share, const DevicePoints& commitments, std::size_t share_index,
                           void* stream = nullptr) const {
    if (share.size() != commitments.cols()) check(SCL_ERR_SIZE_MISMATCH);
    return toHost(verifyOnDevice(share.data(), commitments, share_index, stream), share.size(), stream);
  }
  /// party `party_id`'s row of the share matrix at its index party_id + 1 (feldmanVerify(sharing.getShare(p), p + 1))
  std::vector<bool> verify(const ShareMatrix<F>& shares, std::size_t party_id, const DevicePoints& commitments,
                           void* stream = nullptr) const {
    if (party_id >= shares.parties()) check(SCL_ERR_INVALID_RANGE);
    if (shares.secrets() != commitments.cols()) check(SCL_ERR_SIZE_MISMATCH);
    return toHost(verifyOnDevice(shares.row(party_id), commitments, party_id + 1, stream), shares.secrets(), stream);
  }

 private:
  static std::vector<bool> toHost(const DeviceBuffer& ok, std::size_t n, void* stream) {
    std::vector<unsigned char> v(n);
    if (n) check(scl_hip_memcpy_d2h(v.data(), ok.get(), n, stream));
    check(scl_hip_stream_sync(stream));
    return std::vector<bool>(v.begin(), v.end());
  }
  DeviceBuffer m_table;
};

/// Vector<EC>::add over device points (what "Feldman hom" adds): a[i] + b[i]
inline DevicePoints addPoints(const DevicePoints& a, const DevicePoints& b, void* stream = nullptr) {
  if (a.rows() != b.rows() || a.cols() != b.cols()) check(SCL_ERR_SIZE_MISMATCH);
  DevicePoints out(a.rows(), a.cols());
  check(scl_hip_ec_ew(SCL_OP_ADD, out.data(), a.data(), b.data(), a.rows() * a.cols(), stream));
  return out;
}

}  // namespace scl::hip

#endif  // SCL_HIP_HIP_FELDMAN_H
