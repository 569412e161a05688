// include/scl_hip/hip/pedersen.h -- Pedersen VSS over device-resident secrets: the batch form of ss::pedersenSecretShare /
// pedersenVerify / apply (include/scl/ss/pedersen.h:126-287).  The {secret, randomness} pairs and their shares are the packed
// forms of ss/shamir.h (ss::ArrayVector / ss::ArrayShares with W = 2, component-major), commitments stay in HBM as
// hip::DevicePoints ([k][secret], k = 0..t); one secret's column comes back as the types the per-secret forms use, so the two
// sides are interchangeable.  hip::Pedersen owns the window tables of the generator and of h (built once, at construction; h is
// any finite point), computes the Lagrange basis of an index with the library and uploads it.  Thin calls into the C ABI
// (scl_hip_ec_mul_two_base, scl_hip_ec_matmul, scl_hip_pedersen_*, scl_hip_matmul).
#ifndef SCL_HIP_HIP_PEDERSEN_H
#define SCL_HIP_HIP_PEDERSEN_H

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../math/array.h"
#include "../math/matrix.h"
#include "../ss/pedersen.h"
#include "../ss/shamir.h"
#include "feldman.h"

namespace scl::hip {

using PedersenGroup = FeldmanGroup;
using PedersenField = FeldmanField;
using PedersenSecrets = ss::ArrayVector<PedersenField, 2>;     ///< {secret, randomness}: 2 N elements, component-major
using PedersenShareRows = ss::ArrayShares<PedersenField, 2>;   ///< rows [2 n][N]: component j of party i is row j * n + i

/// what pedersenSecretShare returns for a batch: the packed share matrix and the commitments [t + 1][secret]
struct DevicePedersenSharing {
  PedersenShareRows shares;
  DevicePoints commitments;
  /// secret s as the per-secret form has it (ss::PedersenSharing)
  ss::PedersenSharing<PedersenGroup> sharingOf(std::size_t s) const { return {shares.sharesOf(s), commitments.column(s)}; }
};

/// What ss::apply reads and writes, for N secrets side by side: p Pedersen shares (of p sharings, all held by the same
/// party), each with its m commitments.  pairs is [p][2 N] -- row k is the N shares, then the N randomness values, of
/// sharing k --, commitments is [p][m N] -- row k is sharing k's commitments, commitment c of secret s at column c N + s.
struct DevicePedersenShares {
  ShareMatrix<PedersenField> pairs;
  DevicePoints commitments;
  std::size_t width = 0;    ///< m = t + 1
  std::size_t secrets = 0;  ///< N

  DevicePedersenShares() = default;
  DevicePedersenShares(std::size_t p, std::size_t m, std::size_t N) : pairs(p, 2 * N), commitments(p, m * N), width(m), secrets(N) {}
  /// upload: host[k][s] is the share of secret s under sharing k
  explicit DevicePedersenShares(const std::vector<std::vector<ss::PedersenShare<PedersenGroup>>>& host)
      : DevicePedersenShares(host.size(), host.empty() || host[0].empty() ? 0 : host[0][0].commitments.size(),
                             host.empty() ? 0 : host[0].size()) {
    const std::size_t p = host.size(), m = width, N = secrets;
    std::vector<std::uint64_t> sc(p * 2 * N * 4), pt(p * m * N * DevicePoints::LIMBS);
    for (std::size_t k = 0; k < p; ++k) {
      if (host[k].size() != N) check(SCL_ERR_SIZE_MISMATCH);
      for (std::size_t s = 0; s < N; ++s) {
        if (host[k][s].commitments.size() != m) check(SCL_ERR_SIZE_MISMATCH);
        host[k][s].share[0].toLimbs(sc.data() + ((k * 2 + 0) * N + s) * 4);
        host[k][s].share[1].toLimbs(sc.data() + ((k * 2 + 1) * N + s) * 4);
        for (std::size_t c = 0; c < m; ++c) host[k][s].commitments[c].toLimbs(pt.data() + ((k * m + c) * N + s) * DevicePoints::LIMBS);
      }
    }
    if (!sc.empty()) check(scl_hip_memcpy_h2d(pairs.data(), sc.data(), sc.size() * 8, nullptr));
    if (!pt.empty()) check(scl_hip_memcpy_h2d(commitments.data(), pt.data(), pt.size() * 8, nullptr));
    check(scl_hip_stream_sync(nullptr));
  }

  std::size_t size() const { return pairs.parties(); }
  const std::uint64_t* shareRow(std::size_t k) const { return pairs.row(k); }
  const std::uint64_t* randRow(std::size_t k) const { return pairs.row(k) + secrets * 4; }
  /// share k of secret s as ss::apply returns it
  ss::PedersenShare<PedersenGroup> shareOf(std::size_t k, std::size_t s) const {
    if (k >= size() || s >= secrets) check(SCL_ERR_INVALID_RANGE);
    std::uint64_t sc[8];
    std::vector<std::uint64_t> pt(width * DevicePoints::LIMBS);
    check(scl_hip_memcpy_d2h(sc, shareRow(k) + s * 4, 32, nullptr));
    check(scl_hip_memcpy_d2h(sc + 4, randRow(k) + s * 4, 32, nullptr));
    for (std::size_t c = 0; c < width; ++c)
      check(scl_hip_memcpy_d2h(pt.data() + c * DevicePoints::LIMBS, commitments.row(k) + (c * secrets + s) * DevicePoints::LIMBS,
                               DevicePoints::LIMBS * 8, nullptr));
    check(scl_hip_stream_sync(nullptr));
    ss::PedersenShare<PedersenGroup> out;
    out.share = math::Array<PedersenField, 2>{{PedersenField::fromLimbs(sc), PedersenField::fromLimbs(sc + 4)}};
    std::vector<PedersenGroup> com;
    for (std::size_t c = 0; c < width; ++c) com.emplace_back(PedersenGroup::fromLimbs(pt.data() + c * DevicePoints::LIMBS));
    out.commitments = math::Vector<PedersenGroup>(std::move(com));
    return out;
  }
};

/// The two window tables and the calls that read them.  Construction launches the kernel that fills a table, once per base.
class Pedersen {
 public:
  using F = PedersenField;
  using G = PedersenGroup;

  /// h = infinity is refused (SCL_ERR_BAD_ARG), as by scl_hip_ec_base_table
  explicit Pedersen(const G& h, void* stream = nullptr)
      : m_gtable(scl_hip_ec_base_table_bytes()), m_htable(scl_hip_ec_base_table_bytes()) {
    std::uint64_t base[DevicePoints::LIMBS];
    check(scl_hip_ec_generator(base));
    check(scl_hip_ec_base_table(m_gtable.get(), base, stream));
    h.toLimbs(base);
    check(scl_hip_ec_base_table(m_htable.get(), base, stream));
  }
  const void* gtable() const { return m_gtable.get(); }
  const void* htable() const { return m_htable.get(); }

  /// a[i] * G + b[i] * h
  DevicePoints mulTwoBase(const DeviceVector<F>& a, const DeviceVector<F>& b, void* stream = nullptr) const {
    if (a.size() != b.size()) check(SCL_ERR_SIZE_MISMATCH);
    DevicePoints out(1, a.size());
    check(scl_hip_ec_mul_two_base(out.data(), gtable(), htable(), a.data(), b.data(), a.size(), stream));
    return out;
  }

  /// the commitments of pedersenSecretShare for every secret: row 0 from {secret, randomness}, row k from party k - 1
  DevicePoints commit(const PedersenSecrets& secrets, const PedersenShareRows& shares, std::size_t t, void* stream = nullptr) const {
    const std::size_t N = secrets.secrets;
    if (shares.rows.secrets() != N || shares.rows.parties() != 2 * shares.parties) check(SCL_ERR_SIZE_MISMATCH);
    DevicePoints c(t + 1, N);
    check(scl_hip_pedersen_commit(c.data(), c.stride(), gtable(), htable(), secrets.components.data(), N, shares.rows.data(),
                                  shares.rows.stride(), t, shares.parties, N, stream));
    return c;
  }

  /// pedersenSecretShare (the 6-argument form: the randomness is the second component of `secrets`) for a batch: secret s is
  /// shared and committed to exactly as the reference would on this PRG, in order
  DevicePedersenSharing share(const PedersenSecrets& secrets, std::size_t t, std::size_t n, util::PRG& prg) const {
    PedersenShareRows shares = ss::shamirSecretShare(secrets, t, n, prg);
    DevicePoints c = commit(secrets, shares, t, nullptr);
    return DevicePedersenSharing{std::move(shares), std::move(c)};
  }

  /// pedersenVerify for every secret at one index: {share_dev[s], rand_dev[s]} against column s of the commitments ([m][stride]
  /// points at commit_dev); the verdict bytes stay in HBM (1 = accepted).  Asynchronous on `stream` but for the upload of the
  /// basis, which is waited for.
  DeviceBuffer verifyOnDevice(const std::uint64_t* share_dev, const std::uint64_t* rand_dev, const std::uint64_t* commit_dev,
                              std::size_t commit_stride, std::size_t m, std::size_t N, std::size_t share_index,
                              void* stream = nullptr) const {
    if (m == 0) check(SCL_ERR_SIZE_MISMATCH);
    const auto lb = math::computeLagrangeBasis(math::Vector<F>::range(m), static_cast<int>(share_index));
    std::vector<std::uint64_t> limbs(m * 4);
    for (std::size_t k = 0; k < m; ++k) lb[k].toLimbs(limbs.data() + k * 4);
    DeviceBuffer lambda(limbs.size() * 8), scratch(2 * N * DevicePoints::LIMBS * 8), ok(N);
    check(scl_hip_memcpy_h2d(lambda.get(), limbs.data(), limbs.size() * 8, stream));
    check(scl_hip_pedersen_verify(static_cast<unsigned char*>(ok.get()), share_dev, rand_dev, commit_dev, commit_stride, m - 1,
                                  static_cast<const std::uint64_t*>(lambda.get()), gtable(), htable(),
                                  static_cast<std::uint64_t*>(scratch.get()), N, stream));
    check(scl_hip_stream_sync(stream));  // `limbs`, `lambda` and `scratch` end with this call
    return ok;
  }
  DeviceBuffer verifyOnDevice(const std::uint64_t* share_dev, const std::uint64_t* rand_dev, const DevicePoints& commitments,
                              std::size_t share_index, void* stream = nullptr) const {
    return verifyOnDevice(share_dev, rand_dev, commitments.data(), commitments.stride(), commitments.rows(), commitments.cols(),
                          share_index, stream);
  }

  /// vectors of shares and of randomness (one each per secret) at `share_index`: index 0 verifies the secrets themselves
  std::vector<bool> verify(const DeviceVector<F>& share, const DeviceVector<F>& rand, const DevicePoints& commitments,
                           std::size_t share_index, void* stream = nullptr) const {
    if (share.size() != commitments.cols() || rand.size() != commitments.cols()) check(SCL_ERR_SIZE_MISMATCH);
    return toHost(verifyOnDevice(share.data(), rand.data(), commitments, share_index, stream), share.size(), stream);
  }
  /// the {secret, randomness} pairs themselves, at index 0
  std::vector<bool> verify(const PedersenSecrets& secrets, const DevicePoints& commitments, void* stream = nullptr) const {
    const std::size_t N = secrets.secrets;
    if (N != commitments.cols()) check(SCL_ERR_SIZE_MISMATCH);
    return toHost(verifyOnDevice(secrets.components.data(), secrets.components.data() + N * 4, commitments, 0, stream), N, stream);
  }
  /// party `party_id`'s rows of the packed share matrix at its index party_id + 1 (pedersenVerify(sharing.getShare(p), p + 1, h))
  std::vector<bool> verify(const PedersenShareRows& shares, std::size_t party_id, const DevicePoints& commitments,
                           void* stream = nullptr) const {
    if (party_id >= shares.parties) check(SCL_ERR_INVALID_RANGE);
    if (shares.rows.secrets() != commitments.cols()) check(SCL_ERR_SIZE_MISMATCH);
    return toHost(verifyOnDevice(shares.rows.row(party_id), shares.rows.row(shares.parties + party_id), commitments, party_id + 1,
                                 stream),
                  shares.rows.secrets(), stream);
  }
  /// share k of a DevicePedersenShares (an output of apply) at `share_index`, for every secret
  std::vector<bool> verify(const DevicePedersenShares& shares, std::size_t k, std::size_t share_index, void* stream = nullptr) const {
    if (k >= shares.size()) check(SCL_ERR_INVALID_RANGE);
    return toHost(verifyOnDevice(shares.shareRow(k), shares.randRow(k), shares.commitments.row(k), shares.secrets, shares.width,
                                 shares.secrets, share_index, stream),
                  shares.secrets, stream);
  }

  /// ss::apply for every secret at once: out[i] = sum_k matrix(i, k) in[k].  The {share, randomness} rows are one field matrix
  /// product (scl_hip_matmul: [rows][p] times [p][2 N]), the commitments one product of the same matrix with the points laid
  /// out [p][m N] (scl_hip_ec_matmul).  Needs no table: it is a static member.
  static DevicePedersenShares apply(const DevicePedersenShares& in, const math::Matrix<F>& matrix, void* stream = nullptr) {
    const std::size_t rows = matrix.rows(), p = matrix.cols(), N = in.secrets, m = in.width;
    if (in.size() != p) check(SCL_ERR_SIZE_MISMATCH);
    std::vector<F> flat;
    flat.reserve(rows * p);
    for (std::size_t i = 0; i < rows; ++i)
      for (std::size_t k = 0; k < p; ++k) flat.push_back(matrix(i, k));
    const DeviceVector<F> M(flat);
    DevicePedersenShares out(rows, m, N);
    if (N == 0) return out;
    check(scl_hip_matmul(SCL_SECP256K1_SCALAR, out.pairs.data(), out.pairs.stride(), M.data(), p, in.pairs.data(), in.pairs.stride(),
                         rows, p, 2 * N, stream));
    check(scl_hip_ec_matmul(out.commitments.data(), out.commitments.stride(), M.data(), rows, p, in.commitments.data(),
                            in.commitments.stride(), m * N, stream));
    check(scl_hip_stream_sync(stream));  // `M` ends with this call
    return out;
  }

 private:
  static std::vector<bool> toHost(const DeviceBuffer& ok, std::size_t n, void* stream) {
    std::vector<unsigned char> v(n);
    if (n) check(scl_hip_memcpy_d2h(v.data(), ok.get(), n, stream));
    check(scl_hip_stream_sync(stream));
    return std::vector<bool>(v.begin(), v.end());
  }
  DeviceBuffer m_gtable, m_htable;
};

}  // namespace scl::hip

#endif  // SCL_HIP_HIP_PEDERSEN_H
