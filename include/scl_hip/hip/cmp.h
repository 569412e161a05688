// include/scl_hip/hip/cmp.h -- exact comparison over the device containers: the first level of the comparison tree fused with the
// opening of c, a later level, and the local finish, for every party's row at once.  Thin calls into the C ABI of
// libscl_hip_cmp.so (include/scl_hip_cmp.h, which states the protocol, the ranges and the status), which a program links beside
// libscl_hip.so.  The per-secret host forms are ss/compare.h.
//
// BIT PLANES are those of hip/fx.h: a ShareMatrix of `parties` rows and B * N columns.  A NODE ARRAY is a ShareMatrix of `parties`
// rows and P * N columns: plane q of a party's row is its columns [q N, (q + 1) N), plane 2j the lt and plane 2j + 1 the eq of node
// j -- what one hip::mulFinish over P * N columns leaves (hip/hm.h), used without a copy.
#ifndef SCL_HIP_HIP_CMP_H
#define SCL_HIP_HIP_CMP_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../scl_hip_cmp.h"
#include "device.h"

namespace scl::hip {

namespace cmp_detail {
/// a status of libscl_hip_cmp.so -> the exception of detail/call.h, with THAT library's diagnostic
inline void check(int status) { detail::check(status, scl_cmp_last_error); }
inline std::size_t planesOut(std::size_t nodes_in, unsigned flags) { return (flags & SCL_CMP_LT_ONLY) ? 1 : 2 * ((nodes_in + 1) / 2); }
}  // namespace cmp_detail

template <typename T>
struct CmpFirst {
  ShareMatrix<T> d;                   ///< every party's masked first-level nodes [d]_2t: open them, subtract [R]_t
  DeviceVector<T> cmod;               ///< c mod 2^w per column, public
  DeviceBuffer status;                ///< one byte per column on the device: what hip::cmpFinish reads
  std::vector<unsigned char> flagged;  ///< the same bytes on the host: 0 ok, 1 the opened c was at or above 2^(B+1)
};

/// The opening of c from its first lambda.size() rows (lambda: their Lagrange basis at 0) and the first level for every party's
/// row: bits holds B planes of N columns per party, r2 the level's degree-2t sharings as a node array.  The status bytes are
/// fetched, so the call synchronises the stream.
template <typename T>
CmpFirst<T> cmpFirstMask(const ShareMatrix<T>& c, const std::vector<T>& lambda, const ShareMatrix<T>& bits, const ShareMatrix<T>& r2, std::size_t w,
                         std::size_t B, unsigned flags = 0, void* stream = nullptr) {
  const std::size_t N = c.secrets(), P = cmp_detail::planesOut(w, flags);
  if (N == 0 || B == 0 || lambda.empty() || lambda.size() > c.parties() || bits.secrets() != B * N || r2.secrets() != P * N || r2.parties() != bits.parties())
    detail::raise(SCL_ERR_SIZE_MISMATCH);
  std::vector<std::uint64_t> lam(lambda.size() * ShareMatrix<T>::LIMBS);
  for (std::size_t j = 0; j < lambda.size(); ++j) lambda[j].toLimbs(lam.data() + j * ShareMatrix<T>::LIMBS);
  CmpFirst<T> out{ShareMatrix<T>(bits.parties(), P * N), DeviceVector<T>(N), DeviceBuffer(N), std::vector<unsigned char>(N)};
  cmp_detail::check(scl_cmp_first_mask(T::Field::TAG, out.d.data(), N, out.d.stride(), out.cmod.data(), static_cast<unsigned char*>(out.status.get()), c.data(),
                                       c.stride(), lam.data(), lambda.size(), bits.data(), N, bits.stride(), r2.data(), N, r2.stride(), w, B, bits.parties(), N,
                                       flags, stream));
  hip::check(scl_hip_stream_sync(stream));
  hip::check(scl_hip_memcpy_d2h(out.flagged.data(), out.status.get(), N, nullptr));
  return out;
}

/// A later level for every party's row: nodes holds cnt nodes (2 cnt planes of N columns), r2 the level's degree-2t sharings.
template <typename T>
ShareMatrix<T> cmpLevelMask(const ShareMatrix<T>& nodes, const ShareMatrix<T>& r2, std::size_t cnt, unsigned flags = 0, void* stream = nullptr) {
  if (cnt == 0 || nodes.secrets() % (2 * cnt)) detail::raise(SCL_ERR_SIZE_MISMATCH);
  const std::size_t N = nodes.secrets() / (2 * cnt), P = cmp_detail::planesOut(cnt, flags);
  if (N == 0 || r2.secrets() != P * N || r2.parties() != nodes.parties()) detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> d(nodes.parties(), P * N);
  cmp_detail::check(scl_cmp_level_mask(T::Field::TAG, d.data(), N, d.stride(), nodes.data(), N, nodes.stride(), r2.data(), N, r2.stride(), cnt, nodes.parties(),
                                       N, flags, stream));
  return d;
}

/// The finish for every party's row: lt the shares of [c' < r'] (N columns), rlow and x as hip::truncMask left and took them;
/// what: SCL_CMP_MOD (x is not looked at), SCL_CMP_TRUNC or SCL_CMP_LTZ.
template <typename T>
ShareMatrix<T> cmpFinish(const ShareMatrix<T>& lt, const CmpFirst<T>& first, const ShareMatrix<T>& rlow, const ShareMatrix<T>& x, std::size_t w, int what,
                         void* stream = nullptr) {
  const std::size_t N = lt.secrets();
  if (N == 0 || first.cmod.size() != N || rlow.secrets() != N || rlow.parties() != lt.parties() || x.secrets() != N || x.parties() != lt.parties())
    detail::raise(SCL_ERR_SIZE_MISMATCH);
  ShareMatrix<T> out(lt.parties(), N);
  cmp_detail::check(scl_cmp_finish(T::Field::TAG, out.data(), out.stride(), lt.data(), lt.stride(), first.cmod.data(),
                                   static_cast<const unsigned char*>(first.status.get()), rlow.data(), rlow.stride(), x.data(), x.stride(), w, what, lt.parties(), N,
                                   stream));
  return out;
}

}  // namespace scl::hip

#endif
