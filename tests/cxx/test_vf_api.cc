// tests/cxx/test_vf_api.cc -- batch verification in the C++ mirror: the per-instance host form of include/scl_hip/ss/vf.h and the
// shared accumulate function of include/scl_hip/detail/vf.hpp on the host, hip::combinePrg and hip::combine
// (include/scl_hip/hip/vf.h) on the GPU.
//
//   test_vf_api --host   the contents of tests/golden/golden_vf.json (the same seeds and shapes), printed in the fixture's layout
//                        -- tests/test_vf_host.py compares the two: the coins by ss::combineCoins on a util::PRG that has drawn
//                        and discarded Vector::random(3), every combination by ss::combine, which must equal vf_combine_one on
//                        the elements' limbs; the sharings by ss::shamirSecretShare; the opens by ss::shamirRecoverD / P.  Needs
//                        no GPU.
//   test_vf_api --gpu    hip::combinePrg equals ss::combine on the coins of ss::combineCoins at the same seed and counter, and
//                        hip::combine on the uploaded coins, plain and product, element for element; share -> combinePrg ->
//                        shamirRecoverD opens sum rho secret and reports an altered share.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <scl_hip/scl.h>
#include <scl_hip/detail/vf.hpp>
#include <scl_hip/hip/vf.h>
#include <scl_hip/ss/vf.h>

#include "check.hpp"

using namespace scl;

template <typename T>
static void rows(const char* key, const std::vector<math::Vector<T>>& m, const char* tail) {
  std::printf("\"%s\":[", key);
  for (std::size_t r = 0; r < m.size(); ++r) {
    std::printf("%s[", r ? "," : "");
    for (std::size_t i = 0; i < m[r].size(); ++i) std::printf("%s\"%s\"", i ? "," : "", image(m[r][i]).c_str());
    std::printf("]");
  }
  std::printf("]%s", tail);
}

// ss::combine of one row, held against vf_combine_one (the function the kernels accumulate with) on the limbs
template <typename T, class F>
static math::Vector<T> fold(const math::Vector<T>& x, const math::Vector<T>* y, const std::vector<math::Vector<T>>& rho) {
  const typename F::Ctx ctx{};
  const std::vector<T> out = y ? ss::combine(x, *y, rho) : ss::combine(x, rho);
  std::vector<typename F::E> xv, yv;
  for (std::size_t s = 0; s < x.size(); ++s) {
    xv.push_back(limbs<T, F>(x[s]));
    if (y) yv.push_back(limbs<T, F>((*y)[s]));
  }
  for (std::size_t j = 0; j < rho.size(); ++j) {
    std::vector<typename F::E> rv;
    for (std::size_t s = 0; s < x.size(); ++s) rv.push_back(limbs<T, F>(rho[j][s]));
    REQUIRE(element<T, F>(sclhip::vf_combine_one<F>(ctx, rv.data(), xv.data(), y ? yv.data() : nullptr, xv.size())) == out[j]);
  }
  return math::Vector<T>(out);
}

// the coin: "vf coin" after Vector::random(3) was drawn and discarded; *counter0 = the blocks that took
template <typename T>
static util::PRG coin(std::size_t* counter0) {
  auto prg = util::PRG::create("vf coin");
  (void)math::Vector<T>::random(3, prg);
  *counter0 = (3 * T::byteSize() + 15) / 16;
  return prg;
}

template <typename T, class F>
static void combine(const char* field, bool first) {
  auto px = util::PRG::create("vf inputs");
  auto py = util::PRG::create("vf inputs y");
  std::vector<math::Vector<T>> x, y;
  for (int r = 0; r < 3; ++r) x.push_back(math::Vector<T>::random(5, px)), y.push_back(math::Vector<T>::random(5, py));
  std::printf("%s{\"field\":\"%s\",", first ? "" : ",", field);
  rows("x", x, ",");
  rows("y", y, ",");
  std::printf("\"runs\":[");
  bool f1 = true;
  for (std::size_t N : {1, 2, 5}) {
    std::size_t counter0 = 0;
    auto pc = coin<T>(&counter0);
    const auto rho = ss::combineCoins<T>(N, 2, pc);
    std::vector<math::Vector<T>> plain, product;
    for (int r = 0; r < 3; ++r) {
      const auto xr = x[r].subVector(0, N), yr = y[r].subVector(0, N);
      plain.push_back(fold<T, F>(xr, nullptr, rho));
      product.push_back(fold<T, F>(xr, &yr, rho));
    }
    std::printf("%s{\"N\":%zu,\"counter0\":%zu,", f1 ? "" : ",", N, counter0);
    f1 = false;
    rows("plain", plain, ",");
    rows("product", product, "}");
  }
  std::printf("]}");
}

// party i's row of a [column][party] list of sharings
template <typename T>
static math::Vector<T> party_row(const std::vector<math::Vector<T>>& sh, std::size_t i) {
  std::vector<T> mine;
  for (const auto& s : sh) mine.push_back(s[i]);
  return math::Vector<T>(mine);
}

template <typename T, class F>
static void degree(const char* field, bool first) {
  const std::size_t n = 4, t = 1, N = 5, column = 3, party = 2;
  auto ps = util::PRG::create("vf secrets");
  const auto secrets = math::Vector<T>::random(N, ps);
  auto sharing = util::PRG::create("vf sharing");
  std::vector<math::Vector<T>> shares;  // [column][party]
  for (std::size_t s = 0; s < N; ++s) shares.push_back(ss::shamirSecretShare(secrets[s], t, n, sharing));
  std::size_t counter0 = 0;
  auto pc = coin<T>(&counter0);
  const auto rho = ss::combineCoins<T>(N, 1, pc);
  const auto alphas = math::Vector<T>::range(1, n + 1);
  auto all = [&](const std::vector<math::Vector<T>>& sh) {
    std::vector<T> c;
    for (std::size_t i = 0; i < n; ++i) c.push_back(fold<T, F>(party_row(sh, i), nullptr, rho)[0]);
    return math::Vector<T>(c);
  };
  const auto combined = all(shares);
  const T opened = ss::shamirRecoverD(combined, alphas, n - t, t, T{});
  REQUIRE(opened == ss::combine(secrets, rho)[0]);
  auto bad = shares;
  bad[column][party] = bad[column][party] + T(1);
  const auto combined_bad = all(bad);
  bool thrown = false;
  try {
    (void)ss::shamirRecoverD(combined_bad, alphas, n - t, t, T{});
  } catch (const std::logic_error& e) {
    thrown = std::string(e.what()).find("error detected during recovery") != std::string::npos;
  }
  REQUIRE(thrown);
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"N\":%zu,\"counter0\":%zu,\"column\":%zu,\"party\":%zu,", first ? "" : ",", field, n, t, N, counter0,
              column, party);
  elems("secrets", secrets, ",");
  elems("combined", combined, ",");
  std::printf("\"opened\":\"%s\",", image(opened).c_str());
  elems("combined_bad", combined_bad, "}");
}

template <typename T, class F>
static void product(const char* field, bool first) {
  const std::size_t n = 4, t = 1, N = 5, column = 1;
  auto pa = util::PRG::create("vf a");
  auto pb = util::PRG::create("vf b");
  const auto a = math::Vector<T>::random(N, pa), b = math::Vector<T>::random(N, pb);
  const auto c = a.multiplyEntryWise(b);
  auto sa = util::PRG::create("vf share a");
  auto sb = util::PRG::create("vf share b");
  auto sc = util::PRG::create("vf share c");
  std::vector<math::Vector<T>> as, bs, cs;  // [column][party]
  for (std::size_t s = 0; s < N; ++s) {
    as.push_back(ss::shamirSecretShare(a[s], t, n, sa));
    bs.push_back(ss::shamirSecretShare(b[s], t, n, sb));
    cs.push_back(ss::shamirSecretShare(c[s], t, n, sc));
  }
  std::size_t counter0 = 0;
  auto pc = coin<T>(&counter0);
  const auto rho = ss::combineCoins<T>(N, 1, pc);
  const T delta = T(5);
  auto check = [&](bool off) {
    std::vector<T> v;
    for (std::size_t i = 0; i < n; ++i) {
      auto ci = party_row(cs, i);
      if (off) ci[column] = ci[column] + delta;
      const auto bi = party_row(bs, i);
      v.push_back(fold<T, F>(party_row(as, i), &bi, rho)[0] - fold<T, F>(ci, nullptr, rho)[0]);
    }
    return math::Vector<T>(v);
  };
  const auto good = check(false), bad = check(true);
  REQUIRE(ss::shamirRecoverP(good) == T{});
  const T off = ss::shamirRecoverP(bad);
  REQUIRE(off == T{} - rho[0][column] * delta && !(off == T{}));
  std::printf("%s{\"field\":\"%s\",\"n\":%zu,\"t\":%zu,\"N\":%zu,\"counter0\":%zu,\"column\":%zu,\"delta\":\"%s\",", first ? "" : ",", field, n, t, N, counter0,
              column, image(delta).c_str());
  elems("a", a, ",");
  elems("b", b, ",");
  elems("v", good, ",");
  elems("v_bad", bad, ",");
  std::printf("\"off\":\"%s\"}", image(off).c_str());
}

using F61 = math::Fp<61>;
using F127 = math::Fp<127>;
using Scalar = math::FF<math::ff::Secp256k1Scalar>;

static int host() {
  std::printf("{\"combine\":[");
  combine<F61, sclhip::M61>("m61", true);
  combine<F127, sclhip::M127>("m127", false);
  combine<Scalar, sclhip::Secp256k1Scalar>("secp256k1_scalar", false);
  std::printf("],\"degree\":[");
  degree<F61, sclhip::M61>("m61", true);
  degree<F127, sclhip::M127>("m127", false);
  degree<Scalar, sclhip::Secp256k1Scalar>("secp256k1_scalar", false);
  std::printf("],\"product\":[");
  product<F61, sclhip::M61>("m61", true);
  product<F127, sclhip::M127>("m127", false);
  product<Scalar, sclhip::Secp256k1Scalar>("secp256k1_scalar", false);
  std::printf("]}\n");
  return summary(stderr);
}

// ---- on the device -----------------------------------------------------------------------------------------------------------
template <typename T>
static hip::ShareMatrix<T> upload(const std::vector<math::Vector<T>>& m) {
  constexpr std::size_t L = hip::DeviceVector<T>::LIMBS;
  const std::size_t N = m.empty() ? 0 : m[0].size();
  hip::ShareMatrix<T> out(m.size(), N);
  std::vector<std::uint64_t> w(m.size() * N * L);
  for (std::size_t r = 0; r < m.size(); ++r)
    for (std::size_t s = 0; s < N; ++s) m[r][s].toLimbs(w.data() + (r * N + s) * L);
  if (!w.empty()) hip::check(scl_hip_memcpy_h2d(out.data(), w.data(), w.size() * 8, nullptr));
  hip::check(scl_hip_stream_sync(nullptr));
  return out;
}
template <typename T>
static std::vector<math::Vector<T>> download(const hip::ShareMatrix<T>& m) {
  constexpr std::size_t L = hip::DeviceVector<T>::LIMBS;
  std::vector<std::uint64_t> w(m.parties() * m.secrets() * L);
  if (!w.empty()) hip::check(scl_hip_memcpy_d2h(w.data(), m.data(), w.size() * 8, nullptr));
  hip::check(scl_hip_stream_sync(nullptr));
  std::vector<math::Vector<T>> out;
  for (std::size_t r = 0; r < m.parties(); ++r) {
    std::vector<T> row;
    for (std::size_t s = 0; s < m.secrets(); ++s) row.push_back(T::fromLimbs(w.data() + (r * m.secrets() + s) * L));
    out.push_back(math::Vector<T>(row));
  }
  return out;
}
template <typename T>
static bool same(const std::vector<math::Vector<T>>& a, const std::vector<math::Vector<T>>& b) {
  if (a.size() != b.size()) return false;
  for (std::size_t r = 0; r < a.size(); ++r) {
    if (a[r].size() != b[r].size()) return false;
    for (std::size_t s = 0; s < a[r].size(); ++s)
      if (!(a[r][s] == b[r][s])) return false;
  }
  return true;
}

template <typename T, class F>
static void round_trip(const char* name, std::size_t rows_n, std::size_t N, std::size_t reps) {
  const std::string seed = std::string("vf gpu ") + name;
  auto px = util::PRG::create(seed + " x"), py = util::PRG::create(seed + " y");
  std::vector<math::Vector<T>> x, y;
  for (std::size_t r = 0; r < rows_n; ++r) x.push_back(math::Vector<T>::random(N, px)), y.push_back(math::Vector<T>::random(N, py));
  // the host coin: a PRG that has drawn and discarded counter0 blocks
  const std::size_t discard = 3, counter0 = (discard * T::byteSize() + 15) / 16;
  auto pc = util::PRG::create(seed + " coin");
  (void)math::Vector<T>::random(discard, pc);
  const auto rho = ss::combineCoins<T>(N, reps, pc);
  REQUIRE(hip::coinBlocks<T>(N) == (N * T::byteSize() + 15) / 16);
  std::vector<math::Vector<T>> plain, product;
  for (std::size_t r = 0; r < rows_n; ++r) plain.push_back(fold<T, F>(x[r], nullptr, rho)), product.push_back(fold<T, F>(x[r], &y[r], rho));
  const auto xd = upload(x), yd = upload(y), rd = upload(rho);
  const std::string cs = seed + " coin";
  const auto* sp = reinterpret_cast<const unsigned char*>(cs.data());
  REQUIRE(same(download(hip::combinePrg<T>(xd, nullptr, reps, sp, cs.size(), counter0)), plain));
  REQUIRE(same(download(hip::combinePrg<T>(xd, &yd, reps, sp, cs.size(), counter0)), product));
  REQUIRE(same(download(hip::combine<T>(xd, nullptr, rd)), plain));
  REQUIRE(same(download(hip::combine<T>(xd, &yd, rd)), product));
  bool refused = false;
  try {
    (void)hip::combinePrg<T>(xd, nullptr, 5, sp, cs.size(), counter0);
  } catch (const std::exception&) {
    refused = true;
  }
  REQUIRE(refused);
  std::printf("%s: %zu rows, N = %zu, reps = %zu: combinePrg and combine equal the host form, plain and product\n", name, rows_n, N, reps);
}

// share N secrets among n parties on the device, fold them with one coin, open: sum rho secret; an altered share is reported
template <typename T>
static void degree_gpu(const char* name, std::size_t N, std::size_t n, std::size_t t) {
  const std::string seed = std::string("vf gpu degree ") + name;
  auto ps = util::PRG::create(seed + " secrets"), sh = util::PRG::create(seed + " shares");
  const auto secrets = math::Vector<T>::random(N, ps);
  std::vector<T> sv;
  for (std::size_t s = 0; s < N; ++s) sv.push_back(secrets[s]);
  hip::ShareMatrix<T> shares = ss::shamirSecretShare(hip::DeviceVector<T>(sv), t, n, sh);
  const std::string cs = seed + " coin";
  const auto* sp = reinterpret_cast<const unsigned char*>(cs.data());
  auto pc = util::PRG::create(cs);
  const auto rho = ss::combineCoins<T>(N, 1, pc);
  // the first 2t + 1 parties' combined shares: ss::shamirRecoverD(shares, t) checks t - 1 of them against the first t + 1
  const auto folded = download(hip::combinePrg<T>(shares, nullptr, 1, sp, cs.size(), 0));
  std::vector<math::Vector<T>> first;
  for (std::size_t i = 0; i < 2 * t + 1; ++i) first.push_back(folded[i]);
  const auto opened = ss::shamirRecoverD(upload(first), t).toHost();
  REQUIRE(opened.size() == 1 && opened[0] == ss::combine(secrets, rho)[0]);
  auto bad = first;
  bad[t + 1][0] = bad[t + 1][0] + T(1);
  std::vector<std::size_t> where;
  (void)ss::shamirRecoverD(upload(bad), t, &where);
  REQUIRE(where.size() == 1 && where[0] == 0);
  std::printf("%s: N = %zu, (%zu, %zu): share, combinePrg, shamirRecoverD opens sum rho secret and reports an altered share\n", name, N, n, t);
}

static int gpu() {
  round_trip<F61, sclhip::M61>("Mersenne61", 10, 257, 2);
  round_trip<F61, sclhip::M61>("Mersenne61", 3, 4100, 4);  // past one trip of a fused workgroup
  round_trip<F127, sclhip::M127>("Mersenne127", 7, 65, 3);
  round_trip<Scalar, sclhip::Secp256k1Scalar>("secp256k1_order", 4, 33, 4);  // two launches of two repetitions
  degree_gpu<F61>("Mersenne61", 257, 10, 3);
  degree_gpu<Scalar>("secp256k1_order", 33, 7, 3);
  return summary();
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--host")) return host();
  if (argc == 2 && !std::strcmp(argv[1], "--gpu")) {
    try {
      return gpu();
    } catch (const std::exception& e) {
      std::fprintf(stderr, "FAILED: %s\n", e.what());
      return 1;
    }
  }
  std::fprintf(stderr, "usage: test_vf_api --host | --gpu\n");
  return 2;
}
