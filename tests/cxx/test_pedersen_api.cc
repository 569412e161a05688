// tests/cxx/test_pedersen_api.cc -- Pedersen VSS in the C++ mirror: ss::pedersenSecretShare / pedersenVerify / apply on the host
// (include/scl_hip/ss/pedersen.h) and, with --device, hip::Pedersen (include/scl_hip/hip/pedersen.h).
//
//   test_pedersen_api <cases-file> [--device]
// The cases file is written by the Python test that drives this binary (tests/test_pedersen_host.py) from what the REFERENCE
// computed (tests/golden/golden_pedersen.json); one case per line, points as 65-byte images, scalars as 32-byte images and a
// share as its {share, randomness} pair of 64 bytes, in hex:
//   h <h> <h'>                                           the second base (42 G) and the wrong one of the tampered inputs (43 G)
//   prg <seed>                                           start a PRG ('+' for a space); the lines that follow draw from it in order
//   draw <scalar>                                        FF::random(prg): the secret of a sharing of "Pedersen apply"
//   run <5|6> <secret> <randomness> <t> <n> <counter0> <shares> <commitment,commitment,..>
//                                                        the 5- or 6-argument overload; counter0 = the PRG block its sharing begins at
//   hom <shares> <commitment,..> <secret> <randomness>   the sums of "Pedersen hom" and the pair recovered from them
//   apply <vandermonde|identity> <party> <row> <share> <commitment,..>     one output of ss::apply over getShares(5, 2)
// Besides those it restates all four cases of the reference's test/scl/ss/test_pedersen.cc:34-136.  With --device the batch
// forms are compared with the per-secret forms secret by secret, and hip::Pedersen::apply with the `apply` lines.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "scl_hip/scl.h"

#include "check.hpp"

using namespace scl;

using EC = math::EC<math::ec::Secp256k1>;
using FF = EC::ScalarField;
using Pair = math::Array<FF, 2>;

static const EC h = EC::generator() * FF(42);

static std::string hexOf(const unsigned char* p, std::size_t n) {
  std::string s;
  char b[3];
  for (std::size_t i = 0; i < n; ++i) {
    std::snprintf(b, sizeof b, "%02x", p[i]);
    s += b;
  }
  return s;
}
static std::string image(const EC& p) {
  unsigned char buf[65];
  REQUIRE(seri::Serializer<EC>::write(p, buf) == 65);
  return hexOf(buf, 65);
}
static std::string image(const FF& s) {
  unsigned char buf[32];
  s.write(buf);
  return hexOf(buf, 32);
}
static std::string image(const Pair& p) { return image(p[0]) + image(p[1]); }
static std::string images(const math::Vector<EC>& v) {
  std::string s;
  for (std::size_t k = 0; k < v.size(); ++k) s += (k ? "," : "") + image(v[k]);
  return s;
}
static std::string images(const math::Vector<Pair>& v) {
  std::string s;
  for (std::size_t i = 0; i < v.size(); ++i) s += image(v[i]);
  return s;
}
static EC pointOf(const std::string& hex) {
  EC p;
  REQUIRE(seri::Serializer<EC>::read(p, unhex(hex).data()) == 65);
  return p;
}
static FF scalarOf(const std::string& hex) { return FF::read(unhex(hex).data()); }
// test_pedersen.cc:77-92
static std::vector<std::vector<ss::PedersenShare<EC>>> getShares(std::size_t n, std::size_t t) {
  auto prg = util::PRG::create("Pedersen apply");
  std::vector<std::vector<ss::PedersenShare<EC>>> shares(n);
  for (std::size_t i = 0; i < n; i++) {
    const auto secret = FF::random(prg);
    const auto shrs = ss::pedersenSecretShare<EC>(secret, t, n, prg, h);
    for (std::size_t j = 0; j < n; j++) shares[j].emplace_back(shrs.getShare(j));
  }
  return shares;
}

static void reference_pedersen_cases() {
  {  // "Pedersen"
    auto prg = util::PRG::create("Pedersen");
    const std::size_t t = 4;
    const auto rand = FF(42), secret = FF(123);
    const auto sb = ss::pedersenSecretShare<EC>(secret, t, 24, prg, h, rand);
    REQUIRE(sb.shares.size() == 24);
    REQUIRE(sb.commitments.size() == t + 1);
    REQUIRE(sb.commitments[0] == secret * EC::generator() + rand * h);
    const auto sh = ss::shamirRecoverP(sb.shares.subVector(t + 1));
    REQUIRE(sh[0] == secret);
    REQUIRE(sh[1] == rand);
    REQUIRE(ss::pedersenVerify<EC>({sh, sb.commitments}, 0, h));
    REQUIRE(ss::pedersenVerify<EC>(sh, sb.commitments, 0, h));
  }
  {  // "Pedersen hom"
    auto prg = util::PRG::create("Pedersen hom");
    const std::size_t t = 4;
    const auto s0 = FF(123), s1 = FF(44);
    const auto ss0 = ss::pedersenSecretShare<EC>(s0, t, 10, prg, h);
    const auto ss1 = ss::pedersenSecretShare<EC>(s1, t, 10, prg, h);
    const auto ss2 = ss0.shares.add(ss1.shares);
    const auto com2 = ss0.commitments.add(ss1.commitments);
    REQUIRE(ss::pedersenVerify<EC>({ss2[4], com2}, 5, h));
    const auto secret = ss::shamirRecoverP(ss2.subVector(t + 1));
    REQUIRE(secret[0] == s0 + s1);
    REQUIRE(ss::pedersenVerify<EC>({secret, com2}, 0, h));
  }
  const std::size_t t = 2, n = 5;
  const auto shares_in = getShares(n, t);
  {  // "Pedersen apply id"
    const auto id = math::Matrix<FF>::identity(n);
    for (std::size_t i = 0; i < n; i++) {
      const auto sin = shares_in[i];
      const auto sout = ss::apply<EC>(sin.begin(), sin.end(), id);
      REQUIRE(sout.size() == n);
      for (std::size_t j = 0; j < n && j < sout.size(); j++) {
        REQUIRE(shares_in[i][j].share == sout[j].share);
        REQUIRE(images(shares_in[i][j].commitments) == images(sout[j].commitments));
      }
    }
  }
  {  // "Pedersen apply"
    std::vector<std::vector<ss::PedersenShare<EC>>> shares_out;
    const auto van = math::Matrix<FF>::vandermonde(n - t, n);
    for (std::size_t i = 0; i < n; i++) {
      shares_out.emplace_back(ss::apply(shares_in[i], van));
      REQUIRE(shares_out[i].size() == n - t);
    }
    for (std::size_t i = 0; i < n - t; i++)
      for (std::size_t j = 0; j < n; j++) REQUIRE(ss::pedersenVerify(shares_out[j][i], j + 1, h));
  }
  REQUIRE(ss::apply<EC>(std::vector<ss::PedersenShare<EC>>{}, math::Matrix<FF>::identity(2)).empty());
}

// hip::Pedersen against ss::pedersenSecretShare / pedersenVerify, secret by secret: N secrets of (n, t) = (10, 3) off one PRG
static void device_cases(const hip::Pedersen& pedersen) {
  const std::size_t N = 65, t = 3, n = 10;
  auto sprg = util::PRG::create("device secrets");
  std::vector<Pair> secrets;
  for (std::size_t s = 0; s < N; ++s) secrets.push_back(Pair::random(sprg));
  const hip::PedersenSecrets dsecrets{math::Vector<Pair>(secrets)};
  auto dprg = util::PRG::create("device pedersen"), hprg = util::PRG::create("device pedersen");
  const hip::DevicePedersenSharing dev = pedersen.share(dsecrets, t, n, dprg);
  REQUIRE(dev.commitments.rows() == t + 1 && dev.commitments.cols() == N && dev.shares.parties == n);
  for (std::size_t s = 0; s < N; ++s) {
    const auto host = ss::pedersenSecretShare<EC>(secrets[s][0], t, n, hprg, h, secrets[s][1]);
    const auto mine = dev.sharingOf(s);
    REQUIRE(images(mine.shares) == images(host.shares));
    REQUIRE(images(mine.commitments) == images(host.commitments));
  }
  REQUIRE(dprg.counter() == hprg.counter());
  // every party and the secrets themselves verify; the host agrees on the device's commitments
  for (std::size_t p = 0; p < n; ++p) {
    const auto ok = pedersen.verify(dev.shares, p, dev.commitments);
    REQUIRE(ok.size() == N && std::count(ok.begin(), ok.end(), true) == (std::ptrdiff_t)N);
  }
  const auto ok0 = pedersen.verify(dsecrets, dev.commitments);
  REQUIRE(ok0.size() == N && std::count(ok0.begin(), ok0.end(), true) == (std::ptrdiff_t)N);
  REQUIRE(ss::pedersenVerify(dev.sharingOf(64).getShare(6), 7, h));
  // planted: party 4's share of secret 0 and its randomness of secret 64 exchanged for a neighbour's; the per-secret form
  // gives the same verdicts
  std::vector<FF> share, rand;
  for (std::size_t s = 0; s < N; ++s) {
    const auto mine = dev.shares.sharesOf(s)[4];
    share.push_back(mine[0]);
    rand.push_back(mine[1]);
  }
  share[0] = share[1];
  rand[64] = rand[63];
  const auto planted = pedersen.verify(hip::DeviceVector<FF>(share), hip::DeviceVector<FF>(rand), dev.commitments, 5);
  for (std::size_t s = 0; s < N; ++s) REQUIRE(planted[s] == !(s == 0 || s == 64));
  for (std::size_t s : {std::size_t(0), std::size_t(2), std::size_t(64)})
    REQUIRE(ss::pedersenVerify<EC>(Pair{{share[s], rand[s]}}, dev.commitments.column(s), 5, h) == planted[s]);
  // a wrong index, another h, and the homomorphism through addPoints
  const auto wrong_index = pedersen.verify(hip::DeviceVector<FF>(share), hip::DeviceVector<FF>(rand), dev.commitments, 6);
  REQUIRE(std::count(wrong_index.begin(), wrong_index.end(), true) == 0);
  const hip::Pedersen other_h(EC::generator() * FF(43));
  const auto wrong_h = other_h.verify(dev.shares, 4, dev.commitments);
  REQUIRE(std::count(wrong_h.begin(), wrong_h.end(), true) == 0);
  const hip::DevicePedersenSharing other = pedersen.share(dsecrets, t, n, dprg);
  const hip::DevicePoints com2 = hip::addPoints(dev.commitments, other.commitments);
  std::vector<FF> share5, rand5;
  for (std::size_t s = 0; s < N; ++s) {
    const auto sum = dev.shares.sharesOf(s)[5] + other.shares.sharesOf(s)[5];
    share5.push_back(sum[0]);
    rand5.push_back(sum[1]);
  }
  const auto hom = pedersen.verify(hip::DeviceVector<FF>(share5), hip::DeviceVector<FF>(rand5), com2, 6);
  REQUIRE(std::count(hom.begin(), hom.end(), true) == (std::ptrdiff_t)N);
  // mulTwoBase
  std::vector<FF> a, b;
  for (const auto& s : secrets) {
    a.push_back(s[0]);
    b.push_back(s[1]);
  }
  const auto pts = pedersen.mulTwoBase(hip::DeviceVector<FF>(a), hip::DeviceVector<FF>(b)).toHost();
  REQUIRE(pts.size() == N && pts[7] == a[7] * EC::generator() + b[7] * h && pts[64] == dev.commitments.column(64)[0]);
  bool threw = false;
  try {
    const hip::Pedersen infinity{EC::zero()};
  } catch (const std::exception&) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("device: %zu secrets of (%zu, %zu) compared\n", N, n, t);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_pedersen_api <cases-file> [--device]\n");
    return 2;
  }
  const bool device = argc > 2 && std::string(argv[2]) == "--device";
  reference_pedersen_cases();
  // ss::apply over getShares(5, 2), party by party, for the `apply` lines; on the device the five parties are the five lanes
  // of ONE batch (lane j holds party j's shares), so that a lane verifies at its own index only
  const std::size_t an = 5, at = 2;
  const auto shares_in = getShares(an, at);
  const std::map<std::string, math::Matrix<FF>> matrices = {{"vandermonde", math::Matrix<FF>::vandermonde(an - at, an)},
                                                            {"identity", math::Matrix<FF>::identity(an)}};
  std::map<std::string, std::vector<std::vector<ss::PedersenShare<EC>>>> applied;
  for (const auto& [key, m] : matrices)
    for (std::size_t j = 0; j < an; ++j) applied[key].push_back(ss::apply(shares_in[j], m));
  std::map<std::string, hip::DevicePedersenShares> dev_applied;
  if (device) {
    const hip::Pedersen pedersen(h);
    device_cases(pedersen);
    std::vector<std::vector<ss::PedersenShare<EC>>> by_sharing(an);  // [sharing k][lane = party j]
    for (std::size_t k = 0; k < an; ++k)
      for (std::size_t j = 0; j < an; ++j) by_sharing[k].push_back(shares_in[j][k]);
    const hip::DevicePedersenShares in(by_sharing);
    REQUIRE(in.size() == an && in.width == at + 1 && in.secrets == an);
    for (const auto& [key, m] : matrices) {
      dev_applied[key] = hip::Pedersen::apply(in, m);
      const auto& out = dev_applied[key];
      REQUIRE(out.size() == m.rows() && out.width == at + 1 && out.secrets == an);
      for (std::size_t i = 0; i < out.size(); ++i)
        for (std::size_t j = 0; j < an; ++j) {  // "Pedersen apply": lane j verifies at j + 1, and no other lane does
          const auto ok = pedersen.verify(out, i, j + 1);
          for (std::size_t lane = 0; lane < an; ++lane) REQUIRE(ok[lane] == (lane == j));
        }
    }
    std::printf("device apply: %zu matrices over %zu lanes\n", dev_applied.size(), an);
  }
  std::ifstream in(argv[1]);
  std::string line;
  auto prg = util::PRG::create();
  EC h_wrong;
  ss::PedersenSharing<EC> hom_a, hom_b;
  int cases = 0, hom_seen = 0;
  while (std::getline(in, line)) {
    const auto f = split(line, ' ');
    if (f.empty()) continue;
    ++cases;
    if (f[0] == "h" && f.size() == 3) {
      REQUIRE(image(h) == f[1]);
      h_wrong = pointOf(f[2]);
      REQUIRE(h_wrong == EC::generator() * FF(43));
    } else if (f[0] == "prg" && f.size() == 2) {
      std::string seed = f[1];
      for (char& c : seed)
        if (c == '+') c = ' ';
      prg = util::PRG::create(seed);
      hom_seen = seed == "Pedersen hom" ? 0 : -1;
    } else if (f[0] == "draw" && f.size() == 2) {
      REQUIRE(image(FF::random(prg)) == f[1]);
    } else if (f[0] == "run" && f.size() == 9) {
      const int overload = std::stoi(f[1]);
      const FF secret = scalarOf(f[2]), rand = scalarOf(f[3]);
      const std::size_t t = std::stoul(f[4]), n = std::stoul(f[5]), counter0 = std::stoul(f[6]);
      REQUIRE(prg.counter() + (overload == 5 ? 2 : 0) == counter0);
      const auto sh = overload == 5 ? ss::pedersenSecretShare<EC>(secret, t, n, prg, h) : ss::pedersenSecretShare<EC>(secret, t, n, prg, h, rand);
      REQUIRE(sh.shares.size() == n && images(sh.shares) == f[7]);
      REQUIRE(sh.commitments.size() == t + 1 && images(sh.commitments) == f[8]);
      REQUIRE(ss::pedersenVerify<EC>(Pair{{secret, rand}}, sh.commitments, 0, h));
      for (std::size_t p = 0; p < n; ++p) REQUIRE(ss::pedersenVerify(sh.getShare(p), p + 1, h));
      if (t >= 1) {  // the fixture's five tampered inputs: the reference answers false to each
        auto c = sh.commitments.toStlVector();
        c[0] = EC::generator();
        const Pair last = sh.shares[n - 1];
        REQUIRE(!ss::pedersenVerify<EC>(Pair{{last[0] + FF(1), last[1]}}, sh.commitments, n, h));
        REQUIRE(!ss::pedersenVerify<EC>(Pair{{last[0], last[1] + FF(1)}}, sh.commitments, n, h));
        REQUIRE(!ss::pedersenVerify<EC>(last, math::Vector<EC>{c}, n, h));
        REQUIRE(!ss::pedersenVerify<EC>(last, sh.commitments, n - 1, h));
        REQUIRE(!ss::pedersenVerify<EC>(last, sh.commitments, n, h_wrong));
      }
      if (hom_seen == 0) hom_a = sh;
      if (hom_seen == 1) hom_b = sh;
      if (hom_seen >= 0) ++hom_seen;
    } else if (f[0] == "hom" && f.size() == 5) {
      REQUIRE(hom_seen == 2);
      const auto s2 = hom_a.shares.add(hom_b.shares);
      const auto c2 = hom_a.commitments.add(hom_b.commitments);
      REQUIRE(images(s2) == f[1] && images(c2) == f[2]);
      const auto sum = ss::shamirRecoverP(s2.subVector(5));
      REQUIRE(image(sum[0]) == f[3] && image(sum[1]) == f[4] && sum[0] == FF(167));
      REQUIRE(ss::pedersenVerify<EC>({s2[4], c2}, 5, h) && ss::pedersenVerify<EC>({sum, c2}, 0, h));
    } else if (f[0] == "apply" && f.size() == 6 && applied.count(f[1])) {
      const std::size_t j = std::stoul(f[2]), i = std::stoul(f[3]);
      const auto& out = applied[f[1]];
      REQUIRE(j < out.size() && i < out[j].size());
      if (j < out.size() && i < out[j].size()) {
        REQUIRE(image(out[j][i].share) == f[4] && images(out[j][i].commitments) == f[5]);
        REQUIRE(ss::pedersenVerify(out[j][i], j + 1, h));
        if (device) {
          const auto mine = dev_applied[f[1]].shareOf(i, j);
          REQUIRE(image(mine.share) == f[4] && images(mine.commitments) == f[5]);
        }
      }
    } else {
      REQUIRE(!"a line of the cases file was not understood");
    }
  }
  std::printf("%d cases, %d checks, %d failures\n", cases, g_checks, g_fail);
  return g_fail ? 1 : 0;
}
