// tests/cxx/test_feldman_api.cc -- the verifiable-sharing half of the C++ mirror on the host: math::EC<ec::Secp256k1>
// (include/scl_hip/math/ec.h) and ss::feldmanSecretShare / feldmanVerify (include/scl_hip/ss/feldman.h).
//
//   test_feldman_api <cases-file> [--device]
// The cases file is written by the Python test that drives this binary (tests/test_feldman_host.py) from what the REFERENCE
// computed (tests/golden/golden_feldman.json); one case per line, points as 65-byte images and scalars as 32-byte images in hex:
//   G <point>                                            the generator
//   mul <scalar> <point>                                 scalar * G
//   id <P> <Q> <P+Q> <P+P> <2P> <P-P> <P+inf> <-P> <P==Q: 0|1>
//   prg <seed>                                           start a PRG ('+' for a space); the runs that follow draw from it in order
//   run <secret> <t> <n> <shares> <commitment,commitment,..>
//   hom <commitment,commitment,..>                       the summed commitments of "Feldman hom"
// With --device the batch forms of include/scl_hip/hip/feldman.h (hip::Feldman over DeviceVector / ShareMatrix) are compared
// with the per-secret forms, secret by secret.  Besides those it restates both cases of the reference's test/scl/ss/test_feldman.cc:32-64 and the cases of
// test/scl/math/test_secp256k1.cc:96-260 that do not need math::Number or the compressed image.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "scl_hip/scl.h"

#include "check.hpp"

using namespace scl;

using Curve = math::EC<math::ec::Secp256k1>;
using Field = Curve::Field;
using Scalar = Curve::ScalarField;

static std::string image(const Curve& p) {
  unsigned char buf[65];
  REQUIRE(seri::Serializer<Curve>::write(p, buf) == 65);
  std::string s;
  char b[3];
  for (unsigned char c : buf) {
    std::snprintf(b, sizeof b, "%02x", c);
    s += b;
  }
  return s;
}
static Curve pointOf(const std::string& hex) {
  Curve p;
  REQUIRE(seri::Serializer<Curve>::read(p, unhex(hex).data()) == 65);
  return p;
}
static Curve randomPoint(util::PRG& prg) { return Curve::generator() * Scalar::random(prg); }

static void reference_curve_cases() {
  {  // "Secp256k1 from affine"
    const auto x = Field::fromString("e47b4a1c2e13cf0e97c9adf5a645ce388e04317b7830401aabb42e188c9883fa");
    const auto y = Field::fromString("2aafa6e870684327ec92006e6c601a8b6e0fb9ff06ae120cb330a2eee86009ff");
    const auto g = Curve::fromAffine(x, y);
    REQUIRE(!g.isPointAtInfinity());
    const auto a = g.toAffine();
    REQUIRE(a[0] == x && a[1] == y);
    bool threw = false;
    try {
      Curve::fromAffine(Field(0), Field(0));
    } catch (const std::invalid_argument& e) {
      threw = std::string(e.what()) == "provided (x, y) not on curve";
    }
    REQUIRE(threw);
  }
  REQUIRE(Curve().isPointAtInfinity());  // "Secp256k1 point-at-infinity"
  {                                      // "Secp256k1 generator" (the order as a scalar: q - 1, then + 1)
    const auto g = Curve::generator();
    REQUIRE(g.toString() == "EC{79be667ef9dcbbac55a06295ce870b07029bfcdb2dce28d959f2815b16f81798, "
                            "483ada7726a3c4655da4fbfc0e1108a8fd17b448a68554199c47d08ffb10d4b8}");
    std::stringstream ss;
    ss << g;
    REQUIRE(ss.str() == g.toString());
    REQUIRE(!g.isPointAtInfinity());
    const auto not_poi = g * Scalar(-1);
    const auto poi = not_poi + g;
    REQUIRE(poi.isPointAtInfinity() && poi != not_poi && !not_poi.isPointAtInfinity());
    REQUIRE(poi.toString() == "EC{POINT_AT_INFINITY}");
  }
  {  // "Secp256k1 addition"
    auto prg = util::PRG::create("Secp256k1 addition");
    auto a = randomPoint(prg);
    const auto b = randomPoint(prg);
    REQUIRE(a != b);
    const auto c = a + b;
    REQUIRE(a != c && b != c);
    REQUIRE(a + a == a.doublePoint());
    a += b;
    REQUIRE(a == c && a != b);
    REQUIRE((c - a).isPointAtInfinity());
    auto x = randomPoint(prg);
    const auto y = randomPoint(prg);
    const auto z = x + y;
    x.normalize();
    REQUIRE(x + y == y + x && z == x + y);
  }
  {  // "Secp256k1 negation", "negation special case"
    auto prg = util::PRG::create("Secp256k1 negation");
    const auto a = randomPoint(prg);
    REQUIRE((a + (-a)).isPointAtInfinity());
    Curve P;
    P.negate();
    REQUIRE(P.isPointAtInfinity());
  }
  {  // "Secp256k1 scalar multiplication" without its math::Number lines
    auto prg = util::PRG::create("Secp256k1 scalar-mul");
    const auto a = randomPoint(prg);
    const auto c = a * Scalar(-1);
    REQUIRE(!c.isPointAtInfinity() && (c + a).isPointAtInfinity());
    const auto x = Scalar::random(prg), y = Scalar::random(prg);
    REQUIRE((x + y) * a == x * a + y * a);
    const auto G = Curve::generator();
    REQUIRE(G * Scalar::fromString("06") == (G * Scalar::fromString("03")) * Scalar::fromString("02"));
  }
  {  // "Secp256k1 serialization", the uncompressed half
    auto prg = util::PRG::create();
    REQUIRE(Curve::byteSize() == 32 + 32 + 1);
    const auto a = randomPoint(prg);
    auto buffer = std::make_unique<unsigned char[]>(Curve::byteSize());
    a.write(buffer.get(), false);
    REQUIRE(buffer[0] == 0x04);
    REQUIRE(a == Curve::read(buffer.get()));
    Curve poi;
    poi.write(buffer.get(), false);
    REQUIRE(buffer[0] == 0x06);
    REQUIRE(Curve::read(buffer.get()).isPointAtInfinity());
    buffer[0] = 0x02;  // the compressed image of infinity is still read: the flag wins
    std::memset(buffer.get() + 1, 0xAB, 64);
    REQUIRE(Curve::read(buffer.get()).isPointAtInfinity());
    bool threw = false;
    buffer[0] = 0x01;
    try {
      Curve::read(buffer.get());
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    REQUIRE(threw);
  }
  {  // the field inversion chain of the point functions against FF::inverse
    auto prg = util::PRG::create("finv");
    for (int i = 0; i < 4; ++i) {
      const auto v = Field::random(prg);
      sclhip::U256 raw;
      v.toLimbs(raw.w);
      REQUIRE(Field::fromLimbs(sclhip::secp::finv(raw).w) == v.inverse());
    }
  }
}

static void reference_feldman_cases() {
  {  // "Feldman"
    auto prg = util::PRG::create("feldman");
    const std::size_t t = 4;
    const auto secret = Scalar(123);
    const auto sb = ss::feldmanSecretShare<Curve>(secret, 4, 24, prg);
    REQUIRE(sb.commitments[0] == secret * Curve::generator());
    REQUIRE(sb.shares.size() == 24);
    REQUIRE(sb.commitments.size() == t + 1);
    REQUIRE(ss::feldmanVerify<Curve>({secret, sb.commitments}, 0));
    REQUIRE(ss::feldmanVerify<Curve>(secret, sb.commitments, 0));
    REQUIRE(ss::feldmanVerify(sb.getShare(22), 23));
    REQUIRE(ss::shamirRecoverP(sb.shares.subVector(5)) == secret);
  }
  {  // "Feldman hom"
    auto prg = util::PRG::create("feldman hom");
    const std::size_t t = 4;
    const auto s0 = Scalar(123), s1 = Scalar(44);
    const auto ss0 = ss::feldmanSecretShare<Curve>(s0, t, 10, prg);
    const auto ss1 = ss::feldmanSecretShare<Curve>(s1, t, 10, prg);
    const auto ss2 = ss0.shares.add(ss1.shares);
    const auto com2 = ss0.commitments.add(ss1.commitments);
    REQUIRE(ss::feldmanVerify<Curve>({s0 + s1, com2}, 0));
    REQUIRE(ss::feldmanVerify<Curve>({ss2[5], com2}, 6));
  }
}

// hip::Feldman against ss::feldmanSecretShare / feldmanVerify, secret by secret: N secrets of (n, t) = (10, 3) off one PRG
static void device_cases() {
  const std::size_t N = 65, t = 3, n = 10;
  auto sprg = util::PRG::create("device secrets");
  std::vector<Scalar> secrets;
  for (std::size_t s = 0; s < N; ++s) secrets.push_back(Scalar::random(sprg));
  const hip::DeviceVector<Scalar> dsecrets(secrets);
  const hip::Feldman feldman;
  auto dprg = util::PRG::create("device feldman"), hprg = util::PRG::create("device feldman");
  const hip::DeviceFeldmanSharing dev = feldman.share(dsecrets, t, n, dprg);
  REQUIRE(dev.commitments.rows() == t + 1 && dev.commitments.cols() == N && dev.shares.parties() == n);
  for (std::size_t s = 0; s < N; ++s) {
    const auto host = ss::feldmanSecretShare<Curve>(secrets[s], t, n, hprg);
    const auto shares = dev.sharesOf(s);
    const auto com = dev.commitmentsOf(s);
    REQUIRE(shares.size() == n && com.size() == t + 1);
    bool same = shares.size() == n && com.size() == t + 1;
    for (std::size_t i = 0; same && i < n; ++i) same = shares[i] == host.shares[i];
    for (std::size_t k = 0; same && k <= t; ++k) same = image(com[k]) == image(host.commitments[k]);
    REQUIRE(same);
  }
  // every party and the secrets themselves verify; the host agrees on the device's commitments
  for (std::size_t p = 0; p < n; ++p) {
    const auto ok = feldman.verify(dev.shares, p, dev.commitments);
    REQUIRE(ok.size() == N && std::count(ok.begin(), ok.end(), true) == (std::ptrdiff_t)N);
  }
  const auto ok0 = feldman.verify(dsecrets, dev.commitments, 0);
  REQUIRE(std::count(ok0.begin(), ok0.end(), true) == (std::ptrdiff_t)N);
  REQUIRE(ss::feldmanVerify<Curve>(dev.sharesOf(64)[6], dev.commitmentsOf(64), 7));
  // planted: party 4's shares of secrets 0 and 64 exchanged for a neighbour's; the per-secret form gives the same verdicts
  std::vector<Scalar> mine;
  for (std::size_t s = 0; s < N; ++s) mine.push_back(dev.sharesOf(s)[4]);
  std::swap(mine[0], mine[1]);
  mine[64] = mine[63];
  const auto planted = feldman.verify(hip::DeviceVector<Scalar>(mine), dev.commitments, 5);
  for (std::size_t s = 0; s < N; ++s) REQUIRE(planted[s] == !(s <= 1 || s == 64));
  for (std::size_t s : {std::size_t(0), std::size_t(2), std::size_t(64)})
    REQUIRE(ss::feldmanVerify<Curve>(mine[s], dev.commitmentsOf(s), 5) == planted[s]);
  // a wrong index, and the homomorphism through addPoints
  const auto wrong_index = feldman.verify(hip::DeviceVector<Scalar>(mine), dev.commitments, 6);
  REQUIRE(std::count(wrong_index.begin(), wrong_index.end(), true) == 0);
  const hip::DeviceFeldmanSharing other = feldman.share(dsecrets, t, n, dprg);
  const hip::DevicePoints com2 = hip::addPoints(dev.commitments, other.commitments);
  std::vector<Scalar> sum5;
  for (std::size_t s = 0; s < N; ++s) sum5.push_back(dev.sharesOf(s)[5] + other.sharesOf(s)[5]);
  const auto hom = feldman.verify(hip::DeviceVector<Scalar>(sum5), com2, 6);
  REQUIRE(std::count(hom.begin(), hom.end(), true) == (std::ptrdiff_t)N);
  REQUIRE(com2.column(3)[0] == dev.commitmentsOf(3)[0] + other.commitmentsOf(3)[0]);
  // mulGenerator and the round trip of points
  const auto pts = feldman.mulGenerator(dsecrets).toHost();
  REQUIRE(pts.size() == N && pts[7] == secrets[7] * Curve::generator());
  REQUIRE(hip::DevicePoints(pts).toHost()[7] == pts[7]);
  std::printf("device: %zu secrets of (%zu, %zu) compared\n", N, n, t);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_feldman_api <cases-file> [--device]\n");
    return 2;
  }
  reference_curve_cases();
  reference_feldman_cases();
  if (argc > 2 && std::string(argv[2]) == "--device") device_cases();
  std::ifstream in(argv[1]);
  std::string line;
  auto prg = util::PRG::create();
  int cases = 0;
  while (std::getline(in, line)) {
    const auto f = split(line, ' ');
    if (f.empty()) continue;
    ++cases;
    if (f[0] == "G" && f.size() == 2) {
      REQUIRE(image(Curve::generator()) == f[1]);
    } else if (f[0] == "mul" && f.size() == 3) {
      const auto k = Scalar::read(unhex(f[1]).data());
      const auto p = k * Curve::generator();
      REQUIRE(image(p) == f[2]);
      REQUIRE(pointOf(f[2]) == p);
      REQUIRE(image(pointOf(f[2])) == f[2]);
    } else if (f[0] == "id" && f.size() == 10) {
      const auto P = pointOf(f[1]), Q = pointOf(f[2]);
      const auto sum = P + Q;
      auto flat = sum;
      flat.normalize();
      REQUIRE(image(sum) == f[3]);
      REQUIRE(image(P + P) == f[4]);
      REQUIRE(image(P.doublePoint()) == f[5]);
      REQUIRE(image(P - P) == f[6] && (P - P).isPointAtInfinity());
      REQUIRE(image(P + Curve::zero()) == f[7]);
      REQUIRE(image(Curve::zero() + P) == f[7]);
      REQUIRE(image(-P) == f[8]);
      REQUIRE(sum == flat && flat == sum && image(flat) == f[3]);
      REQUIRE((P == Q) == (f[9] == "1"));
    } else if (f[0] == "prg" && f.size() == 2) {
      std::string seed = f[1];
      for (char& c : seed)
        if (c == '+') c = ' ';
      prg = util::PRG::create(seed);
    } else if (f[0] == "run" && f.size() == 6) {
      const int secret = std::stoi(f[1]);
      const std::size_t t = std::stoul(f[2]), n = std::stoul(f[3]);
      const auto sh = ss::feldmanSecretShare<Curve>(Scalar(secret), t, n, prg);
      std::vector<unsigned char> shares(32 * n);
      for (std::size_t i = 0; i < n; ++i) sh.shares[i].write(shares.data() + 32 * i);
      REQUIRE(shares == unhex(f[4]));
      const auto want = split(f[5], ',');
      REQUIRE(want.size() == t + 1 && sh.commitments.size() == t + 1);
      for (std::size_t k = 0; k <= t && k < want.size(); ++k) REQUIRE(image(sh.commitments[k]) == want[k]);
      REQUIRE(ss::feldmanVerify<Curve>(Scalar(secret), sh.commitments, 0));
      for (std::size_t p = 0; p < n; ++p) REQUIRE(ss::feldmanVerify(sh.getShare(p), p + 1));
      if (t >= 1) {  // the fixture's three tampered inputs: the reference answers false to each
        auto c = sh.commitments.toStlVector();
        c[0] = Curve::generator();
        REQUIRE(!ss::feldmanVerify<Curve>(sh.shares[n - 1] + Scalar(1), sh.commitments, n));
        REQUIRE(!ss::feldmanVerify<Curve>(sh.shares[n - 1], math::Vector<Curve>{c}, n));
        REQUIRE(!ss::feldmanVerify<Curve>(sh.shares[n - 1], sh.commitments, n - 1));
      }
    } else if (f[0] == "hom" && f.size() == 2) {
      auto hp = util::PRG::create("feldman hom");
      const auto a = ss::feldmanSecretShare<Curve>(Scalar(123), 4, 10, hp);
      const auto b = ss::feldmanSecretShare<Curve>(Scalar(44), 4, 10, hp);
      const auto c2 = a.commitments.add(b.commitments);
      const auto want = split(f[1], ',');
      REQUIRE(want.size() == c2.size());
      for (std::size_t k = 0; k < c2.size() && k < want.size(); ++k) REQUIRE(image(c2[k]) == want[k]);
    } else {
      REQUIRE(!"a line of the cases file was not understood");
    }
  }
  std::printf("%d cases, %d checks, %d failures\n", cases, g_checks, g_fail);
  return g_fail ? 1 : 0;
}
