// tests/cxx/test_ecdsa_api.cc -- the signature half of the C++ mirror on the host: util::ECDSA and util::Signature<ECDSA>
// (include/scl_hip/util/sign.h) and the functions they stand on (detail/secp256k1.hpp: rinv, ecdsa_conversion, pt_x_is,
// pt_mul_window).
//
//   test_ecdsa_api <cases-file> [--device]
// The cases file is written by the Python test that drives this binary (tests/test_ecdsa_host.py) from what the REFERENCE
// computed (tests/golden/golden_ecdsa.json) and from its own big-integer model; one case per line, points as 65-byte images,
// scalars as 32-byte images, signatures as 64-byte images, digests as their bytes ('-' for none), all in hex:
//   mul <P> <k> <k P>                                     EC::operator* and pt_mul_window
//   derive <seed> <sk> <pk>                               SecretKey::random off the seed, then derive
//   refsign <seed> <sk> <pk> <digest> <sig> <digest> <sig>  the reference's "ECDSA sign": one key, two signatures off one PRG
//   prg <seed>                                            start a PRG ('+' for a space); `sig` lines draw from it in order
//   sig <sk> <pk> <digest> <h> <R> <conversion> <sig> <other digest> <other pk>
//                                                         sk off the PRG, Sign off the PRG, the verdicts and four tamperings
//   cross <pk> <sig> <digest> <0|1>                       verify alone
//   rinv <a> <a^-1>                                       plain integers; rinv(0) = 0
//   conv <X> <Z> <scalar>                                 ecdsa_conversion of (X : 1 : Z), plain integers in, a scalar image out
//   xis <X> <Z> <r> <0|1>                                 pt_x_is of (X : 1 : Z) against r, plain integers (Z = 0: infinity)
// With --device the batch forms of include/scl_hip/hip/ecdsa.h (hip::Ecdsa) are compared with the per-signature forms.  Besides
// those it restates both cases of the reference's test/scl/util/test_ecdsa.cc:27-48 with Sha256 in the place of Hash<256>.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "scl_hip/scl.h"

#include "check.hpp"

using namespace scl;
namespace secp = sclhip::secp;

using Curve = util::ECDSA::PublicKey;
using Scalar = util::ECDSA::SecretKey;
using Sig = util::Signature<util::ECDSA>;

static std::string hex(const unsigned char* p, std::size_t n) {
  std::string s;
  char b[3];
  for (std::size_t i = 0; i < n; ++i) {
    std::snprintf(b, sizeof b, "%02x", p[i]);
    s += b;
  }
  return s;
}
static std::string image(const Curve& p) {
  unsigned char buf[65];
  p.write(buf, false);
  return hex(buf, 65);
}
static std::string image(const Scalar& s) {
  unsigned char buf[32];
  s.write(buf);
  return hex(buf, 32);
}
static std::string image(const Sig& s) {
  unsigned char buf[64];
  s.write(buf);
  return hex(buf, Sig::byteSize());
}
static Curve pointOf(const std::string& h) { return Curve::read(unhex(h).data()); }
static Scalar scalarOf(const std::string& h) { return Scalar::read(unhex(h).data()); }
static Sig sigOf(const std::string& h) { return Sig::read(unhex(h).data()); }
static sclhip::U256 plainOf(const std::string& h) { return secp::u256_read_be(unhex(h).data()); }
static std::string plainImage(const sclhip::U256& v) {
  unsigned char buf[32];
  for (int i = 0; i < 4; ++i)
    for (int b = 0; b < 8; ++b) buf[8 * i + b] = (unsigned char)(v.w[3 - i] >> (56 - 8 * b));
  return hex(buf, 32);
}
static sclhip::U256 limbsOf(const Scalar& s) {
  sclhip::U256 r;
  s.toLimbs(r.w);
  return r;
}
static std::string seedOf(std::string s) {
  for (char& c : s)
    if (c == '+') c = ' ';
  return s;
}
// (X : 1 : Z) from plain integers below p
static secp::Point synthetic(const std::string& X, const std::string& Z) {
  return secp::Point{secp::FQ::to_mont(secp::FQ::Ctx{}, plainOf(X)), secp::fone(), secp::FQ::to_mont(secp::FQ::Ctx{}, plainOf(Z))};
}

static void reference_cases() {
  {  // "ECDSA derive"
    auto prg = util::PRG::create("ecdsa derive");
    const auto sk = util::ECDSA::SecretKey::random(prg);
    const auto pk = util::ECDSA::derive(sk);
    REQUIRE(pk == sk * Curve::generator());
  }
  {  // "ECDSA sign", Sha256 for Hash<256>
    auto prg = util::PRG::create("ecdsa sign");
    const auto m = util::Sha256{}.update("message").finalize();
    const auto sk = util::ECDSA::SecretKey::random(prg);
    const auto sig = util::ECDSA::Sign(sk, m, prg);
    const auto pk = util::ECDSA::derive(sk);
    REQUIRE(util::ECDSA::verify(pk, sig, m));
    const std::array<unsigned char, 3> m_small = {1, 2, 3};
    const auto sig_small = util::ECDSA::Sign(sk, m_small, prg);
    REQUIRE(util::ECDSA::verify(pk, sig_small, m_small));
    REQUIRE(!util::ECDSA::verify(pk, sig_small, m));
    // the signature's image, and s == 0
    REQUIRE(Sig::byteSize() == 64);
    unsigned char buf[64], again[64];
    sig.write(buf);
    const Sig back = Sig::read(buf);
    back.write(again);
    REQUIRE(back.r == sig.r && back.s == sig.s && std::memcmp(buf, again, 64) == 0);
    bool threw = false;
    try {
      (void)util::ECDSA::verify(pk, Sig{sig.r, Scalar::zero()}, m);
    } catch (const std::logic_error& e) {
      threw = std::string(e.what()) == "0 not invertible modulo prime";
    }
    REQUIRE(threw);
    REQUIRE(!util::ECDSA::verify(pk, Sig{Scalar::zero(), sig.s}, m));
    REQUIRE(util::ECDSA::conversionFunc(Curve::zero()) == Scalar::zero());
  }
  {  // digestToElement at the six lengths: short digests fill the front, long ones give their first 32 bytes
    auto prg = util::PRG::create("digest lengths");
    for (std::size_t len : {0u, 1u, 31u, 32u, 33u, 64u}) {
      std::vector<unsigned char> d(len);
      if (len) prg.next(d.data(), len);
      unsigned char buf[32] = {0};
      std::memcpy(buf, d.data(), std::min<std::size_t>(len, 32));
      REQUIRE(util::ECDSA::digestToElement(d) == Scalar::read(buf));
    }
    REQUIRE(util::ECDSA::digestToElement(std::vector<unsigned char>{}) == Scalar::zero());
    REQUIRE(util::ECDSA::digestToElement(std::vector<unsigned char>{1}) ==
            Scalar::fromString("0100000000000000000000000000000000000000000000000000000000000000"));
  }
}

// hip::Ecdsa against util::ECDSA, signature by signature
static void device_cases() {
  const std::size_t n = 65;
  auto kprg = util::PRG::create("device ecdsa");
  std::vector<Scalar> sk, nonces;
  std::vector<util::Digest<256>> digests;
  for (std::size_t i = 0; i < n; ++i) {
    sk.push_back(Scalar::random(kprg));
    nonces.push_back(Scalar::random(kprg));
    digests.push_back(util::Sha256{}.update(std::vector<unsigned char>(i + 1, (unsigned char)i)).finalize());
  }
  const hip::Ecdsa ecdsa;
  const hip::DeviceVector<Scalar> dsk(sk), dnonces(nonces);
  const hip::DeviceBuffer dd = hip::Ecdsa::digests(digests);
  // derive
  const hip::DevicePoints dpk = ecdsa.derive(dsk);
  const auto pk = dpk.toHost();
  REQUIRE(pk.size() == n && image(pk[7]) == image(util::ECDSA::derive(sk[7])) && image(pk[64]) == image(util::ECDSA::derive(sk[64])));
  // sign with a key per signature: the host's Sign off a PRG that yields the same nonce is what the reference computes; here
  // the nonce is given, so compare with the formula's parts, and verify on both sides
  bool zero = true;
  const hip::DeviceVector<Scalar> dsig = ecdsa.sign(dsk, dnonces, dd, &zero);
  REQUIRE(!zero);
  const auto sig = dsig.toHost();
  REQUIRE(sig.size() == 2 * n);
  for (std::size_t i : {std::size_t(0), std::size_t(1), std::size_t(63), std::size_t(64)}) {
    const Scalar r = util::ECDSA::conversionFunc(nonces[i] * Curve::generator());
    const Scalar s = nonces[i].inverse() * (util::ECDSA::digestToElement(digests[i]) + sk[i] * r);
    REQUIRE(sig[2 * i] == r && sig[2 * i + 1] == s);
    REQUIRE(util::ECDSA::verify(pk[i], Sig{sig[2 * i], sig[2 * i + 1]}, digests[i]));
  }
  const auto ok = ecdsa.verify(dpk, dsig, dd);
  REQUIRE(ok.size() == n && std::count(ok.begin(), ok.end(), 1) == (std::ptrdiff_t)n);
  // planted: s + 1 at 0, s = 0 at 33, r + 1 at 64
  auto bad = sig;
  bad[1] += Scalar::one();
  bad[2 * 33 + 1] = Scalar::zero();
  bad[2 * 64] += Scalar::one();
  const auto planted = ecdsa.verify(dpk, hip::DeviceVector<Scalar>(bad), dd);
  for (std::size_t i = 0; i < n; ++i) REQUIRE(planted[i] == (i == 33 ? 2 : (i == 0 || i == 64) ? 0 : 1));
  REQUIRE(!util::ECDSA::verify(pk[0], Sig{bad[0], bad[1]}, digests[0]));
  // one signer: one key for all lanes through sign and verify (stride 0), and through the key's own table
  const hip::DeviceVector<Scalar> one(std::vector<Scalar>{sk[5]});
  const hip::DevicePoints onepk(std::vector<Curve>{pk[5]});
  const hip::DeviceVector<Scalar> dsig1 = ecdsa.sign(one, dnonces, dd);
  const auto v1 = ecdsa.verify(onepk, dsig1, dd);
  const auto v2 = ecdsa.verifyOneSigner(pk[5], dsig1, dd);
  REQUIRE(std::count(v1.begin(), v1.end(), 1) == (std::ptrdiff_t)n && v1 == v2);
  const auto v3 = ecdsa.verifyOneSigner(pk[6], dsig1, dd);
  REQUIRE(std::count(v3.begin(), v3.end(), 0) == (std::ptrdiff_t)n);
  const auto s1 = dsig1.toHost();
  REQUIRE(util::ECDSA::verify(pk[5], Sig{s1[2 * 40], s1[2 * 40 + 1]}, digests[40]));
  // a zero nonce is reported
  auto zn = nonces;
  zn[3] = Scalar::zero();
  bool flagged = false;
  const auto zs = ecdsa.sign(dsk, hip::DeviceVector<Scalar>(zn), dd, &flagged).toHost();
  REQUIRE(flagged && zs[6] == Scalar::zero() && zs[7] == Scalar::zero() && zs[8] == sig[8] && zs[4] == sig[4]);
  // conversion and the per-lane multiplication
  const auto R = ecdsa.mul(dnonces, dpk).toHost();
  REQUIRE(R.size() == n && R[9] == nonces[9] * pk[9] && R[64] == nonces[64] * pk[64]);
  const auto conv = ecdsa.conversion(dpk).toHost();
  REQUIRE(conv.size() == n && conv[11] == util::ECDSA::conversionFunc(pk[11]));
  std::printf("device: %zu signatures compared\n", n);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: test_ecdsa_api <cases-file> [--device]\n");
    return 2;
  }
  reference_cases();
  if (argc > 2 && std::string(argv[2]) == "--device") device_cases();
  std::ifstream in(argv[1]);
  std::string line;
  auto prg = util::PRG::create();
  int cases = 0;
  while (std::getline(in, line)) {
    const auto f = split(line, ' ');
    if (f.empty()) continue;
    ++cases;
    if (f[0] == "mul" && f.size() == 4) {
      const Curve P = pointOf(f[1]);
      const Scalar k = scalarOf(f[2]);
      REQUIRE(image(k * P) == f[3]);
      std::uint64_t limbs[secp::POINT_LIMBS], table[secp::MUL_TABLE_ENTRIES * secp::POINT_LIMBS];
      P.toLimbs(limbs);
      secp::pt_store(limbs, secp::pt_mul_window(secp::pt_load(limbs), secp::scalar_plain(limbsOf(k)), table, secp::POINT_LIMBS));
      REQUIRE(image(Curve::fromLimbs(limbs)) == f[3]);
    } else if (f[0] == "derive" && f.size() == 4) {
      auto p = util::PRG::create(seedOf(f[1]));
      const Scalar sk = Scalar::random(p);
      REQUIRE(image(sk) == f[2] && image(util::ECDSA::derive(sk)) == f[3]);
    } else if (f[0] == "refsign" && f.size() == 8) {
      auto p = util::PRG::create(seedOf(f[1]));
      const Scalar sk = Scalar::random(p);
      const Curve pk = util::ECDSA::derive(sk);
      REQUIRE(image(sk) == f[2] && image(pk) == f[3]);
      const auto d1 = unhex(f[4]), d2 = unhex(f[6]);
      const Sig s1 = util::ECDSA::Sign(sk, d1, p), s2 = util::ECDSA::Sign(sk, d2, p);
      REQUIRE(image(s1) == f[5] && image(s2) == f[7]);
      REQUIRE(util::ECDSA::verify(pk, s1, d1) && util::ECDSA::verify(pk, s2, d2) && !util::ECDSA::verify(pk, s2, d1));
    } else if (f[0] == "prg" && f.size() == 2) {
      prg = util::PRG::create(seedOf(f[1]));
    } else if (f[0] == "sig" && f.size() == 10) {
      const Scalar sk = Scalar::random(prg);
      REQUIRE(image(sk) == f[1]);
      const Curve pk = util::ECDSA::derive(sk);
      REQUIRE(image(pk) == f[2]);
      const auto d = unhex(f[3]);
      REQUIRE(image(util::ECDSA::digestToElement(d)) == f[4]);
      const Sig sig = util::ECDSA::Sign(sk, d, prg);
      REQUIRE(image(sig) == f[7]);
      REQUIRE(image(sigOf(f[7])) == f[7]);
      REQUIRE(image(util::ECDSA::conversionFunc(pointOf(f[5]))) == f[6] && f[6] == f[7].substr(0, 64));
      REQUIRE(util::ECDSA::verify(pk, sig, d));
      REQUIRE(!util::ECDSA::verify(pk, Sig{sig.r + Scalar::one(), sig.s}, d));
      REQUIRE(!util::ECDSA::verify(pk, Sig{sig.r, sig.s + Scalar::one()}, d));
      REQUIRE(!util::ECDSA::verify(pk, sig, unhex(f[8])));
      REQUIRE(!util::ECDSA::verify(pointOf(f[9]), sig, d));
      REQUIRE(image(util::ECDSA::derive(sk + Scalar::one())) == f[9]);
    } else if (f[0] == "cross" && f.size() == 5) {
      REQUIRE(util::ECDSA::verify(pointOf(f[1]), sigOf(f[2]), unhex(f[3])) == (f[4] == "1"));
    } else if (f[0] == "rinv" && f.size() == 3) {
      const auto a = secp::FR::to_mont(secp::FR::Ctx{}, plainOf(f[1]));
      REQUIRE(plainImage(secp::scalar_plain(secp::rinv(a))) == f[2]);
    } else if (f[0] == "conv" && f.size() == 4) {
      REQUIRE(plainImage(secp::scalar_plain(secp::ecdsa_conversion(synthetic(f[1], f[2])))) == f[3]);
    } else if (f[0] == "xis" && f.size() == 5) {
      REQUIRE(secp::pt_x_is(synthetic(f[1], f[2]), plainOf(f[3])) == (f[4] == "1"));
    } else {
      REQUIRE(!"a line of the cases file was not understood");
    }
  }
  std::printf("%d cases, %d checks, %d failures\n", cases, g_checks, g_fail);
  return g_fail ? 1 : 0;
}
