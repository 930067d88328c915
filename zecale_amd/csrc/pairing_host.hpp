// Host-side Groth16 verification over BW6-761 (product code, CPU): the `wsnarkT::verify` member of
// the snark policy class (reference libzecale/tests/aggregator/aggregator_dummy_test.cpp:61-62) and
// the equation the on-chain verifier checks (contracts/Groth16BW6_761.sol:166-176):
//     e(A, B) * e(acc, -g2) * e(alpha, -beta) * e(C, -delta) = 1,   acc = ABC_0 + sum x_i ABC_i.
// Verification is not on the prover's hot path; this is a plain, serial implementation:
// reduced Tate pairing t(P, Q) = f_{r,P}(psi(Q))^((q^6-1)/r), P in G1(Fq), Q on the sextic twist
// y^2 = x^3 + 4 over Fq, untwisted into Fq6 = Fq[w]/(w^6 + 4) by psi(x', y') = (x'/w^2, y'/w^3).
// Miller lines are scaled by Fq factors and vertical lines dropped (both die in the final exponentiation);
// the four Miller loops share one accumulator (one Fq6 squaring per bit for the whole product).
#pragma once
#include <string.h>

#include <array>
#include <thread>
#include <vector>

#include "../../include/zkhip.h"
#include "combine_scalars.hpp"
#include "host_field.hpp"

namespace zkhip {
namespace host {

struct Fq6 {
  HFq c[6];   // sum c_i w^i,  w^6 = -4
  static Fq6 one() { Fq6 r; for (int i = 0; i < 6; i++) r.c[i] = HFq::zero(); r.c[0] = HFq::one(); return r; }
  bool is_one() const {
    if (c[0] != HFq::one()) return false;
    for (int i = 1; i < 6; i++) if (!c[i].is_zero()) return false;
    return true;
  }
  static HFq times_m4(const HFq& x) { HFq d = x.dbl().dbl(); return d.neg(); }
  Fq6 operator*(const Fq6& o) const {
    HFq t[11];
    for (int i = 0; i < 11; i++) t[i] = HFq::zero();
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) t[i + j] = t[i + j] + c[i] * o.c[j];
    Fq6 r;
    for (int i = 0; i < 6; i++) r.c[i] = (i + 6 < 11) ? t[i] + times_m4(t[i + 6]) : t[i];
    return r;
  }
  Fq6 sqr() const { return (*this) * (*this); }
  // multiply by the sparse line value  l0 + l3 w^3 + l4 w^4
  Fq6 mul_line(const HFq& l0, const HFq& l3, const HFq& l4) const {
    HFq t[11];
    for (int i = 0; i < 11; i++) t[i] = HFq::zero();
    for (int i = 0; i < 6; i++) {
      t[i] = t[i] + c[i] * l0;
      t[i + 3] = t[i + 3] + c[i] * l3;
      t[i + 4] = t[i + 4] + c[i] * l4;
    }
    Fq6 r;
    for (int i = 0; i < 6; i++) r.c[i] = (i + 6 < 11) ? t[i] + times_m4(t[i + 6]) : t[i];
    return r;
  }
  Fq6 pow_limbs(const uint64_t* e, int nlimbs) const {
    Fq6 acc = one();
    bool started = false;
    for (int i = nlimbs * 64 - 1; i >= 0; i--) {
      if (started) acc = acc.sqr();
      if ((e[i / 64] >> (i % 64)) & 1) { acc = started ? acc * (*this) : *this; started = true; }
    }
    return acc;
  }
};

struct MillerPair {
  HFq px, py;        // P in G1, affine
  HFq qx4, qy4;      // -xQ/4 and -yQ/4: psi(Q) = qx4 w^4 , qy4 w^3   (coefficients of w^4, w^3)
  HFq X, Y, Z;       // running T = [k] P, Jacobian
  bool done;         // T reached infinity (last addition is a vertical line)
};

// f <- f * line(T, T)(psi(Q)); T <- 2T.   Line scaled by 2 Y Z^3:
//   l = (2 Y Z^3) yq + (-3 X^2 Z^2) xq + (3 X^3 - 2 Y^2)
inline void miller_double(MillerPair& m, Fq6& f) {
  HFq XX = m.X.sqr(), YY = m.Y.sqr(), ZZ = m.Z.sqr();
  HFq threeXX = XX.dbl() + XX;
  HFq A = (m.Y * m.Z * ZZ).dbl();
  HFq B = (threeXX * ZZ).neg();
  HFq C = threeXX * m.X - YY.dbl();
  f = f.mul_line(C, A * m.qy4, B * m.qx4);
  // dbl-2009-l
  HFq YYYY = YY.sqr();
  HFq D = ((m.X + YY).sqr() - XX - YYYY).dbl();
  HFq F = threeXX.sqr();
  HFq X3 = F - D.dbl();
  HFq Y3 = threeXX * (D - X3) - YYYY.dbl().dbl().dbl();
  HFq Z3 = (m.Y * m.Z).dbl();
  m.X = X3; m.Y = Y3; m.Z = Z3;
}

// f <- f * line(T, P)(psi(Q)); T <- T + P.   Line scaled by D = Z (x2 Z^2 - X):
//   l = D yq - N xq + (N x2 - D y2),  N = y2 Z^3 - Y
inline void miller_add(MillerPair& m, Fq6& f) {
  HFq ZZ = m.Z.sqr();
  HFq H = m.px * ZZ - m.X;               // x2 Z^2 - X
  HFq N = m.py * ZZ * m.Z - m.Y;         // y2 Z^3 - Y
  if (H.is_zero()) {                     // T = +-P: for prime-order points only T = -P occurs (last step): vertical line
    m.done = true;
    return;
  }
  HFq D = m.Z * H;
  f = f.mul_line(N * m.px - D * m.py, D * m.qy4, N.neg() * m.qx4);
  // madd: X3 = N^2 - H^3 - 2 X H^2, Y3 = N (X H^2 - X3) - Y H^3, Z3 = Z H
  HFq HH = H.sqr(), HHH = HH * H, V = m.X * HH;
  HFq X3 = N.sqr() - HHH - V.dbl();
  HFq Y3 = N * (V - X3) - m.Y * HHH;
  m.X = X3; m.Y = Y3; m.Z = D;
}

// prod_i f_{r,P_i}(psi(Q_i)), the UNREDUCED Miller value.   points affine (x, y) in ABI limbs; infinity (all zero) contributes 1.
inline Fq6 miller_product(const std::vector<const uint64_t*>& g1, const std::vector<const uint64_t*>& g2) {
  std::vector<MillerPair> ms;
  HFq quarter_neg = HFq::from_u64(4).inv().neg();    // -1/4
  for (size_t i = 0; i < g1.size(); i++) {
    HFq px = HFq::from_limbs(g1[i]), py = HFq::from_limbs(g1[i] + 12);
    HFq qx = HFq::from_limbs(g2[i]), qy = HFq::from_limbs(g2[i] + 12);
    if ((px.is_zero() && py.is_zero()) || (qx.is_zero() && qy.is_zero())) continue;
    MillerPair m;
    m.px = px; m.py = py; m.qx4 = qx * quarter_neg; m.qy4 = qy * quarter_neg;
    m.X = px; m.Y = py; m.Z = HFq::one(); m.done = false;
    ms.push_back(m);
  }
  Fq6 f = Fq6::one();
  const uint64_t* r = FqParams::R_ORDER64;
  int top = 6 * 64 - 1;
  while (!((r[top / 64] >> (top % 64)) & 1)) top--;
  for (int i = top - 1; i >= 0; i--) {
    f = f.sqr();
    for (auto& m : ms) if (!m.done) miller_double(m, f);
    if ((r[i / 64] >> (i % 64)) & 1)
      for (auto& m : ms) if (!m.done) miller_add(m, f);
  }
  return f;
}

// f^((q^6-1)/r)
inline Fq6 final_exponentiation(const Fq6& f) { return f.pow_limbs(FqParams::FINAL_EXP, FqParams::FINAL_EXP_LIMBS); }

// prod_i t(P_i, Q_i), the reduced value
inline Fq6 pairing_product_value(const std::vector<const uint64_t*>& g1, const std::vector<const uint64_t*>& g2) {
  return final_exponentiation(miller_product(g1, g2));
}

// ---- combined batches: ONE check for a whole batch of proofs (A_i, B_i, C_i), inputs x_i, under one key, with independent non-zero
// 128-bit scalars rho_i:
//     prod_i t(rho_i A_i, B_i) * t(S_acc, -g2) * t(sigma alpha, -beta) * t(S_C, -delta) == 1,
//     sigma = sum rho_i,  S_acc = sigma ABC_0 + sum_j (sum_i rho_i x_ij) ABC_j,  S_C = sum rho_i C_i.
// GT has prime order r: when every point has order r, a batch with an invalid proof passes with probability about 2^-128.
// The per-proof pairs' Miller values come from the device (pairing.hip) or from combined_proofs_host below; the three shared pairs and
// the single final exponentiation are combined_value, the same code behind both routes.

struct CombineKey {      // ABI limbs; the G2 points already negated
  const uint64_t *alpha, *neg_g2, *neg_beta, *neg_delta, *abc;
  size_t n_inputs;
};

// sigma and the n_inputs sums of rho_i x_ij in Fr, proof after proof
struct CombineSums {
  HFr sigma;
  std::vector<HFr> s;
  explicit CombineSums(size_t n_inputs) : sigma(HFr::zero()), s(n_inputs, HFr::zero()) {}
  void add(const uint64_t* rho /* 2 words */, const uint64_t* inputs /* n_inputs x 6 ABI limbs */) {
    const uint64_t k[6] = {rho[0], rho[1], 0, 0, 0, 0};
    const HFr r = HFr::from_canonical(k);
    sigma = sigma + r;
    for (size_t j = 0; j < s.size(); j++) s[j] = s[j] + r * HFr::from_limbs(inputs + j * 6);
  }
};

// (draw_rho, the scalars of a combined batch, is combine_scalars.hpp's: the nested verifier's combined route draws them too)

inline Fq6 fq6_from_limbs(const uint64_t* p) { Fq6 r; for (int k = 0; k < 6; k++) r.c[k] = HFq::from_limbs(p + k * 12); return r; }
inline void fq6_to_limbs(const Fq6& f, uint64_t* p) { for (int k = 0; k < 6; k++) f.c[k].to_limbs(p + k * 12); }
inline HJac jac_from_limbs(const uint64_t* p) { return HJac::from_affine(HFq::from_limbs(p), HFq::from_limbs(p + 12)); }
inline void jac_to_limbs(const HJac& P, uint64_t* o) { HFq x, y; P.to_affine(x, y); x.to_limbs(o); y.to_limbs(o + 12); }

// the reduced value of the combined product: the three shared pairs' Miller value times `proofs_product` (the unreduced
// prod_i f(rho_i A_i, B_i)), then ONE final exponentiation
inline Fq6 combined_value(const CombineKey& key, const CombineSums& sums, const HJac& s_c, const Fq6& proofs_product) {
  uint64_t k[6], pts[3][24];
  sums.sigma.to_canonical(k);
  HJac s_acc = jac_from_limbs(key.abc).mul_canonical(k, 6);
  jac_to_limbs(jac_from_limbs(key.alpha).mul_canonical(k, 6), pts[1]);
  for (size_t j = 0; j < key.n_inputs; j++) {
    sums.s[j].to_canonical(k);
    s_acc = s_acc.add(jac_from_limbs(key.abc + (j + 1) * 24).mul_canonical(k, 6));
  }
  jac_to_limbs(s_acc, pts[0]);
  jac_to_limbs(s_c, pts[2]);
  const Fq6 shared = miller_product({pts[0], pts[1], pts[2]}, {key.neg_g2, key.neg_beta, key.neg_delta});
  return final_exponentiation(shared * proofs_product);
}

// the host route's share of the per-proof work: prod_i f(rho_i A_i, B_i) (unreduced), S_C, and the sums, over the proofs that `skip`
// (null, or one byte per proof) does not leave out; the proofs are dealt to `threads` threads, each with its own partial results.
inline void combined_proofs_host(size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                                 const uint8_t* skip, unsigned threads, Fq6& product, HJac& s_c, CombineSums& sums) {
  if (threads < 1) threads = 1;
  if (threads > count) threads = count ? (unsigned)count : 1;
  std::vector<Fq6> part_f(threads, Fq6::one());
  std::vector<HJac> part_c(threads, HJac::infinity());
  auto work = [&](unsigned t) {
    for (size_t i = t; i < count; i += threads) {
      if (skip && skip[i]) continue;
      const uint64_t* pr = proofs + i * 72;
      uint64_t ra[24];
      jac_to_limbs(jac_from_limbs(pr).mul_canonical(rho + i * 2, 2), ra);
      part_f[t] = part_f[t] * miller_product({ra}, {pr + 24});
      part_c[t] = part_c[t].add(jac_from_limbs(pr + 48).mul_canonical(rho + i * 2, 2));
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  product = Fq6::one();
  s_c = HJac::infinity();
  for (unsigned t = 0; t < threads; t++) { product = product * part_f[t]; s_c = s_c.add(part_c[t]); }
  for (size_t i = 0; i < count; i++) if (!skip || !skip[i]) sums.add(rho + i * 2, inputs + i * n_inputs * 6);
}

// The checks of the checked verifier for one point (x | y, 24 ABI limbs), in their order: 0, or ZKHIP_VERIFY_ENCODING (a
// coordinate >= q), ZKHIP_VERIFY_OFF_CURVE (neither all-zero nor on y^2 = x^3 - 1 / x^3 + 4), ZKHIP_VERIFY_NOT_ORDER_R ([r] P != O).
// The all-zero point is the point at infinity and passes.  HJac's addition is complete, so points of any order go through mul_canonical.
inline int point_check_host(const uint64_t* p, bool g2) {
  if (HFq::geq_p(p) || HFq::geq_p(p + 12)) return ZKHIP_VERIFY_ENCODING;
  const HFq x = HFq::from_limbs(p), y = HFq::from_limbs(p + 12);
  if (x.is_zero() && y.is_zero()) return 0;
  const HFq b = g2 ? HFq::one().dbl().dbl() : HFq::one().neg();
  if (y.sqr() != x.sqr() * x + b) return ZKHIP_VERIFY_OFF_CURVE;
  return HJac::from_affine(x, y).mul_canonical(FqParams::R_ORDER64, 6).is_inf() ? 0 : ZKHIP_VERIFY_NOT_ORDER_R;
}

// The codes of a checked proof's four elements (A, B, C, the inputs as one) on the host: what k_point_check writes for it, and what
// verify_refusal (pairing.cuh) turns into its status byte
inline void proof_check_codes_host(const uint64_t* proof /* 72 */, const uint64_t* inputs, size_t n_inputs, uint8_t e[4]) {
  e[0] = (uint8_t)point_check_host(proof, false);
  e[1] = (uint8_t)point_check_host(proof + 24, true);
  e[2] = (uint8_t)point_check_host(proof + 48, false);
  e[3] = ZKHIP_VERIFY_ACCEPT;
  for (size_t i = 0; i < n_inputs; i++) if (HFr::geq_p(inputs + i * 6)) e[3] = ZKHIP_VERIFY_ENCODING;
}

// prod_i t(P_i, Q_i) == 1 ?
inline bool pairing_product_is_one(const std::vector<const uint64_t*>& g1, const std::vector<const uint64_t*>& g2) {
  return pairing_product_value(g1, g2).is_one();
}

// ---- points and GT values in ABI limbs

// -P (infinity stays infinity)
inline void neg_point_abi(const uint64_t* p, uint64_t* o) {
  memcpy(o, p, 96);
  const HFq y = HFq::from_limbs(p + 12);
  const bool inf = HFq::from_limbs(p).is_zero() && y.is_zero();
  (inf ? y : y.neg()).to_limbs(o + 12);
}

// -g2, the second member of the pair of acc
inline void neg_g2_generator(uint64_t o[24]) {
  uint64_t g2[24];
  memcpy(g2, FqParams::G2_GEN_X64, 96);
  memcpy(g2 + 12, FqParams::G2_GEN_Y64, 96);
  neg_point_abi(g2, o);
}

// a GT value (6 x 12 limbs) is one
inline bool gt_is_one(const uint64_t* value) {
  static const std::array<uint64_t, 72> one = [] {
    std::array<uint64_t, 72> v = {};
    HFq::one().to_limbs(v.data());
    return v;
  }();
  return memcmp(value, one.data(), sizeof one) == 0;
}

// y^2 = x^3 - 1 (G1) or x^3 + 4 (G2), both over Fq; the all-zero encoding of the point at infinity passes
inline bool on_curve_abi(const uint64_t* p, bool g2) {
  const HFq x = HFq::from_limbs(p), y = HFq::from_limbs(p + 12);
  if (x.is_zero() && y.is_zero()) return true;
  const HFq rhs = x.sqr() * x + (g2 ? HFq::one().dbl().dbl() : HFq::one().neg());
  return y.sqr() == rhs;
}

// well-formedness (libsnark: is_well_formed()) of a key's n_inputs + 4 points and of a proof's three: an off-curve point would put
// the pairing in an invalid-curve setting
inline bool key_on_curve(const uint64_t* alpha, const uint64_t* beta, const uint64_t* delta, const uint64_t* abc, size_t n_inputs) {
  bool wf = on_curve_abi(alpha, false) && on_curve_abi(beta, true) && on_curve_abi(delta, true);
  for (size_t i = 0; i <= n_inputs && wf; i++) wf = on_curve_abi(abc + i * 24, false);
  return wf;
}
inline bool proof_on_curve(const uint64_t* proof /* 72 */) {
  return on_curve_abi(proof, false) && on_curve_abi(proof + 24, true) && on_curve_abi(proof + 48, false);
}

}  // namespace host
}  // namespace zkhip
