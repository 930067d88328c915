// Combined batches of the nested (BLS12-377) verifier ON THE HOST: ONE check for a whole batch of proofs (A_i, B_i, C_i) with inputs x_i
// under one nested key, with independent non-zero 128-bit scalars rho_i:
//     prod_i e(rho_i A_i, B_i) * e(S_acc, -g2) * e(sigma alpha, -beta) * e(S_C, -delta) == 1,
//     sigma = sum_i rho_i (mod r),  S_acc = sigma ABC_0 + sum_j (sum_i rho_i x_ij mod r) ABC_j,  S_C = sum_i rho_i C_i,
// r the order of the nested groups, x_ij the low 253 bits of the input's canonical value (what the per-proof route reads) mod r, e the
// optimal ate pairing of circuit/bls12_377.hpp; "== 1" is tested on f^(3 (q^12 - 1) / r).  GT has prime order r: when every point has
// order r, a batch with an invalid proof passes with probability about 2^-128.
// The per-proof pairs' unreduced Miller values and the rho_i C_i come from the device (pairing_bls.hip nested_verify_all) or from
// combined_proofs_host below; the sums in the scalar field, S_acc and sigma alpha by scalar multiplication, the three shared pairs and
// the single final exponentiation are combined_value, the SAME code behind both routes.  There is no input accumulator chain: this
// route answers the group-law statement, where the per-proof route reproduces the host's affine chain.
// Host code only (the circuit DSL with the native field, nested_point_check_host.hpp's NestedJac), so that a CPU program can include it.
#pragma once
#include <string.h>

#include <thread>
#include <vector>

#include "circuit/sections.hpp"
#include "combine_scalars.hpp"
#include "nested_key.hpp"
#include "nested_point_check_host.hpp"

namespace zkhip {
namespace nested_combine {

namespace C = zkhip::circuit;
using C::NF;
using host::HFr;
using nested_key::NestedJac;
using nested_key::NESTED_R_ORDER64;
typedef unsigned __int128 u128;

// left-out bits of a proof, the values of pairing_bls.h's NESTED_OFF_CURVE and NESTED_DEGENERATE
constexpr uint8_t LEFT_OFF_CURVE = 1, LEFT_DEGENERATE = 2;

// ---- sums in the nested scalar field: sum_i rho_i x_i as a plain integer (rho < 2^128, x < 2^253: 381 bits a term, nine words hold
// 2^195 of them), reduced mod r once at the end
struct WideSum {
  uint64_t w[9];
  WideSum() { memset(w, 0, sizeof w); }
  void add_product(const uint64_t rho[2], const uint64_t x[4]) {
    for (int i = 0; i < 2; i++) {
      uint64_t carry = 0;
      for (int j = 0; j < 4; j++) {
        const u128 t = (u128)rho[i] * x[j] + w[i + j] + carry;
        w[i + j] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
      }
      for (int k = i + 4; carry && k < 9; k++) {
        const u128 t = (u128)w[k] + carry;
        w[k] = (uint64_t)t;
        carry = (uint64_t)(t >> 64);
      }
    }
  }
  // the sum mod r, four words: bit by bit from the top, rem <- 2 rem + bit, minus r when that is not below it (rem < r < 2^253)
  void reduce(uint64_t out[4]) const {
    uint64_t rem[4] = {0, 0, 0, 0};
    for (int b = 9 * 64 - 1; b >= 0; b--) {
      uint64_t in = (w[b >> 6] >> (b & 63)) & 1;
      for (int k = 0; k < 4; k++) { const uint64_t top = rem[k] >> 63; rem[k] = (rem[k] << 1) | in; in = top; }
      bool geq = true;
      for (int k = 3; k >= 0; k--) {
        if (rem[k] > NESTED_R_ORDER64[k]) break;
        if (rem[k] < NESTED_R_ORDER64[k]) { geq = false; break; }
      }
      if (!geq) continue;
      uint64_t br = 0;
      for (int k = 0; k < 4; k++) {
        const u128 t = (u128)rem[k] - NESTED_R_ORDER64[k] - br;
        rem[k] = (uint64_t)t;
        br = (uint64_t)(t >> 64) & 1;
      }
    }
    memcpy(out, rem, sizeof rem);
  }
};

// sigma and the n_inputs sums of rho_i x_ij, proof after proof
struct CombineSums {
  WideSum sigma;
  std::vector<WideSum> s;
  explicit CombineSums(size_t n_inputs) : s(n_inputs) {}
  void add(const uint64_t* rho /* 2 words */, const uint64_t* inputs /* n_inputs x 6 ABI limbs */) {
    const uint64_t one[4] = {1, 0, 0, 0};
    sigma.add_product(rho, one);
    for (size_t j = 0; j < s.size(); j++) {
      uint64_t c[6];
      HFr::from_limbs(inputs + j * 6).to_canonical(c);
      c[3] &= (1ull << (C::NESTED_INPUT_BITS - 192)) - 1;          // the low 253 bits, as the per-proof route reads them
      s[j].add_product(rho, c);
    }
  }
};

// ---- points of the nested G1: affine, or the point at infinity
struct Affine {
  HFr x, y;
  bool inf;
};
inline Affine affine_from_limbs(const uint64_t* p) { return {HFr::from_limbs(p), HFr::from_limbs(p + 6), false}; }
inline Affine to_affine(const NestedJac<HFr>& p) {
  if (p.is_inf()) return {HFr::zero(), HFr::zero(), true};
  const HFr zi = p.Z.inv(), zi2 = zi.sqr();
  return {p.X * zi2, p.Y * zi2 * zi, false};
}
// k P for a little-endian scalar of `words` words, double-and-add from the top with the complete mixed addition
inline NestedJac<HFr> scalar_mul(const Affine& p, const uint64_t* k, int words) {
  NestedJac<HFr> acc = NestedJac<HFr>::infinity();
  if (p.inf) return acc;
  for (int i = words * 64 - 1; i >= 0; i--) {
    acc = acc.dbl();
    if ((k[i >> 6] >> (i & 63)) & 1) acc = acc.add_affine(p.x, p.y);
  }
  return acc;
}
inline NestedJac<HFr> add_point(const NestedJac<HFr>& acc, const Affine& p) { return p.inf ? acc : acc.add_affine(p.x, p.y); }

// ---- Fq12 values as 72 ABI limbs
inline C::Fq12<NF> fq12_from_limbs(const uint64_t* p) {
  C::Fq12<NF> r;
  for (int k = 0; k < 12; k++) r.c[k] = NF(HFr::from_limbs(p + k * 6));
  return r;
}
inline void fq12_to_limbs(const C::Fq12<NF>& f, uint64_t* p) { for (int k = 0; k < 12; k++) f.c[k].v.to_limbs(p + k * 6); }
inline bool gt_is_one(const uint64_t* value) {
  uint64_t one[72] = {0};
  HFr::one().to_limbs(one);
  return memcmp(value, one, sizeof one) == 0;
}

// the unreduced Miller value of one pair; a point at infinity in G1 contributes one
inline C::Fq12<NF> miller_pair(const C::G2Lines<NF>& lines, const Affine& p) {
  if (p.inf) return C::Fq12<NF>::one();
  return C::multi_miller_loop<NF>({C::MillerPair<NF>{&lines, C::G1<NF>{NF(p.x), NF(p.y)}}});
}

// what the finish reads of a key: its G1 points as ABI limbs and the lines of -g2, -beta and -delta
struct CombineKey {
  const uint64_t* alpha;                       // 12 limbs
  const uint64_t* abc;                         // (n_inputs + 1) x 12 limbs
  size_t n_inputs;
  std::vector<C::G2Lines<NF>> lines;           // -beta, -delta, the negated generator: nested_key's order
};
// the lines of a key's three shared G2 points; false when a schedule is degenerate (prepare_key refuses such a key by name)
inline bool key_lines(const uint64_t* beta, const uint64_t* delta, std::vector<C::G2Lines<NF>>* out) {
  const C::BlsG2Gen& gg = C::bls_g2_gen();
  const C::G2<NF> gen{C::Fq2<NF>::constant(gg.x0, gg.x1), C::Fq2<NF>::constant(gg.y0, gg.y1)};
  const std::vector<C::G2<NF>> Qs = {C::g2_neg(C::g2_from<NF>(beta, false)), C::g2_neg(C::g2_from<NF>(delta, false)), C::g2_neg(gen)};
  for (const auto& Q : Qs) {
    std::vector<HFr> ninv;
    if (!C::g2_schedule_norm_invs(C::v2_of(Q.x), C::v2_of(Q.y), ninv)) return false;
  }
  *out = C::g2_precompute<NF>(Qs);
  return true;
}

// the reduced value of the combined product: the three shared pairs' Miller value times `proofs_product` (the unreduced
// prod_i f(rho_i A_i, B_i)), then ONE final exponentiation.  S_acc is n_inputs + 1 scalar multiplications, once per batch.
inline C::Fq12<NF> combined_value(const CombineKey& key, const CombineSums& sums, const Affine& s_c, const C::Fq12<NF>& proofs_product) {
  uint64_t k[4];
  sums.sigma.reduce(k);
  const Affine sigma_alpha = to_affine(scalar_mul(affine_from_limbs(key.alpha), k, 4));
  NestedJac<HFr> s_acc = scalar_mul(affine_from_limbs(key.abc), k, 4);
  for (size_t j = 0; j < key.n_inputs; j++) {
    sums.s[j].reduce(k);
    s_acc = add_point(s_acc, to_affine(scalar_mul(affine_from_limbs(key.abc + (j + 1) * 12), k, 4)));
  }
  const C::Fq12<NF> shared = miller_pair(key.lines[2], to_affine(s_acc)) * miller_pair(key.lines[0], sigma_alpha) * miller_pair(key.lines[1], s_c);
  return C::final_exponentiation(shared * proofs_product);
}

// the curve checks of the per-proof route on one proof (48 ABI limbs); the all-zero point is off its curve
inline bool proof_on_curves(const uint64_t* pr) {
  return nested_key::g1_on_curve(C::g1_from<NF>(pr, false)) && nested_key::g2_on_curve(C::g2_from<NF>(pr + 12, false)) &&
         nested_key::g1_on_curve(C::g1_from<NF>(pr + 36, false));
}

// the host route's share of the per-proof work: prod_i f(rho_i A_i, B_i) (unreduced), S_C and the sums over the proofs that are not
// left out.  refused: null, or one byte per proof (the checked route's refusals: nothing of such a proof is converted).  left_out gets
// per proof 0, LEFT_OFF_CURVE (refused, or a point off its curve) or LEFT_DEGENERATE (a slope denominator of B's line schedule is
// zero).  The proofs are dealt to `threads` threads, each with its own partial results.
inline void combined_proofs_host(size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                                 const uint8_t* refused, unsigned threads, C::Fq12<NF>& product, Affine& s_c, CombineSums& sums, uint8_t* left_out) {
  if (threads < 1) threads = 1;
  if (threads > count) threads = count ? (unsigned)count : 1;
  std::vector<C::Fq12<NF>> part_f(threads, C::Fq12<NF>::one());
  std::vector<NestedJac<HFr>> part_c(threads, NestedJac<HFr>::infinity());
  auto work = [&](unsigned t) {
    for (size_t i = t; i < count; i += threads) {
      const uint64_t* pr = proofs + i * 48;
      left_out[i] = 0;
      if ((refused && refused[i]) || !proof_on_curves(pr)) { left_out[i] = LEFT_OFF_CURVE; continue; }
      const C::G2<NF> B = C::g2_from<NF>(pr + 12, false);
      std::vector<HFr> ninv;
      if (!C::g2_schedule_norm_invs(C::v2_of(B.x), C::v2_of(B.y), ninv)) { left_out[i] = LEFT_DEGENERATE; continue; }
      const std::vector<C::G2Lines<NF>> lines = C::g2_precompute<NF>({B});
      part_f[t] = part_f[t] * miller_pair(lines[0], to_affine(scalar_mul(affine_from_limbs(pr), rho + i * 2, 2)));
      part_c[t] = add_point(part_c[t], to_affine(scalar_mul(affine_from_limbs(pr + 36), rho + i * 2, 2)));
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  product = C::Fq12<NF>::one();
  NestedJac<HFr> sum = NestedJac<HFr>::infinity();
  for (unsigned t = 0; t < threads; t++) { product = product * part_f[t]; sum = add_point(sum, to_affine(part_c[t])); }
  s_c = to_affine(sum);
  for (size_t i = 0; i < count; i++) if (!left_out[i]) sums.add(rho + i * 2, inputs + i * n_inputs * 6);
}

// the whole host route: the reduced value (72 ABI limbs) over the proofs not left out
inline void verify_all_host(const CombineKey& key, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                            const uint8_t* refused, unsigned threads, uint8_t* left_out, uint64_t* value) {
  CombineSums sums(key.n_inputs);
  C::Fq12<NF> product = C::Fq12<NF>::one();
  Affine s_c{HFr::zero(), HFr::zero(), true};
  combined_proofs_host(key.n_inputs, inputs, proofs, count, rho, refused, threads, product, s_c, sums, left_out);
  fq12_to_limbs(combined_value(key, sums, s_c, product), value);
}

}  // namespace nested_combine
}  // namespace zkhip
