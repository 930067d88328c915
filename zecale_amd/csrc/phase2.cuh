// A phase-2 contribution's hot path: k P for MANY points P and ONE scalar k (phase2.hip k_common_scalar_mul, one lane per point; g++
// reads the same body through tests/phase2_host_shim.cpp).  The scalar is recoded ONCE on the host into signed binary digits in
// non-adjacent form; every lane walks the same digit array, so a wave never diverges on the scalar - only on a point at infinity, which
// leaves at once, and on the rare same-x branch of the addition.
#pragma once
#include "pairing.cuh"      // (ec.cuh's formulas, xyzz_to_affine_abi)

namespace zkhip {

// digits a recoded scalar below 2^384 can have: a non-adjacent form is at most one digit longer than the binary form
constexpr int PHASE2_MAX_DIGITS = 385;
constexpr int PHASE2_DIGIT_BUFFER = 392;      // the same, padded to a multiple of eight bytes

// k (six canonical words, little endian) -> digits d_i in {-1, 0, 1}, least significant first, no two adjacent digits non-zero,
// sum d_i 2^i = k.  Returns the number of digits (0 for k = 0); the top digit is 1.  A run of ones 0111..1 becomes 100..0-1, so k + 1
// can carry out of the sixth word: the working copy has seven.
inline int phase2_naf_recode(const uint64_t k[6], int8_t digits[PHASE2_DIGIT_BUFFER]) {
  uint64_t w[7] = {k[0], k[1], k[2], k[3], k[4], k[5], 0};
  int n = 0;
  for (;;) {
    uint64_t any = 0;
    for (int i = 0; i < 7; i++) any |= w[i];
    if (!any) break;
    int d = 0;
    if (w[0] & 1) {
      d = 2 - (int)(w[0] & 3);                  // 1 when k = 1 mod 4, -1 when k = 3 mod 4: k - d is a multiple of four
      if (d > 0) w[0] -= 1;                     // (k odd: no borrow)
      else for (int i = 0; i < 7 && ++w[i] == 0; i++) {}
    }
    digits[n++] = (int8_t)d;
    for (int i = 0; i < 6; i++) w[i] = (w[i] >> 1) | (w[i + 1] << 63);
    w[6] >>= 1;
  }
  for (int i = n; i < PHASE2_DIGIT_BUFFER; i++) digits[i] = 0;
  return n;
}

// ---- the endomorphism form.  G1 is y^2 = x^3 - 1 (j = 0): phi(x, y) = (omega x, y) is lambda (x, y) on G1, lambda^2 + lambda + 1 = 0
// mod r (tools/gen_params.py glv_params derives omega, lambda and the lattice basis; FqParams::GLV_*, FrParams::GLV_*).
// k = k1 + k2 lambda (mod r) with |k1|, |k2| < 2^GLV_BITS = 2^190: half the doublings, two recodings walked side by side.
constexpr int PHASE2_GLV_DIGITS = PHASE2_DIGIT_BUFFER / 2;      // digits of k1 at [0, 196), of k2 at [196, 392): each at most 191

namespace phase2_mp {      // little-endian words, host only
inline void mul(const uint64_t* a, int na, const uint64_t* b, int nb, uint64_t* out) {      // out: na + nb words
  for (int i = 0; i < na + nb; i++) out[i] = 0;
  for (int i = 0; i < na; i++) {
    uint64_t c = 0;
    for (int j = 0; j < nb; j++) {
      const unsigned __int128 t = (unsigned __int128)a[i] * b[j] + out[i + j] + c;
      out[i + j] = (uint64_t)t;
      c = (uint64_t)(t >> 64);
    }
    out[i + nb] = c;
  }
}
// acc (n words, two's complement) += / -= t (m <= n words, non-negative)
inline void add_sub(uint64_t* acc, int n, const uint64_t* t, int m, bool subtract) {
  uint64_t c = subtract ? 1 : 0;      // a - t = a + ~t + 1 over n words
  for (int i = 0; i < n; i++) {
    const uint64_t w = i < m ? t[i] : 0;
    const unsigned __int128 x = (unsigned __int128)acc[i] + (subtract ? ~w : w) + c;
    acc[i] = (uint64_t)x;
    c = (uint64_t)(x >> 64);
  }
}
}  // namespace phase2_mp

// k (six canonical words, below 2^384) -> k1, k2 as magnitudes of three words and signs, k1 + k2 lambda = k (mod r).  Babai rounding on the
// reduced basis (a1, b1), (a2, b2): c_i = floor((k G_i + 2^(SHIFT - 1)) / 2^SHIFT) >= 0, then k1 = k -+ c1 |a1| -+ c2 |a2| and
// k2 = -+ c1 |b1| -+ c2 |b2| in two's complement over seven words, the signs from GLV_SIGNS.  false: a half does not fit its bound
// (cannot happen for k < r: the generator checks the bound; the caller refuses rather than trusts).
inline bool phase2_glv_decompose(const uint64_t k[6], uint64_t k1[3], int* neg1, uint64_t k2[3], int* neg2) {
  using namespace phase2_mp;
  const uint64_t* G[2] = {FrParams::GLV_G1_64, FrParams::GLV_G2_64};
  uint64_t c[2][3];
  for (int i = 0; i < 2; i++) {
    uint64_t prod[15];
    mul(k, 6, G[i], 9, prod);
    const uint64_t half[9] = {0, 0, 0, 0, 0, 0, 0, 0, (uint64_t)1 << 63};
    static_assert(FrParams::GLV_SHIFT == 9 * 64, "the quotient starts at a word boundary");
    add_sub(prod, 15, half, 9, false);
    if (prod[12] | prod[13] | prod[14]) return false;
    for (int j = 0; j < 3; j++) c[i][j] = prod[9 + j];
  }
  const uint64_t* M[4] = {FrParams::GLV_A1_64, FrParams::GLV_A2_64, FrParams::GLV_B1_64, FrParams::GLV_B2_64};
  uint64_t acc[2][7] = {{k[0], k[1], k[2], k[3], k[4], k[5], 0}, {0, 0, 0, 0, 0, 0, 0}};
  for (int j = 0; j < 4; j++) {
    uint64_t t[6];
    mul(c[j & 1], 3, M[j], 3, t);
    const bool term_negative = (FrParams::GLV_SIGNS >> j) & 1;
    add_sub(acc[j >> 1], 7, t, 6, !term_negative);      // k_i -= term
  }
  uint64_t* out[2] = {k1, k2};
  int* neg[2] = {neg1, neg2};
  bool fits = true;
  for (int i = 0; i < 2; i++) {
    *neg[i] = (int)(acc[i][6] >> 63);
    if (*neg[i]) {
      uint64_t m[7] = {0, 0, 0, 0, 0, 0, 0};
      add_sub(m, 7, acc[i], 7, true);
      for (int j = 0; j < 7; j++) acc[i][j] = m[j];
    }
    fits = fits && !(acc[i][3] | acc[i][4] | acc[i][5] | acc[i][6]) && (acc[i][2] >> (FrParams::GLV_BITS - 128)) == 0;
    for (int j = 0; j < 3; j++) out[i][j] = acc[i][j];
  }
  return fits;
}

// the digit buffer of the endomorphism form: the non-adjacent forms of k1 and k2, a negative half's digits negated.  Returns the number
// of digit positions (the longer of the two), -1 when the decomposition fails.
inline int phase2_glv_recode(const uint64_t k[6], int8_t digits[PHASE2_DIGIT_BUFFER]) {
  uint64_t h[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
  int neg[2];
  if (!phase2_glv_decompose(k, h[0], &neg[0], h[1], &neg[1])) return -1;
  int n = 0;
  int8_t tmp[PHASE2_DIGIT_BUFFER];
  for (int i = 0; i < 2; i++) {
    const int ni = phase2_naf_recode(h[i], tmp);
    if (ni > PHASE2_GLV_DIGITS) return -1;
    for (int j = 0; j < PHASE2_GLV_DIGITS; j++) digits[i * PHASE2_GLV_DIGITS + j] = (int8_t)(neg[i] ? -tmp[j] : tmp[j]);
    n = ni > n ? ni : n;
  }
  volatile int8_t* v = tmp;
  for (int j = 0; j < PHASE2_DIGIT_BUFFER; j++) v[j] = 0;
  for (int i = 0; i < 2; i++) for (int j = 0; j < 6; j++) { volatile uint64_t* w = &h[i][j]; *w = 0; }
  return n;
}

// o = k p for the recoded k, by double-and-add over its digits, most significant first.  p: 24 reduced ABI limbs (x | y) of a point of
// the r-torsion (the caller's precondition: nothing is checked here); all zero is the point at infinity and stays there.  o: 24 ABI
// limbs, canonical.  The formulas of ec.cuh never use the curve's b and are complete (point_has_order_r's note): a partial sum
// that meets P or -P goes through xyzz_madd's same-x branch, and a digit array of length zero gives infinity.
// Bounds: those of point_has_order_r - acc leaves xyzz_dbl with X [6], Y [4] and xyzz_madd with X [10], Y [4], within what both accept.
// -P is added by negating the ACCUMULATOR around the addition of P (xyzz_neg: Y <- 4 p - Y, [4] again; at infinity it touches nothing
// that is read): a negated ordinate of P would be one more field element alive through the addition, and the kernel spills with it
// (51 VGPRs, 208 bytes of scratch, measured) where this form holds exactly what point_has_order_r holds.
ZK_HD ZK_INL void common_scalar_mul(const uint64_t* p, const int8_t* digits, int n_digits, uint64_t* o) {
  uint64_t nz = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) nz |= p[k];
  if (nz == 0) {
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = 0;
    return;
  }
  const Fq x = fp_from_abi<FqParams>(p), y = fp_from_abi<FqParams>(p + 12);     // [2]
  XYZZ acc = xyzz_infinity();
#pragma unroll 1
  for (int i = n_digits - 1; i >= 0; i--) {
    acc = xyzz_dbl(acc);                                                        // X [6], Y [4]
    const int d = digits[i];                                                    // the same digit on every lane
    if (d < 0) xyzz_neg(acc);                                                   // acc - P = -((-acc) + P): Y [4] (4 p - Y)
    if (d != 0) xyzz_madd(acc, x, y);                                           // X [10], Y [4]
    if (d < 0) xyzz_neg(acc);                                                   // Y [4]
  }
  xyzz_to_affine_abi(acc, o);                                                   // one inversion, 1 / (ZZ ZZZ)
}

// The same product from the endomorphism form's digits (phase2_glv_recode): o = k1 p + k2 phi(p), one doubling per digit POSITION and
// an addition of +-p / +-phi(p) where k1's / k2's digit is not zero.  phi(p) = (omega x, y) is not kept: x is multiplied by omega in
// front of such an addition and by omega^2 = 1 / omega behind it (two products on ~63 of ~190 positions) - a third live abscissa
// would be one more field element through the addition, which is what made the baseline spill.  Products keep x [2].
// Limb-identical to common_scalar_mul: both end in the canonical affine limbs of the same point.
ZK_HD ZK_INL void common_scalar_mul_glv(const uint64_t* p, const int8_t* digits, int n_digits, uint64_t* o) {
  uint64_t nz = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) nz |= p[k];
  if (nz == 0) {
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = 0;
    return;
  }
  Fq x = fp_from_abi<FqParams>(p);                                              // [2]
  const Fq y = fp_from_abi<FqParams>(p + 12);                                   // [2]
  XYZZ acc = xyzz_infinity();
#pragma unroll 1
  for (int i = n_digits - 1; i >= 0; i--) {
    acc = xyzz_dbl(acc);                                                        // X [6], Y [4]
    const int d1 = digits[i], d2 = digits[PHASE2_GLV_DIGITS + i];               // the same digits on every lane
    if (d1 != 0) {
      if (d1 < 0) xyzz_neg(acc);                                                // Y [4]
      xyzz_madd(acc, x, y);                                                     // X [10], Y [4]
      if (d1 < 0) xyzz_neg(acc);                                                // Y [4]
    }
    if (d2 != 0) {
      x = fp_mul(x, fp_const<FqParams>(FqParams::GLV_OMEGA));                   // [2]  omega x
      if (d2 < 0) xyzz_neg(acc);                                                // Y [4]
      xyzz_madd(acc, x, y);                                                     // X [10], Y [4]
      if (d2 < 0) xyzz_neg(acc);                                                // Y [4]
      x = fp_mul(x, fp_const<FqParams>(FqParams::GLV_OMEGA2));                  // [2]  x again
    }
  }
  xyzz_to_affine_abi(acc, o);                                                   // one inversion, 1 / (ZZ ZZZ)
}

}  // namespace zkhip
