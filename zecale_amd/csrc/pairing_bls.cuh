// The optimal-ate pairing of BLS12-377 (the NESTED curve; circuit/bls12_377.hpp is the host route) cut into per-lane bodies for the
// device (pairing_bls.hip) and for g++ (tests/nested_pairing_host_shim.cpp).  The nested base field is Fr of BW6-761: Fp<FrParams>,
// 14 limbs of 29 bits, R = 2^406.  Fq12 = Fq[w]/(w^12 + 5) as in circuit/tower.hpp: Frobenius is a scaling per coefficient, a line
// has the five coefficients w^0, w^1, w^3, w^7, w^9 (line_at), the final exponent is final_exponentiation's 3 (q^12 - 1) / r.
// The seam in the reference is nsnark::verify (libzecale/tests/circuits/dummy_application_test.cpp:32-44).
//
// THE CUT: a verification owns a GROUP of sixteen lanes.  Lanes 0 .. 11 hold one Fq12 coefficient each: coefficient k of a product is
// c_k = sum_i a_i b'_{k-i} (b'_j = b_j, or -5 b_{j+12} below zero): twelve products, six fp_mul2, the same work on every lane, operands
// read from LDS, one coefficient written back.  Lanes 12 .. 15 prepare the lines of the (up to four) pairs while the coefficient lanes
// square: l1, l7 = -lambda' xP (two products).  A fold of a line is five products per coefficient lane.  No point arithmetic runs in
// the Miller loop: the lines (lambda', b) of a G2 point depend on that point alone and come from g2_lines_lane (one lane per point,
// the affine chain of g2_precompute) or from the host (the key's -beta, -delta and the negated generator).
// Every body is a function of (lane index, operand arrays); none waits, spins or branches on data other than by selects - except
// the one-lane-per-point bodies (g2_lines_lane, nested_acc_lane, the curve checks, the checked route's nested_point_check and
// nested_inputs_check, the combined batches' nested_rho_scale and nested_g1_strip_sum at the end of this file), which run in kernels
// without barriers.
//
// LAZY BOUNDS ([k]: value < k p, limbs normalised).  fp29.cuh's contract: a b + c d < 2^10 R p; here R / p > 2^29, so any sum of
// products of operands [k1] x [k2] with sum k1 k2 < 2^39 is inside it and its result is < p (1 + 2^-10): written [1+].
//   Fq12 coefficients in memory are [8]; -5 x of a [8] value is [64]; line coefficients are [2].
#pragma once
#include <vector>

#include "../../include/zkhip.h"
#include "fp29.cuh"
#include "fp_inv.cuh"
#include "pairing.cuh"      // abi_geq_modulus, verify_refusal: shared with the BW6-761 checked route

namespace zkhip {

constexpr int NESTED_GROUP = 16;            // lanes per verification: twelve coefficient lanes + four line lanes
constexpr int NESTED_MAX_PAIRS = 4;
constexpr int NESTED_LINES = 69;            // 63 doublings + the 6 set bits of u below the top one
constexpr int NESTED_INPUT_BITS_DEV = 253;  // bits of an input the accumulator reads (circuit/sections.hpp NESTED_INPUT_BITS)
constexpr uint64_t NESTED_U = 0x8508c00000000001ull;

ZK_HD ZK_INL Fr fr_select(bool c, const Fr& a, const Fr& b) {
  Fr r;
#pragma unroll
  for (int i = 0; i < FrParams::NL; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
// x [k <= 2^9] -> [2]: one product by R mod p
ZK_HD ZK_INL Fr fr_red(const Fr& x) { return fp_mul(x, fp_one<FrParams>()); }
// -5 x for x [8]: 5 x is [40], 64 p - 5 x is [64]
ZK_HD ZK_INL Fr fr_times_m5(const Fr& x) {
  const Fr x4 = fp_dbl(fp_dbl(x));
  return fp_sub_k<FrParams, 64>(fp_zero<FrParams>(), fp_add(x4, x));
}
// b'_j of the reduction by w^12 = -5.   b [8] -> [64]
ZK_HD ZK_INL Fr fq12_wrapped(const Fr* b, int j) {
  const Fr x = b[j < 0 ? j + 12 : j];
  return fr_select(j < 0, fr_times_m5(x), x);
}

// coefficient k (0 .. 11) of a b.  a, b: twelve coefficients [8].  Result [8]:
//   each fp_mul2 sums two products [8] x [64]: 1024 p^2, result [1+]; six of them stay below [8].
ZK_HD ZK_INL Fr fq12_mul_coeff(int k, const Fr* a, const Fr* b) {
  Fr s = fp_zero<FrParams>();
#pragma unroll 1
  for (int t = 0; t < 6; t++) {
    const Fr r = fp_mul2(a[2 * t], fq12_wrapped(b, k - 2 * t), a[2 * t + 1], fq12_wrapped(b, k - 2 * t - 1));
    s = fp_add(s, r);                                   // [1+] each
  }
  return s;
}

// coefficient k of f (l0 + l1 w + l3 w^3 + l7 w^7 + l9 w^9).  f: twelve coefficients [8]; l = {l0, l1, l3, l7, l9}, each [8] at most.
// Result [8]: two fp_mul2 and one fp_mul of [8] x [64], each [1+].
ZK_HD ZK_INL Fr fq12_mul_line_coeff(int k, const Fr* f, const Fr* l) {
  const Fr l1 = fr_select(k < 1, fr_times_m5(l[1]), l[1]);
  const Fr l3 = fr_select(k < 3, fr_times_m5(l[2]), l[2]);
  const Fr l7 = fr_select(k < 7, fr_times_m5(l[3]), l[3]);
  const Fr l9 = fr_select(k < 9, fr_times_m5(l[4]), l[4]);
  const Fr t = fp_mul2(f[k], l[0], f[k < 1 ? k + 11 : k - 1], l1);
  const Fr u = fp_mul2(f[k < 3 ? k + 9 : k - 3], l3, f[k < 7 ? k + 5 : k - 7], l7);
  const Fr v = fp_mul(f[k < 9 ? k + 3 : k - 9], l9);
  return fp_add(fp_add(t, u), v);
}

// x -> x^(q^n) on coefficient k: a scaling by frob[(n k) mod 12] (tower.hpp Fq12Consts::frob, device form [2]).  x [8] -> [1+]
ZK_HD ZK_INL Fr fq12_frob_coeff(int k, int n, const Fr& x, const Fr* frob) { return fp_mul(x, frob[(n * k) % 12]); }

// One line of the Miller schedule as the host stores it (LineCoeffs: lambda', b in Fq2), four Fr in device form [2].
struct NestedLine { Fr lam0, lam1, b0, b1; };
// the five coefficients of line_at(lc, P): yP, -lambda'_0 xP, b_0, -lambda'_1 xP, b_1.  px, py [2].  Results [2] ([4] for the negated ones)
ZK_HD ZK_INL void nested_line_at(const NestedLine& lc, const Fr& px, const Fr& py, Fr* l) {
  const Fr npx = fp_sub<FrParams, 2>(fp_zero<FrParams>(), px);              // [2]
  l[0] = py;
  l[1] = fp_mul(lc.lam0, npx);
  l[2] = lc.b0;
  l[3] = fp_mul(lc.lam1, npx);
  l[4] = lc.b1;
}

// ---- the final exponentiation as a straight-line program over eight Fq12 registers: the kernel and the shim interpret the same list.
//   MUL d, a, b       d = a b                      (d differs from a and b)
//   FROB d, a, n      d = a^(q^n)                  (coefficient-wise; d may be a)
//   INVSCALE d, a, b  d = b / (a b)_0              (with b = prod_{i=1..11} a^(q^i) the product a b is the norm, in Fq: d = 1 / a)
struct Fq12Op { uint8_t op, d, a, b; };
enum { FQ12_OP_MUL = 0, FQ12_OP_FROB = 1, FQ12_OP_INVSCALE = 2 };
constexpr int FQ12_REGS = 8;

inline void fq12_prog_exp_by_u(std::vector<Fq12Op>& p, uint8_t d, uint8_t x, uint8_t t0, uint8_t t1) {    // d = x^u; d, x, t0, t1 distinct
  std::vector<Fq12Op> ops;
  uint8_t cur = x, nxt = t0;
  auto push = [&](uint8_t a, uint8_t b) { ops.push_back({FQ12_OP_MUL, nxt, a, b}); cur = nxt; nxt = cur == t0 ? t1 : t0; };
  for (int i = 62; i >= 0; i--) {
    push(cur, cur);
    if ((NESTED_U >> i) & 1) push(cur, x);
  }
  // the last operation writes d instead of a temporary (its operands are the other temporary and x)
  ops.back().d = d;
  p.insert(p.end(), ops.begin(), ops.end());
}
// register 0 holds f on entry and f^(3 (q^12 - 1) / r) on exit (bls12_377.hpp final_exponentiation, the same field elements)
inline std::vector<Fq12Op> fq12_final_exp_program() {
  std::vector<Fq12Op> p;
  auto mul = [&](uint8_t d, uint8_t a, uint8_t b) { p.push_back({FQ12_OP_MUL, d, a, b}); };
  auto frob = [&](uint8_t d, uint8_t a, uint8_t n) { p.push_back({FQ12_OP_FROB, d, a, n}); };
  // 1 / f through the norm to Fq: s11 = prod_{i=1..11} f^(q^i) by the chain 1, 2, 3, 4, 8, 11
  frob(1, 0, 1);                       // s1
  frob(2, 1, 1); mul(3, 1, 2);         // s2 = s1 s1^q
  frob(2, 1, 2); mul(4, 3, 2);         // s3 = s2 s1^(q^2)
  frob(2, 3, 2); mul(1, 3, 2);         // s4 = s2 s2^(q^2)
  frob(2, 1, 4); mul(3, 1, 2);         // s8 = s4 s4^(q^4)
  frob(2, 4, 8); mul(1, 3, 2);         // s11 = s8 s3^(q^8)
  p.push_back({FQ12_OP_INVSCALE, 2, 0, 1});      // 1 / f
  frob(3, 0, 6); mul(1, 3, 2);         // f1 = conj(f) / f
  frob(2, 1, 2); mul(0, 2, 1);         // f2 = f1^(q^2) f1
  fq12_prog_exp_by_u(p, 1, 0, 6, 7); frob(2, 0, 6); mul(3, 1, 2);      // t0 = f2^u conj(f2)
  fq12_prog_exp_by_u(p, 1, 3, 6, 7); frob(2, 3, 6); mul(4, 1, 2);      // t1 = t0^u conj(t0)
  fq12_prog_exp_by_u(p, 5, 4, 6, 7);                                   // t2 = t1^u
  fq12_prog_exp_by_u(p, 1, 5, 6, 7); frob(2, 4, 6); mul(3, 1, 2);      // t3 = t2^u conj(t1)
  fq12_prog_exp_by_u(p, 1, 3, 6, 7); mul(2, 0, 0); mul(6, 2, 0); mul(7, 1, 6);   // t4 = t3^u f2^3
  frob(1, 3, 1); mul(2, 7, 1);         // t4 t3^q
  frob(1, 5, 2); mul(6, 2, 1);         // ... t2^(q^2)
  frob(1, 4, 3); mul(0, 6, 1);         // ... t1^(q^3)
  return p;
}
// one operation on lane k (0 .. 11) of a group whose registers are reg[FQ12_REGS][12] ([8]).  The caller separates two operations by
// a barrier; an operation writes coefficient k of register d only.
ZK_HD ZK_INL void fq12_op_lane(const Fq12Op& o, int k, Fr (*reg)[12], const Fr* frob) {
  if (o.op == FQ12_OP_MUL) reg[o.d][k] = fq12_mul_coeff(k, reg[o.a], reg[o.b]);
  else if (o.op == FQ12_OP_FROB) reg[o.d][k] = fq12_frob_coeff(k, o.b, reg[o.a][k], frob);
  else {
    const Fr n = fr_red(fq12_mul_coeff(0, reg[o.a], reg[o.b]));             // [2]: the norm (every lane computes the same one)
    reg[o.d][k] = fp_mul(reg[o.b][k], fp_inv<FrParams>(n));                 // 0 -> 0: the product is then not one
  }
}

// ---- Fq2 = Fq[u]/(u^2 + 5) for the one-lane-per-point bodies
struct Fr2 { Fr a, b; };
// x y for x, y [16] at most.  Result [1+] each:  a c - 5 b d  and  a d + b c, one fp_mul2 each (16 x 16 + 16 x 128 = 2304 p^2)
ZK_HD ZK_INL Fr2 fr2_mul(const Fr2& x, const Fr2& y) {
  const Fr d4 = fp_dbl(fp_dbl(y.b));                                                        // [64]
  const Fr m5d = fp_sub_k<FrParams, 128>(fp_zero<FrParams>(), fp_add(d4, y.b));            // 128 p - 5 d: [128]  (5 d is [80])
  Fr2 r;
  r.a = fp_mul2(x.a, y.a, x.b, m5d);
  r.b = fp_mul2(x.a, y.b, x.b, y.a);
  return r;
}
// x - y + K p, y [K] at most
template <int K> ZK_HD ZK_INL Fr2 fr2_sub(const Fr2& x, const Fr2& y) { return Fr2{fp_sub_k<FrParams, K>(x.a, y.a), fp_sub_k<FrParams, K>(x.b, y.b)}; }
ZK_HD ZK_INL Fr2 fr2_add(const Fr2& x, const Fr2& y) { return Fr2{fp_add(x.a, y.a), fp_add(x.b, y.b)}; }
ZK_HD ZK_INL Fr2 fr2_red(const Fr2& x) { return Fr2{fr_red(x.a), fr_red(x.b)}; }
// 1 / d for d [16] at most; *zero is set when d = 0 (the result is then 0).  Result [1+]
ZK_HD ZK_INL Fr2 fr2_inv(const Fr2& d, bool* zero) {
  const Fr b5 = fp_add(fp_dbl(fp_dbl(d.b)), d.b);                                          // [80]
  const Fr n = fp_mul2(d.a, d.a, d.b, b5);                                                  // a^2 + 5 b^2: [1+]
  *zero = fp_is_zero_2p(n);
  const Fr ni = fp_inv<FrParams>(n);                                                        // [2]
  return Fr2{fp_mul(d.a, ni), fp_mul(fp_sub_k<FrParams, 16>(fp_zero<FrParams>(), d.b), ni)};
}

// y^2 = x^3 + 1 for x, y [2] (the nested G1).  One difference, reduced below 2 p before it is compared with zero.
ZK_HD ZK_INL bool nested_g1_on_curve(const Fr& x, const Fr& y) {
  const Fr lhs = fp_sqr(y);                                                                 // [2]
  const Fr rhs = fp_add(fp_mul(fp_sqr(x), x), fp_one<FrParams>());                          // [3]
  return fp_is_zero_2p(fr_red(fp_sub<FrParams, 4>(lhs, rhs)));
}
// y^2 = x^3 + 1/u over Fq2, 1/u = -(1/5) u.  fifth_neg: -1/5 in device form [2].  x, y [2]
ZK_HD ZK_INL bool nested_g2_on_curve(const Fr2& x, const Fr2& y, const Fr& fifth_neg) {
  const Fr2 yy = fr2_mul(y, y);
  Fr2 rhs = fr2_mul(fr2_mul(x, x), x);
  rhs.b = fp_add(rhs.b, fifth_neg);                                                         // [4]
  const Fr2 d = fr2_red(fr2_sub<4>(yy, rhs));
  return fp_is_zero_2p(d.a) && fp_is_zero_2p(d.b);
}

// step s (0 .. 68) of the schedule is an addition: bit s of the mask (a doubling per bit of u below the top one, an addition behind it where set)
struct NestedAddMask {
  uint64_t w[2];
  constexpr NestedAddMask() : w{0, 0} {
    int at = 0;
    for (int i = 62; i >= 0; i--) {
      at++;
      if ((NESTED_U >> i) & 1) { w[at >> 6] |= 1ull << (at & 63); at++; }
    }
  }
};
// The 69 lines of one G2 point Q (x, y [2], on its curve) in Miller-schedule order: the affine chain of g2_precompute, the same field
// elements (lambda', b = lambda' xT - yT).  One lane per point, one Fq2 inversion per step.  Returns false when a slope's denominator
// is zero (2 yT, or xQ - xT): the host's chord-and-tangent step is then not the group law and the caller does not decide the proof; the
// remaining lines are computed from the zero "inverse" as stand-ins.
ZK_HD ZK_INL bool g2_lines_lane(const Fr2& qx, const Fr2& qy, NestedLine* out) {
  constexpr NestedAddMask mask{};
  Fr2 tx = qx, ty = qy;                                                                     // [2] throughout
  bool fine = true;
#pragma unroll 1
  for (int s = 0; s < NESTED_LINES; s++) {
    const bool add = ((s < 64 ? mask.w[0] >> s : mask.w[1] >> (s - 64)) & 1) != 0;          // the same for every lane
    // tangent: 3 xT^2 / 2 yT;  chord: (yQ - yT) / (xQ - xT).  Both numerators and denominators are formed and one pair is selected.
    const Fr2 xx = fr2_mul(tx, tx);
    const Fr2 cn = fr2_sub<2>(qy, ty), cd = fr2_sub<2>(qx, tx);                             // [4]
    const Fr2 num{fr_select(add, cn.a, fp_add(fp_dbl(xx.a), xx.a)), fr_select(add, cn.b, fp_add(fp_dbl(xx.b), xx.b))};    // [6]
    const Fr2 den{fr_select(add, cd.a, fp_dbl(ty.a)), fr_select(add, cd.b, fp_dbl(ty.b))};                                // [4]
    bool zero;
    const Fr2 lam = fr2_mul(num, fr2_inv(den, &zero));                                      // [1+]
    fine = fine && !zero;
    const Fr2 b = fr2_red(fr2_sub<2>(fr2_mul(lam, tx), ty));                                // [2]
    out[s].lam0 = lam.a; out[s].lam1 = lam.b; out[s].b0 = b.a; out[s].b1 = b.b;
    const Fr2 ox{fr_select(add, qx.a, tx.a), fr_select(add, qx.b, tx.b)};
    const Fr2 x3 = fr2_red(fr2_sub<4>(fr2_mul(lam, lam), fr2_add(tx, ox)));                 // [2]
    const Fr2 y3 = fr2_red(fr2_sub<2>(fr2_mul(lam, fr2_sub<2>(tx, x3)), ty));               // [2]
    tx = x3; ty = y3;
  }
  return fine;
}

// ---- acc = ABC_0 + sum_i sum_j bit_j(x_i) 2^j ABC_i, the chain of input_accumulator in its order, as mixed additions in extended
// Jacobian coordinates (x = X / ZZ, y = Y / ZZZ; the nested curve has a = 0).  X [10], Y [4], ZZ, ZZZ [2].
struct NestedAcc { Fr X, Y, ZZ, ZZZ; };
// The step of acc and the chain point (x2, y2), both [2]: acc += (x2, y2) where `bit` is set.  Returns false and leaves acc alone
// when the two have the same x (acc = +-the chain point), WHATEVER the bit: the host forms acc + pw and the inverse of its denominator
// at every bit and selects afterwards, so its affine step is degenerate there at a clear bit too (acc = -pw fails its product check
// and the verdict is 0, not the group law's).  One product and the comparison at a clear bit, the addition only at a set one.
ZK_HD ZK_INL bool nested_acc_step(NestedAcc& a, const Fr& x2, const Fr& y2, bool bit) {
  const Fr U2 = fp_mul(x2, a.ZZ);                                           // [2]
  const Fr P = fr_red(fp_sub<FrParams, 16>(U2, a.X));                       // [2]   x2 ZZ - X          (X is [10] <= 16)
  if (fp_is_zero_2p(P)) return false;
  if (!bit) return true;
  const Fr S2 = fp_mul(y2, a.ZZZ);                                          // [2]
  const Fr Rr = fp_sub<FrParams, 4>(S2, a.Y);                               // [6]   y2 ZZZ - Y         (Y is [4])
  const Fr PP = fp_sqr(P), PPP = fp_mul(PP, P), Q = fp_mul(a.X, PP);        // [2]
  const Fr RR = fp_sqr(Rr);                                                 // [2]
  const Fr X3 = fp_sub_sub2<FrParams, 8>(RR, PPP, Q);                       // [10]  R^2 - P^3 - 2 Q    (P^3 + 2 Q is [6] <= 8)
  const Fr QX = fp_sub<FrParams, 16>(Q, X3);                                // [18]
  const Fr nY = fp_sub<FrParams, 4>(fp_zero<FrParams>(), a.Y);              // [4]
  a.Y = fp_mul2(Rr, QX, nY, PPP);                                           // [2]   6 x 18 + 4 x 2 = 116 p^2
  a.X = X3;
  a.ZZ = fp_mul(a.ZZ, PP);
  a.ZZZ = fp_mul(a.ZZZ, PPP);
  return true;
}
// abc0: ABC_0 (x, y); chain: n_inputs x 253 points (x, y) - 2^j ABC_i, device form [2]; inputs: n_inputs x 6 ABI limbs.
// out: the affine accumulator (x, y) [2].  Returns false when a step was degenerate (out is then a stand-in).
ZK_HD ZK_INL bool nested_acc_lane(const Fr* abc0, const Fr* chain, const uint64_t* inputs, size_t n_inputs, Fr* out) {
  NestedAcc acc{abc0[0], abc0[1], fp_one<FrParams>(), fp_one<FrParams>()};
  bool fine = true;
#pragma unroll 1
  for (size_t i = 0; i < n_inputs; i++) {
    uint32_t w[12];
    fp_abi_to_canonical_words<FrParams>(inputs + i * 6, w);
#pragma unroll 1
    for (int j = 0; j < NESTED_INPUT_BITS_DEV; j++) {
      const bool bit = w[0] & 1u;
#pragma unroll
      for (int t = 0; t < 12; t++) w[t] = (w[t] >> 1) | (t < 11 ? w[t + 1] << 31 : 0u);
      const Fr* pt = chain + (i * NESTED_INPUT_BITS_DEV + j) * 2;
      fine = nested_acc_step(acc, pt[0], pt[1], bit) && fine;
    }
  }
  const Fr zi = fp_inv<FrParams>(fr_red(fp_mul(acc.ZZ, acc.ZZZ)));
  out[0] = fp_mul(acc.X, fp_mul(zi, acc.ZZZ));
  out[1] = fp_mul(acc.Y, fp_mul(zi, acc.ZZ));
  return fine;
}

// ---- checked batches: encoding, curve membership and order of one nested point, one lane per point (k_nested_point_check).
// A G1 point is 12 ABI limbs (x | y), a G2 point 24 (x.c0 | x.c1 | y.c0 | y.c1).  The codes are zkhip.h's ZKHIP_VERIFY_*.  The nested
// format has NO point at infinity: the all-zero point fails its curve equation by itself (0 != 1, 0 != 1/u) and is OFF_CURVE - unlike
// pairing.cuh's point_check.  A lane stops at its first failure: an unreduced coordinate is never converted, a point off its curve
// never enters the group law.
ZK_HD ZK_INL bool nested_abi_geq_modulus(const uint64_t* x /* 6 raw ABI limbs */) { return abi_geq_modulus<FrParams>(x); }

// One set of names over Fr and Fr2, so that the XYZZ formulas below are written once (they never use b: one body serves G1 and G2).
// nf_mul(x, y): any x, y with [kx] x [ky], kx (ky + 128) < 2^39, and y [25] at most (fr2_mul forms 128 p - 5 y.b); result [1+].
ZK_HD ZK_INL Fr nf_mul(const Fr& x, const Fr& y) { return fp_mul(x, y); }
ZK_HD ZK_INL Fr2 nf_mul(const Fr2& x, const Fr2& y) { return fr2_mul(x, y); }
ZK_HD ZK_INL Fr nf_add(const Fr& x, const Fr& y) { return fp_add(x, y); }
ZK_HD ZK_INL Fr2 nf_add(const Fr2& x, const Fr2& y) { return fr2_add(x, y); }
template <int K> ZK_HD ZK_INL Fr nf_sub(const Fr& x, const Fr& y) { return fp_sub_k<FrParams, K>(x, y); }          // x - y + K p, y [K] at most
template <int K> ZK_HD ZK_INL Fr2 nf_sub(const Fr2& x, const Fr2& y) { return fr2_sub<K>(x, y); }
// exact for a product's result ([1+] < 2 p) and for an exact zero; never applied to anything else
ZK_HD ZK_INL bool nf_is_zero_2p(const Fr& x) { return fp_is_zero_2p(x); }
ZK_HD ZK_INL bool nf_is_zero_2p(const Fr2& x) { return fp_is_zero_2p(x.a) && fp_is_zero_2p(x.b); }
ZK_HD ZK_INL void nf_set(Fr& x, bool one) { x = one ? fp_one<FrParams>() : fp_zero<FrParams>(); }
ZK_HD ZK_INL void nf_set(Fr2& x, bool one) { x.a = one ? fp_one<FrParams>() : fp_zero<FrParams>(); x.b = fp_zero<FrParams>(); }

// Extended Jacobian coordinates (x = X / ZZ, y = Y / ZZZ), infinity <=> ZZ = 0.  Stored: X [10], Y [4]; ZZ, ZZZ products [1+] or exact zeros.
template <class E> struct NestedXYZZ { E X, Y, ZZ, ZZZ; };

// 2 P (dbl-2008-s-1, ec.cuh xyzz_dbl).  P.X [10], P.Y [4] -> X [6], Y [4].  A point of order 2 (Y = 0, so U = 0 mod p) gives V = W = 0
// and with them ZZ = ZZZ = 0: infinity.  Infinity stays infinity (ZZ3 = V ZZ).
template <class E> ZK_HD ZK_INL NestedXYZZ<E> nested_xyzz_dbl(const NestedXYZZ<E>& p) {
  NestedXYZZ<E> r;
  const E U = nf_add(p.Y, p.Y);                           // [8]
  const E V = nf_mul(U, U);                               // [1+]
  const E W = nf_mul(U, V);                               // [1+]
  const E S = nf_mul(p.X, V);                             // [1+]
  const E xx = nf_mul(p.X, p.X);                          // [1+]   ([10] x [10])
  const E M = nf_add(nf_add(xx, xx), xx);                 // [6]
  const E MM = nf_mul(M, M);                              // [1+]
  r.X = nf_sub<4>(MM, nf_add(S, S));                      // [6]    (2 S is [4])
  const E t = nf_sub<8>(S, r.X);                          // [10]   (X3 is [6] <= 8)
  const E Wy = nf_mul(W, p.Y);                            // [1+]
  r.Y = nf_sub<2>(nf_mul(M, t), Wy);                      // [4]
  r.ZZ = nf_mul(V, p.ZZ);                                 // [1+]
  r.ZZZ = nf_mul(W, p.ZZZ);                               // [1+]
  return r;
}
// 2 (x, y) for an affine point, x, y [2] (mdbl-2008-s-1): the doubling above with ZZ = ZZZ = 1
template <class E> ZK_HD ZK_INL NestedXYZZ<E> nested_xyzz_dbl_affine(const E& x, const E& y) {
  NestedXYZZ<E> p;
  p.X = x; p.Y = y; nf_set(p.ZZ, true); nf_set(p.ZZZ, true);
  return nested_xyzz_dbl(p);
}
// acc += (x2, y2), a finite affine point with coordinates [2] (madd-2008-s, ec.cuh xyzz_madd), COMPLETE - unlike nested_acc_step it
// takes its same-x branches: it opens from infinity, doubles when acc = (x2, y2) and goes to infinity when acc = -(x2, y2).  The two
// comparisons are made on PP and RR, results of products ([1+]; a square is zero exactly when its root is), never on P [18] or R [6].
template <class E> ZK_HD ZK_INL void nested_xyzz_madd(NestedXYZZ<E>& acc, const E& x2, const E& y2) {
  if (nf_is_zero_2p(acc.ZZ)) {
    acc.X = x2; acc.Y = y2; nf_set(acc.ZZ, true); nf_set(acc.ZZZ, true);
    return;
  }
  const E U2 = nf_mul(x2, acc.ZZ);                        // [1+]
  const E S2 = nf_mul(y2, acc.ZZZ);                       // [1+]
  const E P = nf_sub<16>(U2, acc.X);                      // [18]   (acc.X is [10] <= 16)
  const E R = nf_sub<4>(S2, acc.Y);                       // [6]    (acc.Y is [4])
  const E PP = nf_mul(P, P);                              // [1+]   ([18] x [18], second operand <= [25])
  const E RR = nf_mul(R, R);                              // [1+]
  if (nf_is_zero_2p(PP)) {                                // same x: acc = +-(x2, y2)
    if (nf_is_zero_2p(RR)) acc = nested_xyzz_dbl_affine(x2, y2);
    else { nf_set(acc.X, false); nf_set(acc.Y, false); nf_set(acc.ZZ, false); nf_set(acc.ZZZ, false); }
    return;
  }
  const E PPP = nf_mul(P, PP);                            // [1+]
  const E Q = nf_mul(acc.X, PP);                          // [1+]
  const E X3 = nf_sub<4>(nf_sub<4>(RR, PPP), nf_add(Q, Q));   // [2 + 4 + 4 = 10]
  const E t = nf_sub<16>(Q, X3);                          // [18]   (X3 is [10] <= 16)
  const E Y3a = nf_mul(t, R);                             // [1+]   (the [18] factor first: the second operand stays <= [25])
  const E Y3b = nf_mul(acc.Y, PPP);                       // [1+]
  acc.X = X3;
  acc.Y = nf_sub<2>(Y3a, Y3b);                            // [4]
  acc.ZZ = nf_mul(acc.ZZ, PP);                            // [1+]
  acc.ZZZ = nf_mul(acc.ZZZ, PPP);                         // [1+]
}

// bit i (0 .. 252) of r = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001, the order of the nested groups
ZK_HD ZK_INL bool nested_r_bit(int i) {
  const uint64_t w = i >= 192 ? 0x12ab655e9a2ca556ull : i >= 128 ? 0x60b44d1e5c37b001ull : i >= 64 ? 0x59aa76fed0000001ull : 0x0a11800000000001ull;
  return ((w >> (i & 63)) & 1) != 0;
}
constexpr int NESTED_R_BITS = 253;

// [r] (x, y) = O by double-and-add over r's 253 bits, most significant first: the definition.  x, y [2].  The bit is the same for every
// lane.  Every valid point ends with (r - 1) P + P = O in the same-x branch of the addition; a point of order 3 reaches that branch in
// the second iteration (2 P + P); a point of order 2 sends the doubling to ZZ = 0.
// Bounds: acc leaves the doubling with X [6], Y [4] and the addition with X [10], Y [4] ([2], [2] opened from the point): always
// within the X [10], Y [4] both formulas take.
template <class E> ZK_HD ZK_INL bool nested_point_has_order_r(const E& x, const E& y) {
  NestedXYZZ<E> acc;
  nf_set(acc.X, false); nf_set(acc.Y, false); nf_set(acc.ZZ, false); nf_set(acc.ZZZ, false);
#pragma unroll 1
  for (int i = NESTED_R_BITS - 1; i >= 0; i--) {
    acc = nested_xyzz_dbl(acc);                            // X [6], Y [4]
    if (nested_r_bit(i)) nested_xyzz_madd(acc, x, y);     // X [10], Y [4]
  }
  return nf_is_zero_2p(acc.ZZ);
}

// p: 12 ABI limbs (G1) or 24 (G2).  fifth_neg: -1/5 in device form [2] (read for G2 only).
ZK_HD ZK_INL int nested_point_check(const uint64_t* p, bool g2, const Fr& fifth_neg) {
  bool unreduced = nested_abi_geq_modulus(p) || nested_abi_geq_modulus(p + 6);
  if (g2) unreduced = unreduced || nested_abi_geq_modulus(p + 12) || nested_abi_geq_modulus(p + 18);
  if (unreduced) return ZKHIP_VERIFY_ENCODING;
  if (g2) {
    const Fr2 x{fp_from_abi<FrParams>(p), fp_from_abi<FrParams>(p + 6)}, y{fp_from_abi<FrParams>(p + 12), fp_from_abi<FrParams>(p + 18)};   // [2]
    if (!nested_g2_on_curve(x, y, fifth_neg)) return ZKHIP_VERIFY_OFF_CURVE;
    return nested_point_has_order_r(x, y) ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_NOT_ORDER_R;
  }
  const Fr x = fp_from_abi<FrParams>(p), y = fp_from_abi<FrParams>(p + 6);                 // [2]
  if (!nested_g1_on_curve(x, y)) return ZKHIP_VERIFY_OFF_CURVE;
  return nested_point_has_order_r(x, y) ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_NOT_ORDER_R;
}

// any of `n` inputs (6 raw ABI limbs each) is not an element of the nested scalar field: its limbs are >= the modulus of the field that
// carries it (Fr of BW6-761), or its canonical value is >= r (the accumulator reads 253 bits: x and x + r would share a verdict)
ZK_HD ZK_INL int nested_inputs_check(const uint64_t* inputs, size_t n) {
  constexpr uint32_t r32[12] = {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu, 0, 0, 0, 0};
  bool bad = false;
#pragma unroll 1
  for (size_t i = 0; i < n; i++) {
    if (nested_abi_geq_modulus(inputs + i * 6)) { bad = true; continue; }
    uint32_t w[12];
    fp_abi_to_canonical_words<FrParams>(inputs + i * 6, w);
    uint32_t borrow = 0;                                    // of w - r: clear when w >= r
#pragma unroll
    for (int t = 0; t < 12; t++) {
      const uint32_t a = w[t], m = r32[t], d = a - m;
      borrow = (uint32_t)(a < m) | (uint32_t)(d < borrow);
    }
    bad = bad || borrow == 0;
  }
  return bad ? ZKHIP_VERIFY_ENCODING : ZKHIP_VERIFY_ACCEPT;
}

// ---- combined batches: prod_i f(rho_i A_i, B_i) and S_C = sum_i rho_i C_i for ONE random-combination check of a whole batch
// (nested_combine_host.hpp states the equation).  k_nested_rho_scale runs nested_rho_scale on one lane per (proof, A or C), the existing
// Miller loop runs with one pair, and two reduction trees (k_nested_gt_product on sixteen-lane groups, k_nested_g1_sum on single lanes)
// take NESTED_STRIP values per strip and are relaunched on their partial results until one value is left.
//
// NESTED_STRIP = 8: a launch's dependent chain is seven Fq12 products (or seven point additions) - short against the 132 products
// of the Miller loop in front - and a chunk of 8,192 values is down to one in five launches; a strip of 4 would need seven launches for
// three dependent products each, a strip of 16 leaves 512 groups (64 workgroups) on the first and widest level, a quarter of the
// device's compute units, for a chain twice as long.  The integer rules are constexpr so that the host driver and the tests read them.
constexpr int NESTED_STRIP = 8;
constexpr int NESTED_RHO_BITS = 128;        // bit length of a combination scalar
// values one level of a reduction tree writes for the n it reads
constexpr size_t nested_strips(size_t n) { return (n + NESTED_STRIP - 1) / NESTED_STRIP; }
// launches of a reduction tree over n >= 1 values: level k reads n_k values (n_0 = n) and writes n_{k+1} = nested_strips(n_k); the last
// level is the one that is left with one strip
constexpr int nested_tree_levels(size_t n) {
  int levels = 1;
  for (; nested_strips(n) > 1; n = nested_strips(n)) levels++;
  return levels;
}

template <class E> ZK_HD ZK_INL NestedXYZZ<E> nested_xyzz_infinity() {
  NestedXYZZ<E> r;
  nf_set(r.X, false); nf_set(r.Y, false); nf_set(r.ZZ, false); nf_set(r.ZZZ, false);
  return r;
}

// rho (x, y) by double-and-add over the 128 bits of rho (two 64-bit words, little endian), most significant first, a fixed trip count;
// the scalar is shifted through its four 32-bit words, so no word is picked by a run-time index.  x, y [2], a point of the nested G1's
// curve (the formulas never use b).  A point of order 2 - (-1, 0) - goes to infinity in its first doubling behind a set bit and comes
// back with the next set bit: the result is infinity for an even rho and the point for an odd one.
// Bounds: those of nested_point_has_order_r - acc leaves the doubling with X [6], Y [4] and the addition with X [10], Y [4]: always
// within the X [10], Y [4] both formulas take.
ZK_HD ZK_INL NestedXYZZ<Fr> nested_rho_scale(const Fr& x, const Fr& y, const uint64_t* rho) {
  uint32_t w[4] = {(uint32_t)rho[0], (uint32_t)(rho[0] >> 32), (uint32_t)rho[1], (uint32_t)(rho[1] >> 32)};
  NestedXYZZ<Fr> acc = nested_xyzz_infinity<Fr>();
#pragma unroll 1
  for (int b = 0; b < NESTED_RHO_BITS; b++) {
    acc = nested_xyzz_dbl(acc);                              // X [6], Y [4]
    const bool bit = (w[3] >> 31) != 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) w[j] = (w[j] << 1) | (j ? w[j - 1] >> 31 : 0u);
    if (bit) nested_xyzz_madd(acc, x, y);                    // X [10], Y [4]
  }
  return acc;
}

// p (X [10], Y [4]; ZZ, ZZZ [1+], not infinity) -> affine (x, y) in device form [1+]: one inversion, as nested_acc_lane ends.
// ZZ ZZZ is reduced to [2] in front of the inversion; every other product has operands [10] x [1+] at most.
ZK_HD ZK_INL void nested_xyzz_to_affine(const NestedXYZZ<Fr>& p, Fr* out) {
  const Fr zi = fp_inv<FrParams>(fr_red(fp_mul(p.ZZ, p.ZZZ)));   // 1 / (ZZ ZZZ), [2]
  out[0] = fp_mul(p.X, fp_mul(zi, p.ZZZ));                       // X / ZZ
  out[1] = fp_mul(p.Y, fp_mul(zi, p.ZZ));                        // Y / ZZZ
}

// acc += q, both in XYZZ (add-2008-s), COMPLETE: infinity on either side is neutral, equal summands double, P and -P give infinity.
// acc and q: X [10], Y [4]; ZZ, ZZZ [1+] or exact zeros - what nested_rho_scale and this function leave.  The two comparisons are made
// on PP and RR, results of products ([1+]; a square is zero exactly when its root is), never on P or R [4].
template <class E> ZK_HD ZK_INL void nested_xyzz_add(NestedXYZZ<E>& acc, const NestedXYZZ<E>& q) {
  if (nf_is_zero_2p(q.ZZ)) return;
  if (nf_is_zero_2p(acc.ZZ)) { acc = q; return; }
  const E U1 = nf_mul(acc.X, q.ZZ);                       // [1+]   ([10] x [1+])
  const E U2 = nf_mul(q.X, acc.ZZ);                       // [1+]
  const E S1 = nf_mul(acc.Y, q.ZZZ);                      // [1+]   ([4] x [1+])
  const E S2 = nf_mul(q.Y, acc.ZZZ);                      // [1+]
  const E P = nf_sub<2>(U2, U1);                          // [4]    (U1 is [1+] <= 2)
  const E R = nf_sub<2>(S2, S1);                          // [4]
  const E PP = nf_mul(P, P);                              // [1+]
  const E RR = nf_mul(R, R);                              // [1+]
  if (nf_is_zero_2p(PP)) {                                // same x: q = +-acc
    if (nf_is_zero_2p(RR)) acc = nested_xyzz_dbl(acc);    // X [6], Y [4]
    else acc = nested_xyzz_infinity<E>();
    return;
  }
  const E PPP = nf_mul(P, PP);                            // [1+]
  const E Q = nf_mul(U1, PP);                             // [1+]
  const E X3 = nf_sub<4>(nf_sub<4>(RR, PPP), nf_add(Q, Q));   // [2 + 4 + 4 = 10]
  const E t = nf_sub<16>(Q, X3);                          // [18]   (X3 is [10] <= 16)
  const E Y3a = nf_mul(t, R);                             // [1+]   (the [18] factor first: the second operand stays <= [25])
  const E Y3b = nf_mul(S1, PPP);                          // [1+]
  acc.X = X3;
  acc.Y = nf_sub<2>(Y3a, Y3b);                            // [4]
  acc.ZZ = nf_mul(nf_mul(acc.ZZ, q.ZZ), PP);              // [1+]
  acc.ZZZ = nf_mul(nf_mul(acc.ZZZ, q.ZZZ), PPP);          // [1+]
}

// coefficient k of value i of the strip that starts at `first`: in[first + i] while that lies inside the `count` values and `skip`
// (null, or one byte per value: a proof that is left out) does not flag it, else of one - a select on the clamped index: nothing past
// the arrays is read.  in: twelve coefficients [8] per value; one is [1].
ZK_HD ZK_INL Fr nested_gt_strip_operand(int k, const Fr* in, size_t first, int i, size_t count, const uint8_t* skip) {
  const size_t idx = first + (size_t)i;
  const bool inside = idx < count;
  const size_t at = inside ? idx : count - 1;
  const bool take = inside && !(skip && skip[at]);
  return fr_select(take, in[at * 12 + k], k == 0 ? fp_one<FrParams>() : fp_zero<FrParams>());
}

// the sum of the strip that starts at `first` (< count), at most NESTED_STRIP values.  nested_xyzz_add keeps X [10], Y [4] for summands
// within the same bounds, which nested_rho_scale's results and earlier sums are.
ZK_HD ZK_INL NestedXYZZ<Fr> nested_g1_strip_sum(const NestedXYZZ<Fr>* in, size_t first, size_t count) {
  NestedXYZZ<Fr> acc = in[first];
#pragma unroll 1
  for (int i = 1; i < NESTED_STRIP; i++) {
    if (first + (size_t)i >= count) break;
    const NestedXYZZ<Fr> t = in[first + (size_t)i];
    nested_xyzz_add(acc, t);                              // X [10], Y [4]
  }
  return acc;
}

// p as affine ABI limbs (x | y), all zero for the point at infinity (the nested FORMAT has no such point: this is the sum tree's own
// result, read by the host finish alone).  fp_to_abi reduces the [1+] coordinates.
ZK_HD ZK_INL void nested_xyzz_to_affine_abi(const NestedXYZZ<Fr>& p, uint64_t* o) {
  if (nf_is_zero_2p(p.ZZ)) {
    for (int k = 0; k < 12; k++) o[k] = 0;
    return;
  }
  Fr xy[2];
  nested_xyzz_to_affine(p, xy);
  fp_to_abi<FrParams>(xy[0], o);
  fp_to_abi<FrParams>(xy[1], o + 6);
}

}  // namespace zkhip
