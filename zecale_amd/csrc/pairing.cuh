// The BW6-761 reduced Tate pairing of pairing_host.hpp, cut into per-lane bodies for the device (pairing.hip) and for g++
// (tests/pairing_host_shim.cpp): t(P, Q) = f_{r,P}(psi(Q))^((q^6-1)/r), Fq6 = Fq[w]/(w^6 + 4), lines l0 + l3 w^3 + l4 w^4,
// vertical lines dropped (wsnarkT::verify of the snark policy class, reference libzecale/tests/aggregator/aggregator_dummy_test.cpp:61-62).
//
// THE CUT: one lane per Fq6 coefficient, six lanes of a group of eight, operands exchanged through LDS.
//   * An Fq6 product is 36 Fq products; coefficient k needs exactly six of them (c_k = sum_i a_i b'_{k-i}, b'_j = b_j for j >= 0 and
//     -4 b_{j+6} below), i.e. three fp_mul2 - the same work on every lane, no reduction tree, no partial sums to exchange: a lane
//     reads its twelve operands from LDS and writes one coefficient back.  The house DPP quad would spread ONE Fq product over four
//     lanes; here the six coefficients are the independent units the algebra already offers, and the multiplier's chain stays whole.
//   * The point steps of the (up to four) pairs are independent of each other and of the accumulator's squaring: pair p runs on lane p
//     of the group while all six coefficient lanes square; the group then folds the four lines into the accumulator one after the other
//     (a sparse line costs one fp_mul2 and one fp_mul per lane).
//   * Eight lanes per verification: G = 8 verifications per wave, and a 128-thread workgroup holds WG = 16.
// Every body below is a function of (lane index, operand arrays) with a fixed amount of work; none of them waits, spins or branches on data
// (the choice between b_j and -4 b_j, and "this pair has reached infinity", are selects).
//
// LAZY BOUNDS ([k]: value < k p, limbs normalised; fp29.cuh: a b + c d < 2^10 R p, R / p > 2^22, fp_sub<K>(a, b) needs b <= K p):
//   Fq6 coefficients in memory are [4]; -4 x of a [4] value is [16]; line coefficients l3, l4 are [2], l0 is [6]; Jacobian X [18], Y [4], Z [4].
#pragma once
#include "../../include/zkhip.h"
#include "ec.cuh"
#include "fp29.cuh"
#include "fp_inv.cuh"

namespace zkhip {

constexpr int PAIRING_GROUP = 8;        // lanes per verification (six coefficient lanes + two idle)
constexpr int PAIRING_MAX_PAIRS = 4;    // pairs per product (one point step per lane, lanes 0 .. 3)
constexpr int PAIRING_MILLER_STEPS = 376;   // bit length of r minus one
// combined batches: values one strip of the reduction trees multiplies (k_gt_product) or adds (k_g1_sum).  Eight keeps a launch's
// dependent chain at seven products, and a chunk of 16,384 values is down to one in five launches of microseconds each.
constexpr int PAIRING_STRIP = 8;
constexpr size_t PAIRING_CHUNK = 16384;     // verifications per launch sequence (bounds the work space)
constexpr size_t PAIRING_MAX_TERMS = (size_t)1 << 21;   // terms x_i ABC_i per launch of the per-proof route: 0.9 GB of work space
constexpr int PAIRING_RHO_BITS = 128;       // bit length of a combination scalar

// ---- the integer rules of the host driver (pairing.hip), here so that g++ reads them too (tests/pairing_combine_host_shim.cpp)
// proofs per chunk of the per-proof route: PAIRING_CHUNK while that keeps the chunk's terms within PAIRING_MAX_TERMS, never below one
constexpr size_t pairing_batch_chunk(size_t n_inputs) {
  if (n_inputs == 0 || PAIRING_CHUNK * n_inputs <= PAIRING_MAX_TERMS) return PAIRING_CHUNK;
  return PAIRING_MAX_TERMS / n_inputs ? PAIRING_MAX_TERMS / n_inputs : 1;
}
// points per launch of the key check (key_check.hip k_key_point_check, one lane per point, 5.1 k Fq products each): a launch at one
// wave per SIMD holds 65,536 lanes, so 2^17 points are two rounds of the whole chip and a 2^22-point query vector is 32 launches -
// no single launch is long on a device that others share.  `hook`: zkhip_internal_key_check_set_chunk, 0 = this rule.
constexpr size_t KEY_CHECK_CHUNK = (size_t)1 << 17;
constexpr size_t key_check_chunk(size_t hook) { return hook ? hook : KEY_CHECK_CHUNK; }
// values one level of a reduction tree writes for the n it reads
constexpr size_t pairing_strips(size_t n) { return (n + PAIRING_STRIP - 1) / PAIRING_STRIP; }
// launches of a reduction tree over n >= 1 values: level k reads n_k values (n_0 = n) and writes n_{k+1} = pairing_strips(n_k); the last
// level is the one that is left with one strip
constexpr int pairing_tree_levels(size_t n) {
  int levels = 1;
  for (; pairing_strips(n) > 1; n = pairing_strips(n)) levels++;
  return levels;
}
// located batches keep every level of a chunk's trees in ONE buffer, level after level: level 0 holds the n values the tree starts
// from, level k + 1 the pairing_strips of level k that launch k writes, the last level (number pairing_tree_levels(n)) the one root.
// Node s of level k covers the values [s 8^k, min((s + 1) 8^k, n)).
constexpr size_t pairing_level_size(size_t n, int k) {
  for (; k > 0; k--) n = pairing_strips(n);
  return n;
}
// where level k starts in that buffer: the sizes of the levels below it
constexpr size_t pairing_level_offset(size_t n, int k) {
  size_t off = 0;
  for (; k > 0; k--, n = pairing_strips(n)) off += n;
  return off;
}
// values in that buffer: every level, the root included
constexpr size_t pairing_tree_nodes(size_t n) { return pairing_level_offset(n, pairing_tree_levels(n)) + 1; }
// a call of the located route retains at most this many proofs' trees at a time (1.2 KB per proof: 1.3 GB); a larger batch is cut
// into consecutive located batches
constexpr size_t PAIRING_LOCATE_MAX = (size_t)1 << 20;

ZK_HD ZK_INL Fq fq_select(bool c, const Fq& a, const Fq& b) {
  Fq r;
#pragma unroll
  for (int i = 0; i < FqParams::NL; i++) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
// -4 x for x [4]: 4 x is [16], 16 p - 4 x is [16]
ZK_HD ZK_INL Fq fq_times_m4(const Fq& x) { return fp_sub<FqParams, 16>(fp_zero<FqParams>(), fp_dbl(fp_dbl(x))); }
// b'_j of the reduction by w^6 = -4: b_j for j >= 0, -4 b_{j+6} for j < 0.   b [4] -> [16]
ZK_HD ZK_INL Fq fq6_wrapped(const Fq* b, int j) {
  const Fq x = b[j < 0 ? j + 6 : j];
  return fq_select(j < 0, fq_times_m4(x), x);
}

// coefficient k (0 .. 5) of a b.  a, b: six coefficients [4].  Result [4]:
//   each fp_mul2 sums two products of [4] x [16]: < 128 p^2 < 2^10 R p, its result < 128 p^2 / R + p < p (1 + 2^-15); three of them < 4 p.
ZK_HD ZK_INL Fq fq6_mul_coeff(int k, const Fq* a, const Fq* b) {
  Fq s = fp_zero<FqParams>();
#pragma unroll 1
  for (int t = 0; t < 3; t++) {
    const Fq r = fp_mul2(a[2 * t], fq6_wrapped(b, k - 2 * t), a[2 * t + 1], fq6_wrapped(b, k - 2 * t - 1));
    s = fp_add(s, r);                                   // [1 + 2^-15] each: the sum stays below [4]
  }
  return s;
}

// coefficient k of f (l0 + l3 w^3 + l4 w^4).  f: six coefficients [4]; l = {l0 [6], l3 [2], l4 [2]}.  Result [4]:
//   fp_mul2: [4] x [6] + [4] x [16] < 88 p^2; fp_mul: [4] x [16]; each result < p (1 + 2^-15), their sum < [4].
ZK_HD ZK_INL Fq fq6_mul_line_coeff(int k, const Fq* f, const Fq* l) {
  const Fq l3 = fq_select(k < 3, fq_times_m4(l[1]), l[1]);
  const Fq l4 = fq_select(k < 4, fq_times_m4(l[2]), l[2]);
  const Fq t = fp_mul2(f[k], l[0], f[k < 3 ? k + 3 : k - 3], l3);
  const Fq u = fp_mul(f[k < 4 ? k + 2 : k - 4], l4);
  return fp_add(t, u);
}

struct MillerConst {     // one pair, device form, all [2]
  Fq px, py;             // P in G1, affine
  Fq xq4, yq4n;          // xQ / 4 and -yQ / 4: psi(Q) = (-xQ/4) w^4, (-yQ/4) w^3; the lines only ever use -(-xQ/4)
};
struct MillerPoint {     // running T = [k] P, Jacobian: X [18], Y [4], Z [4]
  Fq X, Y, Z;
};

ZK_HD ZK_INL void miller_identity_line(Fq* line) {
  line[0] = fp_one<FqParams>();
  line[1] = fp_zero<FqParams>();
  line[2] = fp_zero<FqParams>();
}

// line(T, T)(psi(Q)) scaled by 2 Y Z^3 (pairing_host.hpp miller_double), then T <- 2 T (dbl-2009-l with D = 4 X Y^2).
// `done` (T has reached infinity, or the pair has a member at infinity) turns the line into 1; T is then never used again.
ZK_HD ZK_INL void miller_double_step(MillerPoint& T, const MillerConst& c, bool done, Fq* line) {
  const Fq XX = fp_sqr(T.X), YY = fp_sqr(T.Y), ZZ = fp_sqr(T.Z);          // [2]   (X [18]: 324 p^2, far below the limit)
  const Fq t3 = fp_add(fp_dbl(XX), XX);                                   // [6]   3 X^2
  const Fq YZ = fp_mul(T.Y, T.Z);                                         // [2]
  const Fq A = fp_mul(YZ, ZZ);                                            // [2]   Y Z^3
  const Fq tZ = fp_mul(t3, ZZ);                                           // [2]   3 X^2 Z^2
  const Fq m = fp_mul(t3, T.X);                                           // [2]   3 X^3
  line[0] = fp_sub<FqParams, 4>(m, fp_dbl(YY));                           // [6]   3 X^3 - 2 Y^2          (2 Y^2 is [4])
  line[1] = fp_mul(fp_dbl(A), c.yq4n);                                    // [2]   (2 Y Z^3)(-yQ/4)
  line[2] = fp_mul(tZ, c.xq4);                                            // [2]   (-3 X^2 Z^2)(-xQ/4)
  if (done) miller_identity_line(line);
  const Fq S = fp_mul(T.X, YY);                                           // [2]   X Y^2
  const Fq F = fp_sqr(t3);                                                // [2]
  const Fq D = fp_dbl(fp_dbl(S));                                         // [8]   4 X Y^2
  const Fq X3 = fp_sub<FqParams, 16>(F, fp_dbl(D));                       // [18]  F - 2 D                (2 D is [16])
  const Fq DX = fp_sub_k<FqParams, 32>(D, X3);                            // [40]  D - X3                 (X3 is [18] <= 32)
  const Fq nY8 = fp_sub<FqParams, 16>(fp_zero<FqParams>(), fp_dbl(fp_dbl(fp_dbl(YY))));   // [16]  -8 Y^2  (8 Y^2 is [16])
  T.Y = fp_mul2(t3, DX, nY8, YY);                                         // [2]   3 X^2 (D - X3) - 8 Y^4:  6 x 40 + 16 x 2 = 272 p^2
  T.X = X3;
  T.Z = fp_dbl(YZ);                                                       // [4]
}

// line(T, P)(psi(Q)) scaled by D = Z (x2 Z^2 - X) (pairing_host.hpp miller_add), then T <- T + P (madd).
// Returns true when T = +-P (H = 0): the line is vertical, the step contributes 1 and the pair is done - for points of order r
// that is the last addition of the loop and nothing else.
ZK_HD ZK_INL bool miller_add_step(MillerPoint& T, const MillerConst& c, bool done, Fq* line) {
  const Fq ZZ = fp_sqr(T.Z);                                              // [2]
  const Fq U = fp_mul(c.px, ZZ);                                          // [2]
  const Fq ZZZ = fp_mul(ZZ, T.Z);                                         // [2]
  const Fq W = fp_mul(c.py, ZZZ);                                         // [2]
  const Fq H = fp_mul(fp_sub_k<FqParams, 32>(U, T.X), fp_one<FqParams>());  // [2]  x2 Z^2 - X ([34], X is [18] <= 32) brought back below 2 p
  const Fq N = fp_sub<FqParams, 4>(W, T.Y);                               // [6]   y2 Z^3 - Y              (Y is [4])
  done = done || fp_is_zero_2p(H);
  const Fq D = fp_mul(T.Z, H);                                            // [2]
  const Fq npy = fp_sub<FqParams, 2>(fp_zero<FqParams>(), c.py);          // [2]
  line[0] = fp_mul2(N, c.px, D, npy);                                     // [2]   N x2 - D y2:  6 x 2 + 2 x 2 = 16 p^2
  line[1] = fp_mul(D, c.yq4n);                                            // [2]   D (-yQ/4)
  line[2] = fp_mul(N, c.xq4);                                             // [2]   (-N)(-xQ/4)
  if (done) miller_identity_line(line);
  const Fq HH = fp_sqr(H);                                                // [2]
  const Fq HHH = fp_mul(HH, H);                                           // [2]
  const Fq V = fp_mul(T.X, HH);                                           // [2]
  const Fq NN = fp_sqr(N);                                                // [2]
  const Fq X3 = fp_sub_sub2<FqParams, 8>(NN, HHH, V);                     // [10]  N^2 - H^3 - 2 V         (H^3 + 2 V is [6] <= 8)
  const Fq VX = fp_sub<FqParams, 16>(V, X3);                              // [18]                          (X3 is [10] <= 16)
  const Fq nY = fp_sub<FqParams, 4>(fp_zero<FqParams>(), T.Y);            // [4]
  T.Y = fp_mul2(N, VX, nY, HHH);                                          // [2]   N (V - X3) - Y H^3:  6 x 18 + 4 x 2 = 116 p^2
  T.X = X3;
  T.Z = D;                                                                // [2]
  return done;
}

// ---- checked batches: encoding, curve membership and order of one point, one lane per point.
// A point is 24 ABI limbs (x | y); all zero is the point at infinity and passes (it is in the group).  The codes are zkhip.h's
// ZKHIP_VERIFY_*: 0 fine, ENCODING (a coordinate >= q), OFF_CURVE, NOT_ORDER_R.  A lane stops at its first failure: a point that is not
// reduced is never multiplied, a point off its curve never enters the group law.

// x (N64 raw ABI limbs) >= the modulus: the borrow of x - p, no branches
template <class PR>
ZK_HD ZK_INL bool abi_geq_modulus(const uint64_t* x) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < PR::N64; i++) {
    const uint64_t a = x[i], m = PR::P64[i], d = a - m;
    borrow = (uint64_t)(a < m) | (uint64_t)(d < borrow);
  }
  return borrow == 0;
}

// y^2 = x^3 + b (b = -1 on G1's curve, 4 on G2's) for x, y [2].  Both sides go into ONE difference that is reduced below 2 p before it
// is compared with zero (the idiom of ec_edw.cuh edw_from_affine): nothing lazily bounded is ever compared.
ZK_HD ZK_INL bool point_on_curve(const Fq& x, const Fq& y, bool g2) {
  const Fq one = fp_one<FqParams>(), zero = fp_zero<FqParams>();            // one is canonical: [1]
  const Fq yy = fp_sqr(y);                                                  // [2]
  const Fq xxx = fp_mul(fp_sqr(x), x);                                      // [2]
  const Fq lhs = fp_add(yy, fq_select(g2, zero, one));                      // [3]   y^2 (+ 1 on G1)
  const Fq rhs = fp_add(xxx, fq_select(g2, fp_dbl(fp_dbl(one)), zero));     // [6]   x^3 (+ 4 on G2)
  const Fq d = fp_sub<FqParams, 8>(lhs, rhs);                               // [11]  lhs - rhs + 8 p          (rhs is [6] <= 8)
  return fp_is_zero_2p(fp_cond_sub_kp<FqParams, 2>(fp_cond_sub_kp<FqParams, 4>(fp_cond_sub_kp<FqParams, 8>(d))));   // < 16 p -> < 2 p
}

// [r] P = O by double-and-add over r's 377 bits, most significant first; r_order: six 64-bit words, the same bit for every lane.
// x, y [2] (fp_from_abi of reduced limbs), P on its curve.  The formulas of ec.cuh never use b, so one path serves G1 and G2, and they
// are complete: xyzz_madd opens from infinity, takes the same-x branch (every valid point ends with (r - 1) P + P = -P + P = O there;
// a point of order 3 reaches it in the second iteration) and xyzz_dbl sends a point of order 2 (Y = 0) to ZZ = 0.
// Bounds: acc leaves xyzz_dbl with X [6], Y [4] and xyzz_madd with X [10], Y [4] (or [2], [2] opened from P; [6], [4] doubled from P):
// always within xyzz_dbl's and xyzz_madd's X [10], Y [4]; ZZ, ZZZ are products [2] or exact zeros.
ZK_HD ZK_INL bool point_has_order_r(const Fq& x, const Fq& y, const uint64_t* r_order) {
  XYZZ acc = xyzz_infinity();
#pragma unroll 1
  for (int i = PAIRING_MILLER_STEPS; i >= 0; i--) {
    acc = xyzz_dbl(acc);                                                    // X [6], Y [4]
    if ((r_order[i >> 6] >> (i & 63)) & 1) xyzz_madd(acc, x, y);            // X [10], Y [4]
  }
  return xyzz_is_inf(acc);
}

ZK_HD ZK_INL int point_check(const uint64_t* p /* 24 ABI limbs */, bool g2, const uint64_t* r_order) {
  if (abi_geq_modulus<FqParams>(p) || abi_geq_modulus<FqParams>(p + 12)) return ZKHIP_VERIFY_ENCODING;
  uint64_t nz = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) nz |= p[k];
  if (nz == 0) return ZKHIP_VERIFY_ACCEPT;                                  // the point at infinity
  const Fq x = fp_from_abi<FqParams>(p), y = fp_from_abi<FqParams>(p + 12); // [2]
  if (!point_on_curve(x, y, g2)) return ZKHIP_VERIFY_OFF_CURVE;
  return point_has_order_r(x, y, r_order) ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_NOT_ORDER_R;
}

// any of `n` scalars (6 raw ABI limbs each) >= r
ZK_HD ZK_INL int inputs_check(const uint64_t* inputs, size_t n) {
  bool bad = false;
  for (size_t i = 0; i < n; i++) bad = bad || abi_geq_modulus<FrParams>(inputs + i * 6);
  return bad ? ZKHIP_VERIFY_ENCODING : ZKHIP_VERIFY_ACCEPT;
}

// The codes of a proof's elements (A, B, C, the inputs as one) -> its status byte, 0 when nothing is refused: the first of ENCODING,
// OFF_CURVE, NOT_ORDER_R that any element has, and in the high nibble the elements that have exactly that code.
ZK_HD ZK_INL uint8_t verify_refusal(const uint8_t e[4]) {
  for (int code = ZKHIP_VERIFY_ENCODING; code <= ZKHIP_VERIFY_NOT_ORDER_R; code++) {
    int mask = 0;
    for (int k = 0; k < 4; k++) if (e[k] == code) mask |= ZKHIP_VERIFY_MASK_A << k;
    if (mask) return (uint8_t)(code | mask);
  }
  return 0;
}

// ---- combined batches: prod_i t(rho_i A_i, B_i) and S_C = sum_i rho_i C_i for one random-combination check of a whole batch.

// rho P by double-and-add over the 128 bits of rho (two 64-bit words, little endian), most significant first; the scalar is shifted
// through its four 32-bit words as in k_acc_terms, so no word is picked by a run-time index.  p: 24 reduced ABI limbs (x | y), all zero
// is the point at infinity and stays there.  The formulas never use the curve's b; the caller hands in points of G1.
// Bounds: those of point_has_order_r - acc leaves xyzz_dbl with X [6], Y [4] and xyzz_madd with X [10], Y [4], within what both accept.
ZK_HD ZK_INL XYZZ rho_scale(const uint64_t* p, const uint64_t* rho) {
  uint64_t nz = 0;
#pragma unroll
  for (int k = 0; k < 24; k++) nz |= p[k];
  const bool inf = nz == 0;
  const Fq x = fp_from_abi<FqParams>(p), y = fp_from_abi<FqParams>(p + 12);     // [2]
  uint32_t w[4] = {(uint32_t)rho[0], (uint32_t)(rho[0] >> 32), (uint32_t)rho[1], (uint32_t)(rho[1] >> 32)};
  XYZZ acc = xyzz_infinity();
#pragma unroll 1
  for (int b = 0; b < PAIRING_RHO_BITS; b++) {
    acc = xyzz_dbl(acc);                                                        // X [6], Y [4]
    const bool bit = (w[3] >> 31) != 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) w[j] = (w[j] << 1) | (j ? w[j - 1] >> 31 : 0u);
    if (bit && !inf) xyzz_madd(acc, x, y);                                      // X [10], Y [4]
  }
  return acc;
}

// p (X [10], Y [4], ZZ and ZZZ [2]) as affine ABI limbs (x | y), all zero for the point at infinity: one inversion, as k_acc_sum.
// Every operand of a product is [10] at most and every result [2], which fp_to_abi reduces.
ZK_HD ZK_INL void xyzz_to_affine_abi(const XYZZ& p, uint64_t* o) {
  if (xyzz_is_inf(p)) {
    for (int k = 0; k < 24; k++) o[k] = 0;
    return;
  }
  const Fq zi = fp_inv<FqParams>(fp_mul(p.ZZ, p.ZZZ));      // 1 / (ZZ ZZZ)
  const Fq x = fp_mul(p.X, fp_mul(zi, p.ZZZ));              // X / ZZ
  const Fq y = fp_mul(p.Y, fp_mul(zi, p.ZZ));               // Y / ZZZ
  fp_to_abi<FqParams>(x, o);
  fp_to_abi<FqParams>(y, o + 12);
}

// coefficient k of value i of the strip that starts at `first`: in[first + i] while that lies inside the `count` values, else of one
// (a select on the clamped index: nothing past the array is read).  in: six coefficients [4] per value; one is [1].
ZK_HD ZK_INL Fq gt_strip_operand(int k, const Fq* in, size_t first, int i, size_t count) {
  const size_t idx = first + (size_t)i;
  const bool inside = idx < count;
  const Fq v = in[(inside ? idx : count - 1) * 6 + k];
  return fq_select(inside, v, k == 0 ? fp_one<FqParams>() : fp_zero<FqParams>());
}

// the sum of the strip that starts at `first` (< count), at most PAIRING_STRIP values.  xyzz_add is complete - equal summands double,
// P and -P give infinity, infinity on either side is skipped - and keeps X [10], Y [4] (xyzz_dbl: X [6], Y [4]) for summands within
// the same bounds, which rho_scale's results and earlier sums are.
ZK_HD ZK_INL XYZZ g1_strip_sum(const XYZZ* in, size_t first, size_t count) {
  XYZZ acc = in[first];
#pragma unroll 1
  for (int i = 1; i < PAIRING_STRIP; i++) {
    if (first + (size_t)i >= count) break;
    const XYZZ t = in[first + (size_t)i];
    xyzz_add(acc, t);                                       // X [10], Y [4]
  }
  return acc;
}

}  // namespace zkhip
