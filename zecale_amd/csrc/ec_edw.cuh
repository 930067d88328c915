// G1's bucket accumulation on the 2-isogenous twisted Edwards curve (a = -1):  -x^2 + y^2 = 1 + d x^2 y^2  (DESIGN.md section 4).
//
// G1 of BW6-761 (y^2 = x^3 - 1) has all three 2-torsion points rational, so it is 2-isogenous to a twisted Edwards curve, and that
// curve scales to a = -1 (tools/gen_params.py: edwards_params).  chi maps G1 to it, psi maps back, psi(chi(P)) = 2P, both are group
// homomorphisms.  So for points P_i of G1 (order r; not merely odd order: 2 [1/2 mod r] P = P needs r P = O)
//     sum k_i P_i = psi( sum k_i chi(H_i) ),   H_i = [1/2 mod r] P_i,
// and psi of a bucket is a bucket of the original sum.  The Edwards table holds chi of the HALVED table points (msm.hip k_half_bases,
// msm_table_edw), so the digits are XYZZ's own; the accumulation adds chi-images, every slot is mapped back by psi right after it
// (k_slots_edw_to_xyzz), and everything downstream - stitching, reduction, the host - stays XYZZ, bit for bit the same code.
//
// The accumulator is in extended coordinates (X : Y : Z : T), x = X/Z, y = Y/Z, T = XY/Z; the identity is (0 : 1 : 1 : 0).
// Table points are stored precomputed, (y - x, y + x, 2 d x y), so a mixed addition is SEVEN products and no squaring (Hisil, Wong,
// Carter, Dawson 2008, "madd-2008-hwcd-3" with k = 2d as in ref10's ge_madd):
//     A = (Y1 - X1)(y2 - x2), B = (Y1 + X1)(y2 + x2), C = T1 (2d x2 y2), D = 2 Z1, E = B - A, F = D - C, G = D + C, H = B + A,
//     X3 = E F, Y3 = G H, T3 = E H, Z3 = F G
// 7 x 1,458 = 10,206 v_mad_u64_u32 per addition instead of the 13,149 of a mixed addition into XYZZ.  The formula is unified (P + P
// and P + (-P) go through it) and fails only when the sum is one of the curve's points at infinity - points of order 2 or 4, which
// the image of the odd-order subgroup never reaches: no branch, no same-x path.  -(x, y) = (-x, y): negating a table point swaps
// y - x and y + x and negates 2dxy, which is F <-> G.
#pragma once
#include "ec_mem.cuh"
#include "fp_inv.cuh"

namespace zkhip {

// a table point in precomputed form: three canonical coordinates, 24 packed words each (288 bytes).  Points at infinity are never
// read (k_digit_pass drops their entries); their entries hold zeros.
struct EdwPacked {
  uint32_t ymx[24];   // y - x
  uint32_t ypx[24];   // y + x
  uint32_t t2d[24];   // 2 d x y
};
static_assert(sizeof(EdwPacked) == 288, "precomputed Edwards point is 288 bytes");

__device__ __forceinline__ Fq edw_ld(const uint32_t* w) {
  uint32_t v[24];
#pragma unroll
  for (int i = 0; i < 24; i++) v[i] = w[i];
  return fp_unpack32<FqParams>(v);
}

// acc += p (precomputed table point; negated when neg), the accumulator on the CU as in madd_lds_regy: X (packed) in LDS `xs`, Z in
// LDS `zs`, T in LDS `ts`, Y in registers `ty`.  One multiplier body in a rolled loop of seven steps; E, F, G, H and Y are the five
// field elements that live at most.  Bounds: every stored coordinate is a product [2]; A, B, C [2]; E, H [4]; F, G [6].
__device__ __forceinline__ void edw_madd_lds_regy(uint32_t* xs, uint32_t* zs, uint32_t* ts, Fq& ty, const EdwPacked* p, bool neg) {
  Fq T0, T1, T2, T3;      // (not initialised: every one is written by the step before the first that reads it)
#pragma unroll 1
  for (int step = 0; step < 7; step++) {
    Fq a, b;
    switch (step) {
      case 0: a = fp_sub<FqParams, 2>(ty, lds_ld_packed(xs)); b = edw_ld(neg ? p->ypx : p->ymx); break;   // A = (Y1 - X1)(y2 - x2)
      case 1: a = fp_add(ty, lds_ld_packed(xs)); b = edw_ld(neg ? p->ymx : p->ypx); break;               // B = (Y1 + X1)(y2 + x2)
      case 2: a = lds_ld(ts); b = edw_ld(p->t2d); break;                                                  // C = T1 2d x2 y2
      case 3: a = T1; b = fq_sel(neg, T3, T2); break;                                                     // X3 = E F
      case 4: a = T1; b = T0; break;                                                                      // T3 = E H
      case 5: a = fq_sel(neg, T2, T3); b = T0; break;                                                     // Y3 = G H
      default: a = T2; b = T3; break;                                                                     // Z3 = F G
    }
    Fq r = fp_mul(a, b);
    switch (step) {
      case 0: T0 = r; break;                                                                              // A
      case 1: T1 = fp_sub<FqParams, 2>(r, T0); T0 = fp_add(r, T0); break;                                 // E = B - A, H = B + A [4]
      case 2: {
        const Fq D = fp_dbl(lds_ld(zs));                                                                  // [4]
        T2 = fp_sub<FqParams, 2>(D, r);                                                                   // D - C [6]: F (-p: G)
        T3 = fp_add(D, r);                                                                                // D + C [6]: G (-p: F)
        break;
      }
      case 3: lds_st_packed(xs, r); break;
      case 4: lds_st(ts, r); break;
      case 5: ty = r; break;
      default: lds_st(zs, r); break;
    }
  }
}

// The identity (0 : 1 : 1 : 0): where every run of the Edwards accumulation starts (its first entry is an ordinary addition, so the
// lanes of a wave that open a run do the same work as the others).
__device__ __forceinline__ void edw_set_identity(uint32_t* xs, uint32_t* zs, uint32_t* ts, Fq& ty) {
#pragma unroll
  for (int i = 0; i < 24; i++) xs[i * ZK_LDS_STRIDE] = 0u;
  lds_st(zs, fp_one<FqParams>());
  lds_st(ts, fp_zero<FqParams>());
  ty = fp_one<FqParams>();
}

// psi, in place: a slot that holds an Edwards point (X : Y : Z : T) in its X | Y | ZZ | ZZZ words receives the XYZZ point psi(P).
// With W = Z^2 - Y^2 and lambda = X W:  ZZ = lambda^2, ZZZ = lambda^3, X' = (X^2 + c1 Z^2) W^2, Y' = c2 Y Z^2 ZZ
// (x = 1 + c1 Z^2 / X^2, y = c2 Y Z^2 / (X W): tools/gen_params.py edwards_params).  The identity (X = 0) gives ZZ = 0: XYZZ's
// infinity.  Twelve products in a rolled loop (one multiplier body), four temporaries; every output [2].
__device__ __forceinline__ void edw_to_xyzz_mem(const XyzzRef& r) {
  Fq T0, T1, T2, T3;
#pragma unroll 1
  for (int step = 0; step < 12; step++) {
    Fq a, b;
    switch (step) {
      case 0: a = mem_ld(r, CX); b = a; break;                                   // X^2
      case 1: a = mem_ld(r, CZZ); b = a; break;                                  // Z^2
      case 2: a = mem_ld(r, CY); b = a; break;                                   // Y^2
      case 3: a = mem_ld(r, CX); b = T2; break;                                  // lambda = X W
      case 4: a = T2; b = T2; break;                                             // W^2
      case 5: a = T1; b = fp_const<FqParams>(FqParams::EDW_C1); break;           // c1 Z^2
      case 6: a = T0; b = T2; break;                                             // X' = (X^2 + c1 Z^2) W^2
      case 7: a = T3; b = T3; break;                                             // ZZ = lambda^2
      case 8: a = T0; b = T3; break;                                             // ZZZ = ZZ lambda
      case 9: a = mem_ld(r, CY); b = T1; break;                                  // Y Z^2
      case 10: a = T3; b = T0; break;                                            // Y Z^2 ZZ
      default: a = T3; b = fp_const<FqParams>(FqParams::EDW_C2); break;         // Y' = c2 Y Z^2 ZZ
    }
    Fq v = fp_mul(a, b);
    switch (step) {
      case 0: T0 = v; break;
      case 1: T1 = v; break;
      case 2: T2 = fp_sub<FqParams, 2>(T1, v); break;                            // W [4]
      case 3: T3 = v; break;
      case 4: T2 = v; break;
      case 5: T0 = fp_add(T0, v); break;                                         // X^2 + c1 Z^2 [4]
      case 6: mem_st(r, CX, v); break;                                           // (X is not read after step 3)
      case 7: T0 = v; mem_st(r, CZZ, v); break;                                  // (Z: not read after step 1)
      case 8: mem_st(r, CZZZ, v); break;                                         // (T is never read)
      case 9: T3 = v; break;
      case 10: T3 = v; break;
      default: mem_st(r, CY, v); break;
    }
  }
}

// chi for one affine point of G1 (device form, canonical), written out in precomputed form.  With X = x - 1:
//   x_e = t s y / (3 - X^2),  y_e = (y^2 - s X^2) / (y^2 + s X^2)        (one inversion of the product of the two denominators)
// Returns false when the point is not on G1's curve y^2 = x^3 - 1 (a G2 base set) or hits a denominator that vanishes (a point of
// even order): the caller then keeps the base set on the XYZZ path.
__device__ __forceinline__ bool edw_from_affine(const Fq& x, const Fq& y, EdwPacked* out) {
  const Fq one = fp_one<FqParams>();
  const Fq yy = fp_mul(y, y);
  const Fq xxx = fp_mul(fp_mul(x, x), x);
  const bool on_curve = fp_is_zero_2p(fp_cond_sub_kp<FqParams, 2>(fp_cond_sub_kp<FqParams, 4>(
                            fp_sub<FqParams, 4>(fp_add(yy, one), xxx))));                                  // y^2 + 1 - x^3 [7] -> [2]
  const Fq X = fp_sub<FqParams, 2>(x, one);                                                                // [3]
  const Fq XX = fp_mul(X, X);
  const Fq sXX = fp_mul(XX, fp_const<FqParams>(FqParams::EDW_S));
  const Fq D1 = fp_sub<FqParams, 2>(fp_const<FqParams>(FqParams::EDW_THREE), XX);                           // [3]
  const Fq D2 = fp_add(yy, sXX);                                                                           // [4]
  const Fq N2 = fp_sub<FqParams, 2>(yy, sXX);                                                              // [4]
  const Fq den = fp_mul(D1, D2);
  const Fq inv = fp_inv<FqParams>(den);
  const Fq xe = fp_mul(fp_mul(fp_mul(y, fp_const<FqParams>(FqParams::EDW_TS)), D2), inv);
  const Fq ye = fp_mul(fp_mul(N2, D1), inv);
  const Fq t2d = fp_mul(fp_mul(xe, ye), fp_const<FqParams>(FqParams::EDW_D2));
  const bool ok = on_curve && !fp_is_zero_2p(den) && !fp_is_zero_2p(xe);
  fp_pack32<FqParams>(fp_canon(fp_sub<FqParams, 2>(ye, xe)), out->ymx);
  fp_pack32<FqParams>(fp_canon(fp_add(ye, xe)), out->ypx);
  fp_pack32<FqParams>(fp_canon(t2d), out->t2d);
  return ok;
}

}  // namespace zkhip
