// G1's bucket accumulation on the 2-isogenous twisted Edwards curve (a = -1):  -x^2 + y^2 = 1 + d x^2 y^2  (DESIGN.md section 4).
//
// G1 of BW6-761 (y^2 = x^3 - 1) has all three 2-torsion points rational, so it is 2-isogenous to a twisted Edwards curve, and that
// curve scales to a = -1 (tools/gen_params.py: edwards_params).  chi maps G1 to it, psi maps back, psi(chi(P)) = 2P, both are group
// homomorphisms.  So for points P_i of G1 (order r; not merely odd order: 2 [1/2 mod r] P = P needs r P = O)
//     sum k_i P_i = psi( sum k_i chi(H_i) ),   H_i = [1/2 mod r] P_i.
// The Edwards table holds chi of the HALVED table points (msm.hip k_half_bases, msm_table_edw), so the digits are XYZZ's own.  The
// accumulation adds chi-images, the stitching and the bucket reduction add and double Edwards points (below), and psi is applied
// ONCE, on the host, to the one point per window that leaves the device (msm.hip edw_abi_to_jac).
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

// ---- the lockstep kernel's own forms (msm.hip k_accumulate_edw_lock): the table point gathered a whole multiplication ahead ----
// The sliced kernel's addition above gathers its point in three groups (ymx at step 0, ypx at step 1, t2d at step 2) and waits
// for each within the step that issued it.  Here the 72 packed words of the point are in registers BEFORE the addition starts, in
// the addition's own temporaries: T0 = ymx, T1 = ypx, T2 = t2d (words 0 .. 23 of each).  Each is consumed by the step that then
// writes it (0: A, 1: E and H, 2: F and G - the roles of edw_madd_lds_regy) and they are refilled - with the NEXT entry's point -
// before the last product, Z3 = F G, where T0, T1 are dead and T2, T3 have just been copied into the multiplier's operands: no
// register beyond edw_madd_lds_regy's, no second buffer, and the gather has that whole product to arrive.  A negated entry swaps
// the two source addresses (ymx <-> ypx) when the loads are issued; its t2d is not negated - F <-> G are selected instead, as above.
// The addresses are formed where the loads are issued (the entry word passes through an empty asm statement: hoisted out of the
// rolled loop, three 64-bit pointers would be live across every multiplication of the addition).
__device__ __forceinline__ void edw_pre_issue(Fq& T0, Fq& T1, Fq& T2, const EdwPacked* etab, uint32_t e) {
  asm volatile("" : "+v"(e));
  const char* p = reinterpret_cast<const char*>(etab + (e & 0x7fffffffu));         // (a table point is 18 x 16 bytes, 16-byte aligned)
  const uint32_t sw = (e >> 31) * 96u;                                              // negated: ypx first
  const zk_u32x4* a = reinterpret_cast<const zk_u32x4*>(p + sw);
  const zk_u32x4* b = reinterpret_cast<const zk_u32x4*>(p + (96u - sw));
  const zk_u32x4* c = reinterpret_cast<const zk_u32x4*>(p + 192);
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const zk_u32x4 u = a[j], v = b[j], w = c[j];
    T0.l[4 * j] = u.x; T0.l[4 * j + 1] = u.y; T0.l[4 * j + 2] = u.z; T0.l[4 * j + 3] = u.w;
    T1.l[4 * j] = v.x; T1.l[4 * j + 1] = v.y; T1.l[4 * j + 2] = v.z; T1.l[4 * j + 3] = v.w;
    T2.l[4 * j] = w.x; T2.l[4 * j + 1] = w.y; T2.l[4 * j + 2] = w.z; T2.l[4 * j + 3] = w.w;
  }
}
static_assert(offsetof(EdwPacked, ypx) == 96 && offsetof(EdwPacked, t2d) == 192, "edw_pre_issue addresses the coordinates by offset");

// acc += the point in T0, T1, T2 (edw_pre_issue: already swapped when negated; neg selects F <-> G), the accumulator as in
// edw_madd_lds_regy.  Step 0 loads and unpacks X once and forms both Y1 - X1 and Y1 + X1: the sum stays in ty ([4]; ty is dead
// until step 5 writes Y3).  The last product, Z3 = F G, stands BEHIND the rolled loop of the other six, with a multiplier body of
// its own: there the compiler sees that T0 .. T3 are dead, and the 72 words of the next point land in registers nobody holds
// (inside the rolled loop every temporary is live at every step as far as the allocator can tell: the same code as a seventh
// switch arm compiled to 256 VGPRs with 21 spilled; this form: 245, none - and only with the switches written as they are, six
// cases and an unreachable default: with step 5 as the default arm the allocator spills 28).  Before that product the gather of
// the next entry e1's point is issued when the lane has one, and behind it the load of the index after that one (entries[k2]
// into e2, when has_e2): every load of an addition is in flight under a whole product, and the one wait of the next addition's
// step 0 finds them all done.  Bounds as above.
__device__ __forceinline__ void edw_madd_lds_pre(uint32_t* xs, uint32_t* zs, uint32_t* ts, Fq& ty, Fq& T0, Fq& T1, Fq& T2, bool neg,
                                                 const EdwPacked* etab, uint32_t e1, bool has_e1, uint32_t& e2,
                                                 const uint32_t* entries, uint32_t k2, bool has_e2) {
  Fq T3;                  // (not initialised: written by step 2, read from step 3 on)
#pragma unroll 1
  for (int step = 0; step < 6; step++) {
    Fq a, b;
    switch (step) {
      case 0: {                                                                                           // A = (Y1 - X1)(y2 - x2)
        const Fq X = lds_ld_packed(xs);
        a = fp_sub<FqParams, 2>(ty, X); ty = fp_add(ty, X); b = fp_unpack32<FqParams>(T0.l);
        break;
      }
      case 1: a = ty; b = fp_unpack32<FqParams>(T1.l); break;                                             // B = (Y1 + X1)(y2 + x2)
      case 2: a = lds_ld(ts); b = fp_unpack32<FqParams>(T2.l); break;                                     // C = T1 2d x2 y2
      case 3: a = T1; b = fq_sel(neg, T3, T2); break;                                                     // X3 = E F
      case 4: a = T1; b = T0; break;                                                                      // T3 = E H
      case 5: a = fq_sel(neg, T2, T3); b = T0; break;                                                     // Y3 = G H
      default: __builtin_unreachable();
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
      default: __builtin_unreachable();
    }
  }
  const Fq F = T2, G = T3;
  if (has_e1) edw_pre_issue(T0, T1, T2, etab, e1);
  if (has_e2) {
    asm volatile("" : "+v"(k2));                                                                          // (as in edw_pre_issue)
    e2 = entries[k2];
  }
  lds_st(zs, fp_mul(F, G));                                                                               // Z3 = F G
}

// A bucket's first entry is not added to the identity: the accumulator is SET to the point in T0, T1, T2 (already swapped when
// negated), (X : Y : Z : T) = ((y + x) - (y - x) : (y + x) + (y - x) : 2 : (2 d x y) / d) = (2x : 2y : 2 : 2xy) - one product
// instead of seven.  The lanes of a lockstep wave open together (iteration 0 is wave-uniform), so no lane waits for another's six
// idle steps.  A negated entry negates t2d before the product (T = -2xy).  Bounds: the table's words are canonical [1], so
// X = ypx - ymx + p [2], Y = ypx + ymx [2], Z = 2 in Montgomery form [2], T a product [2]: what step 0 of the addition
// (fp_sub<2>) and the close of a one-entry bucket expect of stored coordinates.  The gather of e1's point is issued under the
// product.
__device__ __forceinline__ void edw_open_lds_pre(uint32_t* xs, uint32_t* zs, uint32_t* ts, Fq& ty, Fq& T0, Fq& T1, Fq& T2, bool neg,
                                                 const EdwPacked* etab, uint32_t e1, bool has_e1) {
  {
    const Fq ymx = fp_unpack32<FqParams>(T0.l), ypx = fp_unpack32<FqParams>(T1.l);
    lds_st_packed(xs, fp_sub_k<FqParams, 1>(ypx, ymx));
    ty = fp_add(ypx, ymx);
  }
  lds_st(zs, fp_dbl(fp_one<FqParams>()));
  Fq a = fp_unpack32<FqParams>(T2.l);
  if (neg) a = fp_sub_k<FqParams, 1>(fp_zero<FqParams>(), a);                                              // [2]
  if (has_e1) edw_pre_issue(T0, T1, T2, etab, e1);
  lds_st(ts, fp_mul(a, fp_const<FqParams>(FqParams::EDW_DINV)));
}

// ---- full additions and doublings: the stitching and the bucket reduction of an Edwards launch (msm.hip, point model EDW) ----
// Every array the reduction touches holds extended points in the X | Y | ZZ | ZZZ words (X | Y | Z | T).  A slot or item whose Z
// words are ZERO is EMPTY - nothing was ever accumulated there (k_slots_clear_zz, pt_set_inf) - and counts as the neutral element:
// every operation below that reads memory tests for it first and copies the other operand or returns, because an all-zero "point"
// would turn every sum it enters into zeros.  The true identity (0 : Y : Y : 0), which P + (-P) produces, is an ordinary point.
// Unified addition add-2008-hwcd-3 (k = 2d), nine products:
//     A = (Y1 - X1)(Y2 - X2), B = (Y1 + X1)(Y2 + X2), C = 2d T1 T2, D = 2 Z1 Z2, E = B - A, F = D - C, G = D + C, H = B + A,
//     X3 = E F, Y3 = G H, T3 = E H, Z3 = F G
// P + P and P + (-P) go through it (the trees do add equal points); like the mixed addition it is exact on the image of the
// order-r subgroup (d is a square).  9 x 1,458 = 13,122 v_mad_u64_u32 instead of the 18,981 of add_lds_regy / add_mem_s.
// Doubling dbl-2008-hwcd for a = -1, four squarings and four products:
//     A = X^2, B = Y^2, C = 2 Z^2, E = (X + Y)^2 - A - B, G = B - A, F = G - C, H = -A - B, then the same four output products.
// Bounds: stored coordinates are products [2]; sums and differences of two of them [4]; A, B, C [2]; D [4]; E, H [4]; F, G [6]
// (doubling: E [6], G [4], F [8], H [4]).

__device__ __forceinline__ bool edw_is_empty(const XyzzRef& r) { return fp_is_zero_2p(mem_ld(r, CZZ)); }

// acc += B: the accumulator on the CU as in edw_madd_lds_regy (X packed in LDS `xs`, Z in `zs`, T in `ts`, Y in registers), B a
// point in memory (not empty) - the counterpart of add_lds_regy.  One multiplier body in a rolled loop of nine steps.
__device__ __forceinline__ void edw_add_lds_regy(uint32_t* xs, uint32_t* zs, uint32_t* ts, Fq& ty, const XyzzRef& B) {
  Fq T0, T1, T2, T3;      // (not initialised: every one is written by the step before the first that reads it)
#pragma unroll 1
  for (int step = 0; step < 9; step++) {
    Fq a, b;
    switch (step) {
      case 0: a = fp_sub<FqParams, 2>(ty, lds_ld_packed(xs)); b = fp_sub<FqParams, 2>(mem_ld(B, CY), mem_ld(B, CX)); break;   // A
      case 1: a = fp_add(ty, lds_ld_packed(xs)); b = fp_add(mem_ld(B, CY), mem_ld(B, CX)); break;                               // B
      case 2: a = lds_ld(ts); b = mem_ld(B, CZZZ); break;                                                 // T1 T2
      case 3: a = T2; b = fp_const<FqParams>(FqParams::EDW_D2); break;                                    // C = 2d T1 T2
      case 4: a = lds_ld(zs); b = mem_ld(B, CZZ); break;                                                  // Z1 Z2
      case 5: a = T1; b = T2; break;                                                                      // X3 = E F
      case 6: a = T1; b = T0; break;                                                                      // T3 = E H
      case 7: a = T3; b = T0; break;                                                                      // Y3 = G H
      default: a = T2; b = T3; break;                                                                     // Z3 = F G
    }
    Fq r = fp_mul(a, b);
    switch (step) {
      case 0: T0 = r; break;                                                                              // A
      case 1: T1 = fp_sub<FqParams, 2>(r, T0); T0 = fp_add(r, T0); break;                                 // E = B - A, H = B + A [4]
      case 2: T2 = r; break;
      case 3: T2 = r; break;                                                                              // C
      case 4: {
        const Fq D = fp_dbl(r);                                                                           // [4]
        T3 = fp_add(D, T2);                                                                               // G = D + C [6]
        T2 = fp_sub<FqParams, 2>(D, T2);                                                                  // F = D - C [6]
        break;
      }
      case 5: lds_st_packed(xs, r); break;
      case 6: lds_st(ts, r); break;
      case 7: ty = r; break;
      default: lds_st(zs, r); break;
    }
  }
}

// A (memory) += B (memory), one lane; either may be empty; A is updated in place, B is not written - the counterpart of add_mem_s.
__device__ __forceinline__ void edw_add_mem(const XyzzRef& A, const XyzzRef& B) {
  if (edw_is_empty(B)) return;
  if (edw_is_empty(A)) { mem_copy(A, B); return; }
  Fq T0, T1, T2, T3;
#pragma unroll 1
  for (int step = 0; step < 9; step++) {
    Fq a, b;
    switch (step) {
      case 0: a = fp_sub<FqParams, 2>(mem_ld(A, CY), mem_ld(A, CX)); b = fp_sub<FqParams, 2>(mem_ld(B, CY), mem_ld(B, CX)); break;   // A
      case 1: a = fp_add(mem_ld(A, CY), mem_ld(A, CX)); b = fp_add(mem_ld(B, CY), mem_ld(B, CX)); break;                               // B
      case 2: a = mem_ld(A, CZZZ); b = mem_ld(B, CZZZ); break;                                            // T1 T2
      case 3: a = T2; b = fp_const<FqParams>(FqParams::EDW_D2); break;                                    // C
      case 4: a = mem_ld(A, CZZ); b = mem_ld(B, CZZ); break;                                              // Z1 Z2
      case 5: a = T1; b = T2; break;                                                                      // X3 = E F
      case 6: a = T1; b = T0; break;                                                                      // T3 = E H
      case 7: a = T3; b = T0; break;                                                                      // Y3 = G H
      default: a = T2; b = T3; break;                                                                     // Z3 = F G
    }
    Fq r = fp_mul(a, b);
    switch (step) {
      case 0: T0 = r; break;
      case 1: T1 = fp_sub<FqParams, 2>(r, T0); T0 = fp_add(r, T0); break;                                 // E, H [4]
      case 2: T2 = r; break;
      case 3: T2 = r; break;
      case 4: {
        const Fq D = fp_dbl(r);
        T3 = fp_add(D, T2);                                                                               // G [6]
        T2 = fp_sub<FqParams, 2>(D, T2);                                                                  // F [6]
        break;
      }
      case 5: mem_st(A, CX, r); break;                                                                    // (A is not read after step 4)
      case 6: mem_st(A, CZZZ, r); break;
      case 7: mem_st(A, CY, r); break;
      default: mem_st(A, CZZ, r); break;
    }
  }
}

// The last round of a quad addition or doubling: E, F, G, H are known to all four lanes; lane q computes coordinate q:
// q0 X3 = E F, q1 Y3 = G H, q2 Z3 = F G, q3 T3 = E H
#define ZK_EDW_QUAD_OUT_A(q, E, F, G, H) (((q) == 0 || (q) == 3) ? (E) : ((q) == 1) ? (G) : (F))
#define ZK_EDW_QUAD_OUT_B(q, E, F, G, H) (((q) == 0) ? (F) : ((q) == 2) ? (G) : (H))

// A += B by the four lanes of a quad (all four pass the same A and B; either may be empty) - the counterpart of add_mem_quad, a
// chain of three products instead of four.  One multiplier body in a rolled loop.
//   round 1: q0 A = (Y1 - X1)(Y2 - X2), q1 B = (Y1 + X1)(Y2 + X2), q2 T1 T2, q3 Z1 Z2
//   round 2: q2 C = 2d (T1 T2)                                      (the other lanes' products are not used)
//   round 3: the four output products, lane q stores coordinate q
__device__ __forceinline__ void edw_add_mem_quad(const XyzzRef& A, const XyzzRef& B, uint32_t q) {
  if (edw_is_empty(B)) return;
  if (edw_is_empty(A)) { mem_st_lane(A, q, mem_ld_lane(B, q)); return; }   // lane q copies coordinate q
  Fq E = fp_zero<FqParams>(), F = E, G = E, H = E, keep = E;
#pragma unroll 1
  for (int round = 0; round < 3; round++) {
    Fq a, b;
    if (round == 0) {
      const uint32_t c = (q < 2) ? CX : (q == 2) ? CZZZ : CZZ;         // q0, q1: X (Y joins below); q2: T; q3: Z
      const Fq u1 = mem_ld_lane(A, c), u2 = mem_ld_lane(B, c);
      const Fq y1 = mem_ld(A, CY), y2 = mem_ld(B, CY);
      a = (q == 0) ? fp_sub<FqParams, 2>(y1, u1) : (q == 1) ? fp_add(y1, u1) : u1;
      b = (q == 0) ? fp_sub<FqParams, 2>(y2, u2) : (q == 1) ? fp_add(y2, u2) : u2;
    } else if (round == 1) {
      a = keep; b = fp_const<FqParams>(FqParams::EDW_D2);
    } else {
      a = ZK_EDW_QUAD_OUT_A(q, E, F, G, H); b = ZK_EDW_QUAD_OUT_B(q, E, F, G, H);
    }
    const Fq r = fp_mul(a, b);
    if (round == 0) {
      const Fq pa = quad_bcast<0>(r), pb = quad_bcast<1>(r);
      E = fp_sub<FqParams, 2>(pb, pa);                                  // [4]
      H = fp_add(pb, pa);                                               // [4]
      G = fp_dbl(quad_bcast<3>(r));                                     // D = 2 Z1 Z2 [4], parked in G
      keep = r;                                                         // q2: T1 T2
    } else if (round == 1) {
      const Fq C = quad_bcast<2>(r);
      F = fp_sub<FqParams, 2>(G, C);                                    // D - C [6]
      G = fp_add(G, C);                                                 // D + C [6]
    } else {
      mem_st_lane(A, q, r);
    }
  }
}

// A = 2 A by a quad (A may be empty) - the counterpart of dbl_mem_quad, a chain of two products instead of three.
//   round 1: q0 X^2, q1 Y^2, q2 Z^2, q3 (X + Y)^2;   round 2: the four output products
__device__ __forceinline__ void edw_dbl_mem_quad(const XyzzRef& A, uint32_t q) {
  if (edw_is_empty(A)) return;
  Fq E = fp_zero<FqParams>(), F = E, G = E, H = E;
#pragma unroll 1
  for (int round = 0; round < 2; round++) {
    Fq a, b;
    if (round == 0) {
      a = mem_ld_lane(A, q == 3 ? (uint32_t)CX : q);
      if (q == 3) a = fp_add(a, mem_ld(A, CY));                         // X + Y [4]
      b = a;
    } else {
      a = ZK_EDW_QUAD_OUT_A(q, E, F, G, H); b = ZK_EDW_QUAD_OUT_B(q, E, F, G, H);
    }
    const Fq r = fp_mul(a, b);
    if (round == 0) {
      const Fq xx = quad_bcast<0>(r), yy = quad_bcast<1>(r), zz = quad_bcast<2>(r), xy = quad_bcast<3>(r);
      H = fp_add(xx, yy);                                               // A + B [4]
      E = fp_sub<FqParams, 4>(xy, H);                                   // (X + Y)^2 - A - B [6]
      G = fp_sub<FqParams, 2>(yy, xx);                                  // B - A [4]
      F = fp_sub<FqParams, 4>(G, fp_dbl(zz));                           // G - C [8]
      H = fp_sub<FqParams, 4>(fp_zero<FqParams>(), H);                  // -A - B [4]
    } else {
      mem_st_lane(A, q, r);
    }
  }
}

// chi for one affine point of G1 (device form, canonical), written out in precomputed form.  With X = x - 1:
//   x_e = t s y / (3 - X^2),  y_e = (y^2 - s X^2) / (y^2 + s X^2)        (one inversion of the product of the two denominators)
// Returns false when the point is not on G1's curve y^2 = x^3 - 1 (a G2 base set), hits a denominator that vanishes, maps to
// x_e = 0 (the points of order 2) or has an x - 1 that is not a square: the caller then keeps the base set on the XYZZ path.
// The square test is what refuses P + (1, 0): (1, 0) generates chi's kernel, so chi(P + (1, 0)) = chi(P) with no denominator
// vanishing, and nothing in the image tells the two apart.  x - 1 is the 2-descent coordinate at (1, 0): a square for every point
// of 2 E(Fq) - all of G1, whose order is odd - and for P + (1, 0) it is x(P) - 1 times (1 - w)(1 - w^2) = 3, w^3 = 1, which is
// not a square (s^2 = -3 and p = 3 mod 4).  Euler's criterion, X^((p-1)/2) = 1: 759 squarings and 344 products in one rolled loop.
// (Odd order is still not ESTABLISHED here - P + (w, 0) passes the square test and maps to a proper point of even order; order r
// is k_half_bases' check, 2 [1/2 mod r] P = P.)
__device__ __forceinline__ bool fq_is_square_nonzero(const Fq& X) {          // X [4]
  Fq acc = X;                                                                // bit 759 of (p - 1) / 2 = bit 760 of p
#pragma unroll 1
  for (int j = 758; j >= 0; j--) {
    acc = fp_sqr(acc);
    if ((FqParams::P[(j + 1) / 29] >> ((j + 1) % 29)) & 1u) acc = fp_mul(acc, X);      // (uniform: the bits of p)
  }
  const Fq c = fp_cond_sub_p(acc), one = fp_one<FqParams>();                 // canonical: 1, p - 1 or 0 (Montgomery form)
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 27; i++) d |= c.l[i] ^ one.l[i];
  return d == 0;
}
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
  const bool ok = on_curve && fq_is_square_nonzero(X) && !fp_is_zero_2p(den) && !fp_is_zero_2p(xe);
  fp_pack32<FqParams>(fp_canon(fp_sub<FqParams, 2>(ye, xe)), out->ymx);
  fp_pack32<FqParams>(fp_canon(fp_add(ye, xe)), out->ypx);
  fp_pack32<FqParams>(fp_canon(t2d), out->t2d);
  return ok;
}

}  // namespace zkhip
