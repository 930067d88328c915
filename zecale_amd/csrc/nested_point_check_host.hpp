// The checks of the checked nested (BLS12-377) verifier ON THE HOST: the route the device's k_nested_point_check is pinned on.
// Encoding (raw limbs against the modulus of Fr of BW6-761 = Fq of BLS12-377), curve membership (G1: y^2 = x^3 + 1 over Fq, G2:
// y^2 = x^3 + 1/u over Fq2 = Fq[u]/(u^2 + 5)) and the order: [r] P = O by double-and-add in Jacobian coordinates with a complete mixed
// addition, over fully reduced 64-bit Montgomery limbs (host_field.hpp) - formulas, coordinates and limb form all differ from the
// device's lane body.  Host code only, no device and no library state, so that a CPU program can run it by itself (as nested_key.hpp).
// The nested format has no point at infinity: the all-zero point fails the curve equation and is ZKHIP_VERIFY_OFF_CURVE.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkhip.h"
#include "host_field.hpp"

namespace zkhip {
namespace nested_key {

using host::HFr;

// r of BLS12-377 (253 bits), little-endian words: the order of the nested groups and the modulus of the nested scalar field
constexpr uint64_t NESTED_R_ORDER64[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull, 0x12ab655e9a2ca556ull};
constexpr int NESTED_R_ORDER_BITS = 253;

// Fq2 = Fq[u]/(u^2 + 5) with the operations the generic point below uses
struct HFr2 {
  HFr a, b;
  static HFr2 zero() { return {HFr::zero(), HFr::zero()}; }
  static HFr2 one() { return {HFr::one(), HFr::zero()}; }
  bool is_zero() const { return a.is_zero() && b.is_zero(); }
  bool operator==(const HFr2& o) const { return a == o.a && b == o.b; }
  HFr2 operator+(const HFr2& o) const { return {a + o.a, b + o.b}; }
  HFr2 operator-(const HFr2& o) const { return {a - o.a, b - o.b}; }
  HFr2 operator*(const HFr2& o) const {
    const HFr bd = b * o.b, bd4 = bd.dbl().dbl();
    return {a * o.a - (bd4 + bd), a * o.b + b * o.a};
  }
  HFr2 sqr() const { return (*this) * (*this); }
  HFr2 dbl() const { return {a.dbl(), b.dbl()}; }
};

// Jacobian point over F on a curve with a = 0 (the formulas never use b).  Infinity: Z = 0.
template <class F>
struct NestedJac {
  F X, Y, Z;
  static NestedJac infinity() { return {F::zero(), F::one(), F::zero()}; }
  bool is_inf() const { return Z.is_zero(); }
  NestedJac dbl() const {                                  // dbl-2009-l; a point with Y = 0 goes to Z = 0
    if (is_inf()) return *this;
    const F A = X.sqr(), B = Y.sqr(), C = B.sqr();
    const F D = ((X + B).sqr() - A - C).dbl();
    const F E = A.dbl() + A, Fv = E.sqr();
    NestedJac r;
    r.X = Fv - D.dbl();
    r.Y = E * (D - r.X) - C.dbl().dbl().dbl();
    r.Z = (Y * Z).dbl();
    return r;
  }
  NestedJac add_affine(const F& x2, const F& y2) const {   // madd-2007-bl with its exceptional cases: complete
    if (is_inf()) return {x2, y2, F::one()};
    const F Z1Z1 = Z.sqr();
    const F U2 = x2 * Z1Z1, S2 = y2 * Z * Z1Z1;
    if (U2 == X) return S2 == Y ? dbl() : infinity();
    const F H = U2 - X, HH = H.sqr(), I = HH.dbl().dbl(), J = H * I, r = (S2 - Y).dbl(), V = X * I;
    NestedJac q;
    q.X = r.sqr() - J - V.dbl();
    q.Y = r * (V - q.X) - (Y * J).dbl();
    q.Z = (Z + H).sqr() - Z1Z1 - HH;
    return q;
  }
};

// [r] (x, y) = O, most significant bit first; any (x, y), on a curve y^2 = x^3 + b or not (the law of the curve through it is applied)
template <class F>
inline bool has_order_r_host(const F& x, const F& y) {
  NestedJac<F> acc = NestedJac<F>::infinity();
  for (int i = NESTED_R_ORDER_BITS - 1; i >= 0; i--) {
    acc = acc.dbl();
    if ((NESTED_R_ORDER64[i >> 6] >> (i & 63)) & 1) acc = acc.add_affine(x, y);
  }
  return acc.is_inf();
}

// one point: 12 ABI limbs (G1: x | y) or 24 (G2: x.c0 | x.c1 | y.c0 | y.c1) -> 0, ZKHIP_VERIFY_ENCODING, _OFF_CURVE or _NOT_ORDER_R
inline int point_check_host(const uint64_t* p, bool g2) {
  for (int k = 0; k < (g2 ? 4 : 2); k++)
    if (HFr::geq_p(p + k * 6)) return ZKHIP_VERIFY_ENCODING;
  if (g2) {
    const HFr2 x{HFr::from_limbs(p), HFr::from_limbs(p + 6)}, y{HFr::from_limbs(p + 12), HFr::from_limbs(p + 18)};
    const HFr2 b{HFr::zero(), HFr::from_u64(5).inv().neg()};                  // 1/u = -(1/5) u
    if (!(y.sqr() == x.sqr() * x + b)) return ZKHIP_VERIFY_OFF_CURVE;
    return has_order_r_host(x, y) ? 0 : ZKHIP_VERIFY_NOT_ORDER_R;
  }
  const HFr x = HFr::from_limbs(p), y = HFr::from_limbs(p + 6);
  if (!(y.sqr() == x.sqr() * x + HFr::one())) return ZKHIP_VERIFY_OFF_CURVE;
  return has_order_r_host(x, y) ? 0 : ZKHIP_VERIFY_NOT_ORDER_R;
}

// n inputs of 6 ABI limbs: ZKHIP_VERIFY_ENCODING when one is not an element of the nested scalar field - its limbs are >= the modulus
// of the field that carries it, or its value is >= r
inline int inputs_check_host(const uint64_t* inputs, size_t n) {
  for (size_t i = 0; i < n; i++) {
    if (HFr::geq_p(inputs + i * 6)) return ZKHIP_VERIFY_ENCODING;
    uint64_t c[6];
    HFr::from_limbs(inputs + i * 6).to_canonical(c);
    bool geq = c[4] != 0 || c[5] != 0;
    if (!geq) {
      geq = true;                                            // equal counts
      for (int k = 3; k >= 0; k--) {
        if (c[k] > NESTED_R_ORDER64[k]) break;
        if (c[k] < NESTED_R_ORDER64[k]) { geq = false; break; }
      }
    }
    if (geq) return ZKHIP_VERIFY_ENCODING;
  }
  return 0;
}

// the k + 4 points of a key (alpha | beta | delta | ABC_0 .. ABC_k) in their order: 0, or the first failing code with *element set
// (0 alpha, 1 beta, 2 delta, 3 + i ABC_i)
inline int key_check_host(const uint64_t* vk, size_t k, size_t* element) {
  for (size_t i = 0; i < k + 4; i++) {
    const uint64_t* p = i == 0 ? vk : i == 1 ? vk + 12 : i == 2 ? vk + 36 : vk + 60 + (i - 3) * 12;
    const int code = point_check_host(p, i == 1 || i == 2);
    if (code) { *element = i; return code; }
  }
  return 0;
}

}  // namespace nested_key
}  // namespace zkhip
