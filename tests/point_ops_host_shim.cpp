// Host-side test shim: the five register forms of the product's ec.cuh (ZK_HD, compiled for the CPU by g++) on raw limbs, in the row
// layout of the device hook zkhip_internal_point_ops_selftest (224 words in, 217 out), so that one case list and one checker
// (tests/point_ops_cases.py) serve both builds.  Test infrastructure only.
#include <cstddef>
#include <cstdint>

#include "../zecale_amd/csrc/ec.cuh"
using namespace zkhip;

static Fq ld(const uint32_t* w) {
  Fq v;
  for (int k = 0; k < 27; k++) v.l[k] = w[k];
  return v;
}
static XYZZ ld_xyzz(const uint32_t* w) {
  XYZZ p;
  p.X = ld(w); p.Y = ld(w + 27); p.ZZ = ld(w + 54); p.ZZZ = ld(w + 81);
  return p;
}

extern "C" int point_op(int op, const uint32_t* in, uint32_t* out) {
  XYZZ a = ld_xyzz(in);
  const XYZZ b = ld_xyzz(in + 108);               // (the affine operand of ops 0 and 2 is its first two coordinates)
  switch (op) {
    case 0: a = xyzz_dbl_affine(b.X, b.Y); break;
    case 1: a = xyzz_dbl(a); break;
    case 2: xyzz_madd(a, b.X, b.Y); break;
    case 3: xyzz_add(a, b); break;
    case 4: xyzz_neg(a); break;
    default: return -1;
  }
  const Fq* f[4] = {&a.X, &a.Y, &a.ZZ, &a.ZZZ};
  const Fq* g[4] = {&b.X, &b.Y, &b.ZZ, &b.ZZZ};
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < 27; k++) { out[c * 27 + k] = f[c]->l[k]; out[109 + c * 27 + k] = g[c]->l[k]; }
  out[108] = xyzz_is_inf(a) ? 1u : 0u;            // void functions: does the result test as infinity?
  return 0;
}
