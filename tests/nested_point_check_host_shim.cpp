// Host-side test shim: the lane bodies of the checked nested verifier (zecale_amd/csrc/pairing_bls.cuh nested_point_check,
// nested_inputs_check, nested_point_has_order_r - the code k_nested_point_check runs on every lane) compiled for the CPU by g++, so
// tests/test_nested_point_check_model.py can compare them with the host route and with Python big integers without a GPU.  Test
// infrastructure only.
#include "../zecale_amd/csrc/pairing_bls.cuh"
using namespace zkhip;

// -1/5 in device form, from the canonical integer 5 through the host inversion of fp_inv.cuh
static Fr fifth_neg_dev() {
  Fr five = fp_zero<FrParams>();
  const Fr one = fp_one<FrParams>();
  for (int i = 0; i < 5; i++) five = fp_add(five, one);                     // [5]
  return fr_red(fp_sub_k<FrParams, 2>(fp_zero<FrParams>(), fp_inv<FrParams>(fr_red(five))));   // 2 p - 1/5, brought back to [2]
}

extern "C" {
// p: 12 ABI limbs (x | y), or with g2 24 (x.c0 | x.c1 | y.c0 | y.c1); the code of zkhip.h (0, 2, 3, 4)
int nested_point_check_lane(const uint64_t* p, int g2) { return nested_point_check(p, g2 != 0, fifth_neg_dev()); }
// n inputs of 6 ABI limbs: 0 or 2
int nested_inputs_check_lane(const uint64_t* inputs, size_t n) { return nested_inputs_check(inputs, n); }
// four element codes (A, B, C, inputs) -> the refusal byte (the one definition both checked routes share)
int nested_refusal_byte(const uint8_t* e) { return verify_refusal(e); }
// the order body alone on ANY pair (x, y) of Fq2 elements (24 ABI limbs, reduced), on a curve or not: 1 when the walk over r's bits ends
// at infinity.  Reaches the Y = 0 doubling of the Fr2 body, for which the twist has no small-order point.
int nested_order_body_fr2(const uint64_t* p) {
  const Fr2 x{fp_from_abi<FrParams>(p), fp_from_abi<FrParams>(p + 6)}, y{fp_from_abi<FrParams>(p + 12), fp_from_abi<FrParams>(p + 18)};
  return nested_point_has_order_r(x, y) ? 1 : 0;
}
// the same over Fq (12 ABI limbs)
int nested_order_body_fr(const uint64_t* p) {
  return nested_point_has_order_r(fp_from_abi<FrParams>(p), fp_from_abi<FrParams>(p + 6)) ? 1 : 0;
}
}

#ifdef POINT_CHECK_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DPOINT_CHECK_SHIM_MAIN): the points come on the command
// line as hexadecimal limbs, one argument per point (12 x 16 digits: a G1 point; 24 x 16: a G2 point); prints one code per point.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    const size_t len = strlen(argv[a]);
    if (len != 12 * 16 && len != 24 * 16) return 2;
    uint64_t p[24];
    const size_t n = len / 16;
    for (size_t i = 0; i < n; i++) {
      char w[17];
      memcpy(w, argv[a] + i * 16, 16);
      w[16] = 0;
      p[i] = strtoull(w, nullptr, 16);
    }
    printf("%d%c", nested_point_check_lane(p, n == 24), a + 1 == argc ? '\n' : ' ');
  }
  return 0;
}
#endif
