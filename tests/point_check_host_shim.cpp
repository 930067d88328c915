// Host-side test shim: the lane body of the checked verifier's point check (zecale_amd/csrc/pairing.cuh point_check, the code
// k_point_check runs on every lane) compiled for the CPU by g++, so tests/test_point_check_model.py can compare it with the host route
// and with Python big integers without a GPU.  Test infrastructure only.
#include "../zecale_amd/csrc/pairing.cuh"
using namespace zkhip;

extern "C" {
// p: 24 ABI limbs (x | y); the code of zkhip.h (0, 2, 3, 4)
int point_check_lane(const uint64_t* p, int g2) { return point_check(p, g2 != 0, FqParams::R_ORDER64); }
// n scalars of 6 ABI limbs: 0 or 2
int inputs_check_lane(const uint64_t* inputs, size_t n) { return inputs_check(inputs, n); }
// four element codes (A, B, C, inputs) -> the refusal byte
int refusal_byte(const uint8_t* e) { return verify_refusal(e); }
}

#ifdef POINT_CHECK_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DPOINT_CHECK_SHIM_MAIN): both generators (full walk over r's
// bits, ending in the same-x branch), infinity, (1, 0) of order 2 and a coordinate equal to q
#include <stdio.h>
#include <string.h>
int main() {
  uint64_t p[24];
  int codes[5];
  memcpy(p, FqParams::G1_GEN_X64, 96); memcpy(p + 12, FqParams::G1_GEN_Y64, 96);
  codes[0] = point_check_lane(p, 0);
  memcpy(p, FqParams::G2_GEN_X64, 96); memcpy(p + 12, FqParams::G2_GEN_Y64, 96);
  codes[1] = point_check_lane(p, 1);
  memset(p, 0, sizeof p);
  codes[2] = point_check_lane(p, 0);
  memcpy(p, FqParams::ONE64, 96);
  codes[3] = point_check_lane(p, 0);
  memcpy(p + 12, FqParams::P64, 96);
  codes[4] = point_check_lane(p, 0);
  printf("%d %d %d %d %d\n", codes[0], codes[1], codes[2], codes[3], codes[4]);
  return 0;
}
#endif
