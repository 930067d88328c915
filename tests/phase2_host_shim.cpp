// Host-side test shim: the lane body of a phase-2 contribution (zecale_amd/csrc/phase2.cuh common_scalar_mul, the code
// k_common_scalar_mul runs on every lane), the host's recoding of the common scalar and the library's SHA-256, compiled for the CPU by
// g++, so tests/test_phase2_lane_model.py and tests/test_sha256_host.py can compare them with Python without a GPU.
// Test infrastructure only.
#include "../zecale_amd/csrc/phase2.cuh"
#include "../zecale_amd/csrc/sha256.hpp"
#include <string.h>
using namespace zkhip;

extern "C" {
// k: six canonical words -> digits (PHASE2_DIGIT_BUFFER bytes, least significant first); the number of digits
int phase2_recode(const uint64_t* k, int8_t* digits) { return phase2_naf_recode(k, digits); }
int phase2_digit_buffer() { return PHASE2_DIGIT_BUFFER; }
// o = k p: p, o 24 ABI limbs (x | y), k six canonical words
void phase2_lane(const uint64_t* p, const uint64_t* k, uint64_t* o) {
  int8_t digits[PHASE2_DIGIT_BUFFER];
  const int n = phase2_naf_recode(k, digits);
  common_scalar_mul(p, digits, n, o);
}
// the endomorphism form: the decomposition (k1, k2: three words of magnitude each, neg: two flags; 1 when both halves fit their bound),
// its digit buffer, and the lane body over it
int phase2_decompose(const uint64_t* k, uint64_t* k1, uint64_t* k2, int* neg) { return phase2_glv_decompose(k, k1, &neg[0], k2, &neg[1]) ? 1 : 0; }
int phase2_recode_glv(const uint64_t* k, int8_t* digits) { return phase2_glv_recode(k, digits); }
int phase2_glv_digits() { return PHASE2_GLV_DIGITS; }
int phase2_glv_bits() { return FrParams::GLV_BITS; }
void phase2_lambda(uint64_t* out) { memcpy(out, FrParams::GLV_LAMBDA64, 48); }
int phase2_lane_glv(const uint64_t* p, const uint64_t* k, uint64_t* o) {
  int8_t digits[PHASE2_DIGIT_BUFFER];
  const int n = phase2_glv_recode(k, digits);
  if (n < 0) return -1;
  common_scalar_mul_glv(p, digits, n, o);
  return n;
}
void sha256_shim(const uint8_t* data, size_t len, uint8_t* out) { host::sha256(data, len, out); }
// the same message in pieces of `piece` bytes: the incremental interface
void sha256_pieces_shim(const uint8_t* data, size_t len, size_t piece, uint8_t* out) {
  host::Sha256 h;
  for (size_t lo = 0; lo < len; lo += piece) h.update(data + lo, len - lo < piece ? len - lo : piece);
  h.finish(out);
}
}

#ifdef PHASE2_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DPHASE2_SHIM_MAIN): the generator times r - 1 (every digit of
// the longest chain), times a scalar whose recoding carries into a seventh word, the point at infinity, and two hashes
#include <stdio.h>
int main() {
  uint64_t p[24], o[24], k[6];
  memcpy(p, FqParams::G1_GEN_X64, 96); memcpy(p + 12, FqParams::G1_GEN_Y64, 96);
  memcpy(k, FqParams::R_ORDER64, 48); k[0] -= 1;
  phase2_lane(p, k, o);
  int neg = memcmp(o, p, 96) == 0 && memcmp(o + 12, p + 12, 96) != 0;
  for (int i = 0; i < 6; i++) k[i] = ~(uint64_t)0;
  phase2_lane(p, k, o);
  uint64_t og[24];
  memcpy(k, FqParams::R_ORDER64, 48); k[0] -= 2;
  phase2_lane(p, k, o);
  neg = neg && phase2_lane_glv(p, k, og) > 0 && memcmp(o, og, 192) == 0;      // the two forms agree
  memset(p, 0, sizeof p);
  phase2_lane(p, k, o);
  uint64_t nz = 0;
  for (int i = 0; i < 24; i++) nz |= o[i];
  uint8_t d[32], msg[1000];
  memset(msg, 'a', sizeof msg);
  sha256_shim(msg, 0, d);
  sha256_pieces_shim(msg, sizeof msg, 7, d);
  printf("%d %d %02x\n", neg, nz == 0, d[0]);
  return 0;
}
#endif
