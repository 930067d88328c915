// Host-side test shim: the per-lane bodies of zecale_amd/csrc/pairing_bls.cuh (the code the nested pairing kernels run on every lane)
// compiled for the CPU by g++ and driven lane by lane, so tests/test_nested_pairing_model.py can compare them with Python big integers
// and with the host route without a GPU.  Test infrastructure only.
#include "../zecale_amd/csrc/pairing_bls.cuh"
using namespace zkhip;

static void load12(const uint64_t* a, Fr* o) { for (int k = 0; k < 12; k++) o[k] = fp_from_abi<FrParams>(a + k * 6); }

extern "C" {
// op 0: a b, 1: a^2, 2: a (b0 + b1 w + b3 w^3 + b7 w^7 + b9 w^9); 12 x 6 ABI limbs each
void fq12_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  Fr A[12], B[12], L[5];
  load12(a, A); load12(b, B);
  L[0] = B[0]; L[1] = B[1]; L[2] = B[3]; L[3] = B[7]; L[4] = B[9];
  for (int k = 0; k < 12; k++) {
    const Fr r = op == 0 ? fq12_mul_coeff(k, A, B) : op == 1 ? fq12_mul_coeff(k, A, A) : fq12_mul_line_coeff(k, A, L);
    fp_to_abi<FrParams>(r, out + k * 6);
  }
}

// The kernels' schedule for ONE product of np <= 4 pairs, lanes run one after the other: the lines of every G2 point (k_nested_g2_lines),
// the Miller loop (k_nested_miller), the final exponentiation's program (k_nested_final_exp).  g1: np x 12 ABI limbs, g2: np x 24,
// frob: the twelve Frobenius constants (ABI).  out: 12 x 6 ABI limbs.  Returns 1 when a line schedule was degenerate.
int nested_product_lanes(const uint64_t* g1, const uint64_t* g2, int np, const uint64_t* frob_abi, uint64_t* out) {
  static NestedLine lines[NESTED_MAX_PAIRS][NESTED_LINES];
  Fr px[NESTED_MAX_PAIRS], py[NESTED_MAX_PAIRS], L[NESTED_MAX_PAIRS][5], F[2][12], frob[12];
  static Fr reg[FQ12_REGS][12];
  int degenerate = 0;
  load12(frob_abi, frob);
  for (int p = 0; p < np; p++) {
    const uint64_t* q = g2 + p * 24;
    const Fr2 qx{fp_from_abi<FrParams>(q), fp_from_abi<FrParams>(q + 6)}, qy{fp_from_abi<FrParams>(q + 12), fp_from_abi<FrParams>(q + 18)};
    if (!g2_lines_lane(qx, qy, lines[p])) degenerate = 1;
    px[p] = fp_from_abi<FrParams>(g1 + p * 12);
    py[p] = fp_from_abi<FrParams>(g1 + p * 12 + 6);
  }
  for (int k = 0; k < 12; k++) F[0][k] = k == 0 ? fp_one<FrParams>() : fp_zero<FrParams>();
  int cur = 0, at = 0;
  for (int i = 62; i >= 0; i--) {
    for (int add = 0; add < 2; add++) {
      if (add && !((NESTED_U >> i) & 1)) break;
      if (!add) { for (int k = 0; k < 12; k++) F[cur ^ 1][k] = fq12_mul_coeff(k, F[cur], F[cur]); }
      for (int p = 0; p < np; p++) nested_line_at(lines[p][at], px[p], py[p], L[p]);
      if (!add) cur ^= 1;
      for (int p = 0; p < np; p++) {
        for (int k = 0; k < 12; k++) F[cur ^ 1][k] = fq12_mul_line_coeff(k, F[cur], L[p]);
        cur ^= 1;
      }
      at++;
    }
  }
  for (int k = 0; k < 12; k++) reg[0][k] = F[cur][k];
  for (const Fq12Op& o : fq12_final_exp_program())
    for (int k = 0; k < 12; k++) fq12_op_lane(o, k, reg, frob);
  for (int k = 0; k < 12; k++) fp_to_abi<FrParams>(reg[0][k], out + k * 6);
  return degenerate;
}

// the accumulator body of k_nested_acc: abc0 (12 ABI limbs), chain (n_inputs x 253 x 12), inputs (n_inputs x 6) -> out (12 ABI limbs).
// Returns 1 when a step took the same-x branch.
int nested_acc(const uint64_t* abc0, const uint64_t* chain, const uint64_t* inputs, size_t n_inputs, uint64_t* out) {
  std::vector<Fr> ch(n_inputs * NESTED_INPUT_BITS_DEV * 2);
  for (size_t i = 0; i < ch.size(); i++) ch[i] = fp_from_abi<FrParams>(chain + i * 6);
  const Fr a0[2] = {fp_from_abi<FrParams>(abc0), fp_from_abi<FrParams>(abc0 + 6)};
  Fr o[2];
  const bool fine = nested_acc_lane(a0, ch.data(), inputs, n_inputs, o);
  fp_to_abi<FrParams>(o[0], out);
  fp_to_abi<FrParams>(o[1], out + 6);
  return fine ? 0 : 1;
}

// the curve checks of k_nested_prep: g2 = 0: a G1 point (12 limbs); else a G2 point (24 limbs) with -1/5 (6 limbs)
int nested_on_curve(const uint64_t* p, int g2, const uint64_t* fifth_neg) {
  if (!g2) return nested_g1_on_curve(fp_from_abi<FrParams>(p), fp_from_abi<FrParams>(p + 6)) ? 1 : 0;
  const Fr2 x{fp_from_abi<FrParams>(p), fp_from_abi<FrParams>(p + 6)}, y{fp_from_abi<FrParams>(p + 12), fp_from_abi<FrParams>(p + 18)};
  return nested_g2_on_curve(x, y, fp_from_abi<FrParams>(fifth_neg)) ? 1 : 0;
}
}

#ifdef NESTED_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DNESTED_SHIM_MAIN): every coefficient at q - 1 (Montgomery
// form of -1 is p - ONE64) through the three Fq12 bodies and the final exponentiation's program
#include <stdio.h>
int main() {
  uint64_t a[72], out[72];
  for (int k = 0; k < 12; k++) {
    unsigned __int128 br = 0;
    for (int i = 0; i < 6; i++) {
      unsigned __int128 t = (unsigned __int128)FrParams::P64[i] - FrParams::ONE64[i] - br;
      a[k * 6 + i] = (uint64_t)t;
      br = (t >> 64) & 1;
    }
  }
  uint64_t acc = 0;
  for (int op = 0; op < 3; op++) { fq12_op(op, a, a, out); for (int i = 0; i < 72; i++) acc ^= out[i]; }
  static Fr reg[FQ12_REGS][12];
  Fr frob[12];
  load12(a, frob);
  load12(a, reg[0]);
  for (const Fq12Op& o : fq12_final_exp_program())
    for (int k = 0; k < 12; k++) fq12_op_lane(o, k, reg, frob);
  for (int k = 0; k < 12; k++) { fp_to_abi<FrParams>(reg[0][k], out + k * 6); }
  for (int i = 0; i < 72; i++) acc ^= out[i];
  printf("%016llx\n", (unsigned long long)acc);
  return 0;
}
#endif
