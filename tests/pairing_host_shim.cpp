// Host-side test shim: the per-lane bodies of zecale_amd/csrc/pairing.cuh (the code the pairing kernels run on every lane) compiled
// for the CPU by g++ and driven lane by lane, so tests/test_pairing_model.py can compare them with Python big integers and with the
// host pairing without a GPU.  Test infrastructure only.
#include "../zecale_amd/csrc/pairing.cuh"
using namespace zkhip;

static void load6(const uint64_t* a, Fq* o) { for (int k = 0; k < 6; k++) o[k] = fp_from_abi<FqParams>(a + k * 12); }

extern "C" {
// op 0: a b, 1: a^2, 2: a (b0 + b3 w^3 + b4 w^4); 6 x 12 ABI limbs each
void fq6_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  Fq A[6], B[6], L[3];
  load6(a, A); load6(b, B);
  L[0] = B[0]; L[1] = B[3]; L[2] = B[4];
  for (int k = 0; k < 6; k++) {
    const Fq r = op == 0 ? fq6_mul_coeff(k, A, B) : op == 1 ? fq6_mul_coeff(k, A, A) : fq6_mul_line_coeff(k, A, L);
    fp_to_abi<FqParams>(r, out + k * 12);
  }
}

// The kernels' schedule for ONE product of np <= 4 pairs, lanes run one after the other: Miller loop (k_miller), then the final
// exponentiation by `e` (k_final_exp).  quarter: 1/4 and -1/4 (ABI).  out: 6 x 12 ABI limbs.
void pairing_product_lanes(const uint64_t* g1, const uint64_t* g2, int np, const uint64_t* quarter, const uint64_t* r_order,
                           const uint64_t* e, int e_bits, uint64_t* out) {
  MillerConst c[PAIRING_MAX_PAIRS];
  MillerPoint T[PAIRING_MAX_PAIRS];
  bool done[PAIRING_MAX_PAIRS];
  Fq L[PAIRING_MAX_PAIRS][3], F[2][6], B[6];
  for (int p = 0; p < np; p++) {
    uint64_t nz1 = 0, nz2 = 0;
    for (int k = 0; k < 24; k++) { nz1 |= g1[p * 24 + k]; nz2 |= g2[p * 24 + k]; }
    c[p].px = fp_from_abi<FqParams>(g1 + p * 24);
    c[p].py = fp_from_abi<FqParams>(g1 + p * 24 + 12);
    c[p].xq4 = fp_mul(fp_from_abi<FqParams>(g2 + p * 24), fp_from_abi<FqParams>(quarter));
    c[p].yq4n = fp_mul(fp_from_abi<FqParams>(g2 + p * 24 + 12), fp_from_abi<FqParams>(quarter + 12));
    done[p] = nz1 == 0 || nz2 == 0;
    T[p].X = c[p].px; T[p].Y = c[p].py; T[p].Z = fp_one<FqParams>();
  }
  for (int k = 0; k < 6; k++) F[0][k] = k == 0 ? fp_one<FqParams>() : fp_zero<FqParams>();
  int cur = 0;
  auto fold = [&]() {
    for (int p = 0; p < np; p++) {
      for (int k = 0; k < 6; k++) F[cur ^ 1][k] = fq6_mul_line_coeff(k, F[cur], L[p]);
      cur ^= 1;
    }
  };
  for (int i = PAIRING_MILLER_STEPS - 1; i >= 0; i--) {
    for (int k = 0; k < 6; k++) F[cur ^ 1][k] = fq6_mul_coeff(k, F[cur], F[cur]);
    for (int p = 0; p < np; p++) miller_double_step(T[p], c[p], done[p], L[p]);
    cur ^= 1;
    fold();
    if ((r_order[i >> 6] >> (i & 63)) & 1) {
      for (int p = 0; p < np; p++) done[p] = miller_add_step(T[p], c[p], done[p], L[p]);
      fold();
    }
  }
  for (int k = 0; k < 6; k++) { B[k] = F[cur][k]; F[0][k] = B[k]; }
  cur = 0;
  for (int i = e_bits - 2; i >= 0; i--) {
    for (int k = 0; k < 6; k++) F[cur ^ 1][k] = fq6_mul_coeff(k, F[cur], F[cur]);
    cur ^= 1;
    if ((e[i >> 6] >> (i & 63)) & 1) {
      for (int k = 0; k < 6; k++) F[cur ^ 1][k] = fq6_mul_coeff(k, F[cur], B);
      cur ^= 1;
    }
  }
  for (int k = 0; k < 6; k++) fp_to_abi<FqParams>(F[cur][k], out + k * 12);
}
}

#ifdef PAIRING_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DPAIRING_SHIM_MAIN): every coefficient at q - 1
// (Montgomery form of -1 is p - ONE64) through the three bodies
#include <stdio.h>
int main() {
  uint64_t a[72], out[72];
  for (int k = 0; k < 6; k++) {
    unsigned __int128 br = 0;
    for (int i = 0; i < 12; i++) {
      unsigned __int128 t = (unsigned __int128)FqParams::P64[i] - FqParams::ONE64[i] - br;
      a[k * 12 + i] = (uint64_t)t;
      br = (t >> 64) & 1;
    }
  }
  uint64_t acc = 0;
  for (int op = 0; op < 3; op++) { fq6_op(op, a, a, out); for (int i = 0; i < 72; i++) acc ^= out[i]; }
  printf("%016llx\n", (unsigned long long)acc);
  return 0;
}
#endif
