// Host-side test shim of the combined batches: the new per-lane bodies of zecale_amd/csrc/pairing.cuh (rho_scale, the strip product's
// operand select around fq6_mul_coeff, g1_strip_sum, xyzz_to_affine_abi) compiled for the CPU by g++ and driven lane after lane in the
// kernels' schedule, and the host route of pairing_host.hpp, so tests/test_pairing_combine_model.py can compare them with Python big
// integers without a GPU.  Test infrastructure only.
#include <string.h>

#include <vector>

#include "../zecale_amd/csrc/pairing.cuh"
#include "../zecale_amd/csrc/pairing_host.hpp"
using namespace zkhip;

static XYZZ from_abi_point(const uint64_t* p) {
  uint64_t nz = 0;
  for (int k = 0; k < 24; k++) nz |= p[k];
  return nz ? xyzz_from_affine(fp_from_abi<FqParams>(p), fp_from_abi<FqParams>(p + 12)) : xyzz_infinity();
}

extern "C" {
int pairing_strip() { return PAIRING_STRIP; }

// the integer rules of the host driver: proofs per chunk of the per-proof route, and the levels of a reduction tree over n values as
// the driver walks them - reads[k] values go into level k, which writes pairing_strips of them.  Returns the number of levels.
size_t batch_chunk(size_t n_inputs) { return pairing_batch_chunk(n_inputs); }
int tree_levels(size_t n, size_t* reads, size_t* writes) {
  const int levels = pairing_tree_levels(n);
  for (int k = 0; k < levels; k++, n = pairing_strips(n)) { reads[k] = n; writes[k] = pairing_strips(n); }
  return levels;
}

// k_rho_scale's A lane: rho P as affine ABI limbs, all zero for infinity
void rho_scale_lane(const uint64_t* p, const uint64_t* rho, uint64_t* out) { xyzz_to_affine_abi(rho_scale(p, rho), out); }

// One launch of k_gt_product on n values (72 ABI limbs each): strip after strip, the six coefficient lanes one after the other, both
// copies of the running product and of the operand as the kernel keeps them.  out: ceil(n / PAIRING_STRIP) x 72 limbs.
void gt_product_level(const uint64_t* vals, size_t n, uint64_t* out) {
  std::vector<Fq> in(n * 6);
  for (size_t i = 0; i < n * 6; i++) in[i] = fp_from_abi<FqParams>(vals + i * 12);
  const size_t strips = (n + PAIRING_STRIP - 1) / PAIRING_STRIP;
  for (size_t s = 0; s < strips; s++) {
    const size_t first = s * PAIRING_STRIP;
    Fq F[2][6], B[2][6];
    for (int k = 0; k < 6; k++) {
      F[0][k] = gt_strip_operand(k, in.data(), first, 0, n);
      B[0][k] = gt_strip_operand(k, in.data(), first, 1, n);
    }
    int cur = 0;
    for (int i = 1; i < PAIRING_STRIP; i++) {
      for (int k = 0; k < 6; k++) {
        F[cur ^ 1][k] = fq6_mul_coeff(k, F[cur], B[cur]);
        if (i + 1 < PAIRING_STRIP) B[cur ^ 1][k] = gt_strip_operand(k, in.data(), first, i + 1, n);
      }
      cur ^= 1;
    }
    for (int k = 0; k < 6; k++) fp_to_abi<FqParams>(F[cur][k], out + s * 72 + k * 12);
  }
}

// One launch of k_g1_sum on n points (24 ABI limbs each, all zero = infinity), one lane per strip.  out: ceil(n / PAIRING_STRIP) x 24.
void g1_sum_level(const uint64_t* pts, size_t n, uint64_t* out) {
  std::vector<XYZZ> in(n);
  for (size_t i = 0; i < n; i++) in[i] = from_abi_point(pts + i * 24);
  const size_t strips = (n + PAIRING_STRIP - 1) / PAIRING_STRIP;
  for (size_t s = 0; s < strips; s++) xyzz_to_affine_abi(g1_strip_sum(in.data(), s * PAIRING_STRIP, n), out + s * 24);
}

// The host route (what zkhip_groth16_verify_all computes behind its curve check): the reduced value of the combined product.
void verify_all_value_host(const uint64_t* alpha, const uint64_t* beta, const uint64_t* delta, const uint64_t* abc, size_t n_inputs,
                           const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, unsigned threads, uint64_t* out) {
  using namespace host;
  uint64_t neg_g2[24], neg_beta[24], neg_delta[24];
  neg_g2_generator(neg_g2); neg_point_abi(beta, neg_beta); neg_point_abi(delta, neg_delta);
  const CombineKey key = {alpha, neg_g2, neg_beta, neg_delta, abc, n_inputs};
  CombineSums sums(n_inputs);
  Fq6 product = Fq6::one();
  HJac s_c = HJac::infinity();
  combined_proofs_host(n_inputs, inputs, proofs, count, rho, nullptr, threads, product, s_c, sums);
  fq6_to_limbs(combined_value(key, sums, s_c, product), out);
}

// count x 2 words from the OS; 1 when it worked
int draw_scalars(uint64_t* rho, size_t count) { return host::draw_rho(rho, count) ? 1 : 0; }
}

#ifdef PAIRING_COMBINE_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DPAIRING_COMBINE_SHIM_MAIN): the bodies on the generator
// with the all-ones scalar, strips of every length up to one past two strips (the operand select at the end of the array), infinity
// among the summands
#include <stdio.h>
int main() {
  uint64_t gen[24], rho[2] = {~0ull, ~0ull}, p[24];
  memcpy(gen, FqParams::G1_GEN_X64, 96); memcpy(gen + 12, FqParams::G1_GEN_Y64, 96);
  rho_scale_lane(gen, rho, p);
  uint64_t acc = 0;
  for (int i = 0; i < 24; i++) acc ^= p[i];
  const size_t top = 2 * PAIRING_STRIP + 1;
  std::vector<uint64_t> vals(top * 72, 0), pts(top * 24, 0), out(top * 72);
  for (size_t i = 0; i < top; i++) {
    for (int k = 0; k < 6; k++) memcpy(&vals[i * 72 + k * 12], k % 2 ? p : p + 12, 96);
    if (i % 3) memcpy(&pts[i * 24], i % 2 ? p : gen, 192);
  }
  for (size_t n = 1; n <= top; n++) {
    gt_product_level(vals.data(), n, out.data());
    for (size_t i = 0; i < (n + PAIRING_STRIP - 1) / PAIRING_STRIP * 72; i++) acc ^= out[i];
    g1_sum_level(pts.data(), n, out.data());
    for (size_t i = 0; i < (n + PAIRING_STRIP - 1) / PAIRING_STRIP * 24; i++) acc ^= out[i];
  }
  printf("%016llx\n", (unsigned long long)acc);
  return 0;
}
#endif
