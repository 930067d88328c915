// Host-side test shim of the nested verifier's combined batches: the new per-lane bodies of zecale_amd/csrc/pairing_bls.cuh
// (nested_rho_scale, the strip product's operand select around fq12_mul_coeff, nested_g1_strip_sum with the complete XYZZ addition,
// nested_xyzz_to_affine_abi) compiled for the CPU by g++ and driven lane after lane in the kernels' schedule, and the host route of
// nested_combine_host.hpp, so tests/test_nested_combine_model.py can compare them with Python big integers without a GPU.
// Test infrastructure only.
#include <string.h>

#include <vector>

#include "../zecale_amd/csrc/nested_combine_host.hpp"
#include "../zecale_amd/csrc/pairing_bls.cuh"
using namespace zkhip;
namespace NC = zkhip::nested_combine;

// 12 ABI limbs (x | y), all zero = infinity (the sum tree's own encoding) -> XYZZ with ZZ = ZZZ = 1
static NestedXYZZ<Fr> from_abi_point(const uint64_t* p) {
  uint64_t nz = 0;
  for (int k = 0; k < 12; k++) nz |= p[k];
  if (!nz) return nested_xyzz_infinity<Fr>();
  NestedXYZZ<Fr> r;
  r.X = fp_from_abi<FrParams>(p); r.Y = fp_from_abi<FrParams>(p + 6);
  r.ZZ = fp_one<FrParams>(); r.ZZZ = fp_one<FrParams>();
  return r;
}

extern "C" {
int nested_strip() { return NESTED_STRIP; }

// the levels of a reduction tree over n values as the driver walks them - reads[k] values go into level k, which writes nested_strips
// of them.  Returns the number of levels.
int tree_levels(size_t n, size_t* reads, size_t* writes) {
  const int levels = nested_tree_levels(n);
  for (int k = 0; k < levels; k++, n = nested_strips(n)) { reads[k] = n; writes[k] = nested_strips(n); }
  return levels;
}

// k_nested_rho_scale's A lane: rho P as affine ABI limbs, all zero for infinity.  p: 12 ABI limbs of a finite point.
void rho_scale_lane(const uint64_t* p, const uint64_t* rho, uint64_t* out) {
  nested_xyzz_to_affine_abi(nested_rho_scale(fp_from_abi<FrParams>(p), fp_from_abi<FrParams>(p + 6), rho), out);
}

// One launch of k_nested_gt_product on n values (72 ABI limbs each): strip after strip, the twelve coefficient lanes one after the
// other, both copies of the running product and of the operand as the kernel keeps them.  skip: null, or n bytes.
// out: ceil(n / NESTED_STRIP) x 72 limbs.
void gt_product_level(const uint64_t* vals, size_t n, const uint8_t* skip, uint64_t* out) {
  std::vector<Fr> in(n * 12);
  for (size_t i = 0; i < n * 12; i++) in[i] = fp_from_abi<FrParams>(vals + i * 6);
  const size_t strips = nested_strips(n);
  for (size_t s = 0; s < strips; s++) {
    const size_t first = s * NESTED_STRIP;
    Fr F[2][12], B[2][12];
    for (int k = 0; k < 12; k++) {
      F[0][k] = nested_gt_strip_operand(k, in.data(), first, 0, n, skip);
      B[0][k] = nested_gt_strip_operand(k, in.data(), first, 1, n, skip);
    }
    int cur = 0;
    for (int i = 1; i < NESTED_STRIP; i++) {
      for (int k = 0; k < 12; k++) {
        F[cur ^ 1][k] = fq12_mul_coeff(k, F[cur], B[cur]);
        if (i + 1 < NESTED_STRIP) B[cur ^ 1][k] = nested_gt_strip_operand(k, in.data(), first, i + 1, n, skip);
      }
      cur ^= 1;
    }
    for (int k = 0; k < 12; k++) fp_to_abi<FrParams>(F[cur][k], out + s * 72 + k * 6);
  }
}

// One launch of k_nested_g1_sum on n points (12 ABI limbs each, all zero = infinity), one lane per strip.  scale: 0, or a factor z (ABI
// limbs): every point enters as (x z^2, y z^3, z^2, z^3) - the same point in another representation, as the tree's partial sums are.
// out: ceil(n / NESTED_STRIP) x 12.
void g1_sum_level(const uint64_t* pts, size_t n, const uint64_t* scale, uint64_t* out) {
  std::vector<NestedXYZZ<Fr>> in(n);
  for (size_t i = 0; i < n; i++) {
    in[i] = from_abi_point(pts + i * 12);
    if (!scale || nf_is_zero_2p(in[i].ZZ)) continue;
    Fr z = fp_from_abi<FrParams>(scale);
    for (size_t t = 0; t < i; t++) z = fr_red(fp_add(z, fp_one<FrParams>()));           // another factor per position
    const Fr zz = fp_mul(z, z), zzz = fp_mul(zz, z);
    in[i].X = fp_mul(in[i].X, zz); in[i].Y = fp_mul(in[i].Y, zzz); in[i].ZZ = zz; in[i].ZZZ = zzz;
  }
  const size_t strips = nested_strips(n);
  for (size_t s = 0; s < strips; s++) nested_xyzz_to_affine_abi(nested_g1_strip_sum(in.data(), s * NESTED_STRIP, n), out + s * 12);
}

// The host route (what zkhip_bls12_377_groth16_verify_all computes): the reduced value of the combined product over the proofs that are
// not left out; left_out: count bytes.  vk: alpha | beta | delta | ABC.  Returns 0, or 1 when a line schedule of the key is degenerate.
int verify_all_value_host(const uint64_t* vk, size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                          unsigned threads, uint8_t* left_out, uint64_t* out) {
  NC::CombineKey key = {vk, vk + 60, n_inputs, {}};
  if (!NC::key_lines(vk + 12, vk + 36, &key.lines)) return 1;
  NC::verify_all_host(key, inputs, proofs, count, rho, nullptr, threads, left_out, out);
  return 0;
}

// sum_i rho_i x_i mod r through WideSum: x: count x 4 words (below 2^253), out: 4 words
void wide_sum(const uint64_t* rho, const uint64_t* x, size_t count, uint64_t* out) {
  NC::WideSum s;
  for (size_t i = 0; i < count; i++) s.add_product(rho + i * 2, x + i * 4);
  s.reduce(out);
}

// count x 2 words from the OS; 1 when it worked
int draw_scalars(uint64_t* rho, size_t count) { return host::draw_rho(rho, count) ? 1 : 0; }
}

#ifdef NESTED_COMBINE_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DNESTED_COMBINE_SHIM_MAIN): the bodies on the curve point
// (2, 3) with the all-ones scalar and on (-1, 0) with an even one, strips of every length up to one past two strips (the operand
// select at the end of the array, with and without skip bytes), infinity among the summands
#include <stdio.h>
int main() {
  uint64_t pt[12], two[12], rho[2] = {~0ull, ~0ull}, even[2] = {6, 0}, p[12], o[12];
  host::HFr::from_u64(2).to_limbs(pt); host::HFr::from_u64(3).to_limbs(pt + 6);
  host::HFr::one().neg().to_limbs(two); host::HFr::zero().to_limbs(two + 6);
  rho_scale_lane(pt, rho, p);
  rho_scale_lane(two, even, o);
  uint64_t acc = 0;
  for (int i = 0; i < 12; i++) acc ^= p[i] ^ (o[i] + 1);
  const size_t top = 2 * NESTED_STRIP + 1;
  std::vector<uint64_t> vals(top * 72, 0), pts(top * 12, 0), out(top * 72);
  std::vector<uint8_t> skip(top, 0);
  for (size_t i = 0; i < top; i++) {
    for (int k = 0; k < 12; k++) memcpy(&vals[i * 72 + k * 6], k % 2 ? p : p + 6, 48);
    if (i % 3) memcpy(&pts[i * 12], i % 2 ? p : pt, 96);
    skip[i] = i % 5 == 4;
  }
  for (size_t n = 1; n <= top; n++) {
    gt_product_level(vals.data(), n, n % 2 ? skip.data() : nullptr, out.data());
    for (size_t i = 0; i < nested_strips(n) * 72; i++) acc ^= out[i];
    g1_sum_level(pts.data(), n, n % 2 ? pt : nullptr, out.data());
    for (size_t i = 0; i < nested_strips(n) * 12; i++) acc ^= out[i];
  }
  uint64_t w[4], x[8] = {~0ull, ~0ull, ~0ull, (1ull << 61) - 1, 5, 0, 0, 0}, rr[4] = {~0ull, ~0ull, 7, 0};
  wide_sum(rr, x, 2, w);
  for (int i = 0; i < 4; i++) acc ^= w[i];
  printf("%016llx\n", (unsigned long long)acc);
  return 0;
}
#endif
