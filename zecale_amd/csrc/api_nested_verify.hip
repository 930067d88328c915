// C ABI (include/zkhip.h): nested (BLS12-377) Groth16 verification in batches on the device (pairing_bls.hip).  The host side of a
// handle lives here: what it derives from its key (nested_key.hpp: the curve checks, the lines of -beta, -delta and the negated
// generator, the doubling chains 2^j ABC_i), the host route of the test hook and the fallback of proofs the device does not decide;
// and the host route of the CHECKED batches (nested_point_check_host.hpp: encoding, curve and order of a point, range of an input),
// which also checks a checked handle's key before anything else reads it; and the host side of the COMBINED batches
// (nested_combine_host.hpp: the sums, the shared finish behind both routes, the host route).
#include <string.h>
#include <chrono>
#include <stdexcept>
#include <string>
#include <thread>

#include "api_internal.hpp"
#include "circuit/sections.hpp"
#include "nested_combine_host.hpp"
#include "nested_key.hpp"
#include "nested_point_check_host.hpp"
#include "pairing.cuh"               // verify_refusal: one definition for both checked routes
#include "pairing.h"                 // pairing_key_refusal
#include "pairing_bls.h"

using namespace zkhip::api;
namespace C = zkhip::circuit;

#pragma GCC visibility push(hidden)      // this file's own helpers and handle structs

struct zkhip_nested_verifier {
  NestedCtx* ctx;
  int device;
  size_t n_inputs;
  std::vector<uint64_t> vk;              // the key as given: the fallback verifies under it
  size_t last_fallbacks;
  std::vector<uint8_t> status;
  bool checked;                          // made by zkhip_nested_verifier_new_checked: the key's points passed the host point check
  // combined batches (zkhip_nested_verifier_verify_all)
  std::vector<zkhip::circuit::G2Lines<zkhip::circuit::NF>> key_lines;   // of -beta, -delta and the negated generator, for the host finish (made at the first call)
  size_t last_degenerate;                // proofs of the last combined batch whose B has a degenerate line schedule
  double finish_ms;                      // host time of the last combined batch behind the device's work
  std::vector<uint64_t> chunk_products, chunk_sums;
  std::vector<uint8_t> left_out;
};

namespace {

using C::HFr;
using C::NF;

using zkhip::nested_key::g1_on_curve;
using zkhip::nested_key::g2_on_curve;
using zkhip::nested_key::put;
using zkhip::nested_key::PreparedKey;

// the constants every context needs: the Frobenius scalings and the twist's -1/5
struct NestedConsts {
  std::vector<uint64_t> frob, fifth_neg;
  NestedConsts() {
    for (int i = 0; i < 12; i++) put(frob, C::fq12_consts().frob[i]);
    put(fifth_neg, C::small_consts().fifth_neg);
  }
};
const NestedConsts& nested_consts() { static NestedConsts c; return c; }

NestedKeyData consts_only() {
  NestedKeyData kd = {};
  kd.frob = nested_consts().frob.data();
  kd.fifth_neg = nested_consts().fifth_neg.data();
  return kd;
}

// the host point check of a key's k + 4 points; a failure leaves pairing_key_refusal's message in t_err
int nested_key_point_check(const uint64_t* nested_vk, size_t k) {
  size_t element = 0;
  const int code = zkhip::nested_key::key_check_host(nested_vk, k, &element);
  if (!code) return ZKHIP_OK;
  pairing_key_refusal(element, code, t_err, sizeof t_err);
  return ZKHIP_ERR_ARG;
}

int nested_verifier_new(const uint64_t* nested_vk, size_t inputs_per_proof, bool checked, zkhip_nested_verifier** out) {
  if (!nested_vk || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (inputs_per_proof > 16) return fail(ZKHIP_ERR_ARG, "inputs_per_proof 0 .. 16");
  if (checked) {                                                        // before anything else reads the key's limbs as field elements
    const int rc = nested_key_point_check(nested_vk, inputs_per_proof);
    if (rc != ZKHIP_OK) return rc;
  }
  PreparedKey pk;
  try {
    std::string why;                                                    // on the host, before a device is touched
    if (!zkhip::nested_key::prepare_key(nested_vk, inputs_per_proof, &pk, &why)) return fail(ZKHIP_ERR_ARG, why.c_str());
  } catch (const std::exception& e) {
    return fail(ZKHIP_ERR_STATE, e.what());
  }
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called (the nested pairing kernels are the only batch verifier)");
  BIND_CUR();
  NestedKeyData kd = consts_only();
  kd.alpha = nested_vk;
  kd.abc0 = nested_vk + 60;
  kd.lines = pk.lines.data();
  kd.chain = pk.chain.data();
  kd.n_inputs = inputs_per_proof;
  NestedCtx* ctx = nullptr;
  const int rc = nested_ctx_new(&kd, &ctx, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  zkhip_nested_verifier* v = new zkhip_nested_verifier{ctx, cur_dev(), inputs_per_proof, {}, 0, {}, checked, {}, 0, 0, {}, {}, {}};
  v->vk.assign(nested_vk, nested_vk + 60 + 12 * (inputs_per_proof + 1));
  *out = v;
  return ZKHIP_OK;
}

// one batch on either route.  out: ok bytes (1 / 0), or on the checked route the status bytes of zkhip.h.  What the device marked
// degenerate is decided by the host's verifier; a refused proof is never among them (nested_verify_batch clears its status).
int nested_verifier_run(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs, size_t count, bool checked, uint8_t* out) {
  v->last_fallbacks = 0;
  if (count == 0) return ZKHIP_OK;
  if (!nested_proofs || !out || (v->n_inputs && !nested_inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(v);
  v->status.resize(count);
  const int rc = nested_verify_batch(v->ctx, nested_inputs, nested_proofs, count, checked, out, v->status.data(), t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  const uint64_t* vk = v->vk.data();
  size_t fallbacks = 0;
  for (size_t i = 0; i < count; i++) {
    if (!(v->status[i] & NESTED_DEGENERATE)) continue;
    fallbacks++;
    const uint64_t* pr = nested_proofs + i * 48;
    int one = 0;
    const int rc2 = zkhip_bls12_377_groth16_verify(vk, vk + 12, vk + 36, vk + 60, v->n_inputs ? nested_inputs + i * v->n_inputs * 6 : nullptr, v->n_inputs,
                                                   pr, pr + 12, pr + 36, &one);
    if (rc2 != ZKHIP_OK) return fail(rc2, "the host verifier refused a proof the device handed back");
    out[i] = checked ? (uint8_t)(one ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_REJECT) : (uint8_t)(one ? 1 : 0);
  }
  v->last_fallbacks = fallbacks;
  return ZKHIP_OK;
}

namespace NC = zkhip::nested_combine;

// the scalars of a combined batch: the caller's (none zero), or count x 16 bytes from the OS into `own`
int nested_combine_scalars(const uint64_t* rho, size_t count, std::vector<uint64_t>& own, const uint64_t** out) {
  if (rho) {
    for (size_t i = 0; i < count; i++) if ((rho[i * 2] | rho[i * 2 + 1]) == 0) return fail(ZKHIP_ERR_ARG, "a combination scalar is zero");
    *out = rho;
    return ZKHIP_OK;
  }
  own.resize(count * 2);
  if (!zkhip::host::draw_rho(own.data(), count)) return fail(ZKHIP_ERR_STATE, "getrandom failed: no scalars for the combination, and no weaker generator stands in");
  *out = own.data();
  return ZKHIP_OK;
}

unsigned host_route_threads() {
  const unsigned hw = std::thread::hardware_concurrency();
  return hw > 16 ? 16 : hw;
}

// the handle's key in the finish's form; its lines are made at the first combined batch (the key passed prepare_key: none is degenerate)
int handle_combine_key(zkhip_nested_verifier* v, NC::CombineKey* key) {
  if (v->key_lines.empty() && !NC::key_lines(v->vk.data() + 12, v->vk.data() + 36, &v->key_lines)) return fail(ZKHIP_ERR_STATE, "the key's line schedules are degenerate");
  key->alpha = v->vk.data();
  key->abc = v->vk.data() + 60;
  key->n_inputs = v->n_inputs;
  key->lines = v->key_lines;
  return ZKHIP_OK;
}

// The combined check on the device route: the reduced value, the refusal bytes (checked handle, or null) and the proofs left out.
// The device gives per chunk the unreduced product of the per-proof pairs and the sum of the rho_i C_i; the host multiplies and adds
// the chunks' results, forms the sums in the scalar field over the proofs that are not left out, and finishes (combined_value).
int nested_verify_all_device(zkhip_nested_verifier* v, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                             uint8_t* refusal, uint64_t* value) {
  NC::CombineKey key;
  int rc = handle_combine_key(v, &key);
  if (rc != ZKHIP_OK) return rc;
  const size_t chunks = nested_verify_all_chunks(count);
  v->chunk_products.resize(chunks * 72);
  v->chunk_sums.resize(chunks * 12);
  v->left_out.resize(count);
  if ((rc = nested_verify_all(v->ctx, inputs, proofs, count, rho, checked, v->chunk_products.data(), v->chunk_sums.data(), v->left_out.data(), refusal,
                              t_err, sizeof t_err)) != ZKHIP_OK)
    return rc;
  const auto t0 = std::chrono::steady_clock::now();
  NC::CombineSums sums(v->n_inputs);
  size_t degenerate = 0;
  for (size_t i = 0; i < count; i++) {
    if (!v->left_out[i]) sums.add(rho + i * 2, inputs + i * v->n_inputs * 6);
    else if (!(v->left_out[i] & NESTED_OFF_CURVE)) degenerate++;
  }
  zkhip::circuit::Fq12<zkhip::circuit::NF> product = zkhip::circuit::Fq12<zkhip::circuit::NF>::one();
  NC::NestedJac<HFr> s_c = NC::NestedJac<HFr>::infinity();
  for (size_t k = 0; k < chunks; k++) {
    product = product * NC::fq12_from_limbs(&v->chunk_products[k * 72]);
    const uint64_t* p = &v->chunk_sums[k * 12];
    uint64_t nz = 0;
    for (int t = 0; t < 12; t++) nz |= p[t];
    if (nz) s_c = s_c.add_affine(HFr::from_limbs(p), HFr::from_limbs(p + 6));
  }
  NC::fq12_to_limbs(NC::combined_value(key, sums, NC::to_affine(s_c), product), value);
  v->last_degenerate = degenerate;
  v->finish_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ZKHIP_OK;
}

}  // namespace

#pragma GCC visibility pop

extern "C" {

int zkhip_nested_verifier_new(const uint64_t* nested_vk, size_t inputs_per_proof, zkhip_nested_verifier** out) {
  return nested_verifier_new(nested_vk, inputs_per_proof, false, out);
}
int zkhip_nested_verifier_new_checked(const uint64_t* nested_vk, size_t inputs_per_proof, zkhip_nested_verifier** out) {
  return nested_verifier_new(nested_vk, inputs_per_proof, true, out);
}

// ---- the checks of the checked nested verifier on the host (nested_point_check_host.hpp): no device
int zkhip_bls12_377_point_check(const uint64_t* p, int g2, int* code) {
  if (!p || !code) return fail(ZKHIP_ERR_ARG, "null pointer");
  *code = zkhip::nested_key::point_check_host(p, g2 != 0);
  return ZKHIP_OK;
}

int zkhip_bls12_377_groth16_verify_checked(const uint64_t vk_alpha_g1[12], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                           const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs, const uint64_t proof_a[12],
                                           const uint64_t proof_b[24], const uint64_t proof_c[12], uint8_t* status) {
  namespace K = zkhip::nested_key;
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc || !proof_a || !proof_b || !proof_c || !status || (n_inputs && !inputs))
    return fail(ZKHIP_ERR_ARG, "null pointer");
  const uint64_t* key[3] = {vk_alpha_g1, vk_beta_g2, vk_delta_g2};
  for (size_t i = 0; i < n_inputs + 4; i++) {      // the order and the words of zkhip_nested_verifier_new_checked
    const int code = K::point_check_host(i < 3 ? key[i] : vk_abc + (i - 3) * 12, i == 1 || i == 2);
    if (!code) continue;
    pairing_key_refusal(i, code, t_err, sizeof t_err);
    return ZKHIP_ERR_ARG;
  }
  uint8_t e[4];
  e[0] = (uint8_t)K::point_check_host(proof_a, false);
  e[1] = (uint8_t)K::point_check_host(proof_b, true);
  e[2] = (uint8_t)K::point_check_host(proof_c, false);
  e[3] = (uint8_t)K::inputs_check_host(inputs, n_inputs);
  if ((*status = verify_refusal(e)) != 0) return ZKHIP_OK;
  int ok = 0;
  const int rc = zkhip_bls12_377_groth16_verify(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, inputs, n_inputs, proof_a, proof_b, proof_c, &ok);
  if (rc != ZKHIP_OK) return fail(rc, "zkhip_bls12_377_groth16_verify failed");
  *status = ok ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_REJECT;
  return ZKHIP_OK;
}

size_t zkhip_nested_verifier_num_inputs(const zkhip_nested_verifier* v) { return v ? v->n_inputs : 0; }

int zkhip_nested_verifier_verify_batch(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs, size_t count,
                                       uint8_t* ok) {
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  return nested_verifier_run(v, nested_inputs, nested_proofs, count, false, ok);
}

int zkhip_nested_verifier_verify_batch_checked(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs, size_t count,
                                               uint8_t* status) {
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  if (!v->checked) return fail(ZKHIP_ERR_STATE, "checked batches need a handle of zkhip_nested_verifier_new_checked");
  return nested_verifier_run(v, nested_inputs, nested_proofs, count, true, status);
}

int zkhip_nested_verifier_last_fallbacks(const zkhip_nested_verifier* v, size_t* out) {
  if (!v || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  *out = v->last_fallbacks;
  return ZKHIP_OK;
}

// ---- combined batches: ONE random-combination check for a whole batch
int zkhip_nested_verifier_verify_all(zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs, size_t count,
                                     const uint64_t* rho, int* all_ok, uint8_t* status) {
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  if (!all_ok) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (status && !v->checked) return fail(ZKHIP_ERR_STATE, "a per-proof status needs a handle of zkhip_nested_verifier_new_checked");
  v->last_degenerate = 0;
  v->finish_ms = 0;
  if (count == 0) { *all_ok = 1; return ZKHIP_OK; }
  if (!nested_proofs || (v->n_inputs && !nested_inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  int rc = nested_combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  BIND(v);
  uint64_t value[72];
  try {
    if ((rc = nested_verify_all_device(v, nested_inputs, nested_proofs, count, rho, status != nullptr, status, value)) != ZKHIP_OK) return rc;
  } catch (const std::exception& e) {
    return fail(ZKHIP_ERR_STATE, e.what());
  }
  bool ok = NC::gt_is_one(value);
  for (size_t i = 0; ok && i < count; i++) ok = v->left_out[i] == 0;      // a proof that is left out of the product fails the batch
  *all_ok = ok ? 1 : 0;
  return ZKHIP_OK;
}

// the combined check on the host alone (nested_combine_host.hpp): the route zkhip_nested_verifier_verify_all is pinned on
int zkhip_bls12_377_groth16_verify_all(const uint64_t vk_alpha_g1[12], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24], const uint64_t* vk_abc,
                                       size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, int* all_ok) {
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc || !all_ok) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (count == 0) { *all_ok = 1; return ZKHIP_OK; }
  if (!proofs || (n_inputs && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  const int rc = nested_combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  try {
    // well-formedness first, as zkhip_bls12_377_groth16_verify: a key point off its curve fails the batch before any pairing arithmetic
    bool wf = g1_on_curve(C::g1_from<NF>(vk_alpha_g1, false)) && g2_on_curve(C::g2_from<NF>(vk_beta_g2, false)) && g2_on_curve(C::g2_from<NF>(vk_delta_g2, false));
    for (size_t i = 0; i <= n_inputs && wf; i++) wf = g1_on_curve(C::g1_from<NF>(vk_abc + i * 12, false));
    NC::CombineKey key = {vk_alpha_g1, vk_abc, n_inputs, {}};
    if (!wf || !NC::key_lines(vk_beta_g2, vk_delta_g2, &key.lines)) { *all_ok = 0; return ZKHIP_OK; }
    std::vector<uint8_t> left_out(count);
    uint64_t value[72];
    NC::verify_all_host(key, inputs, proofs, count, rho, nullptr, host_route_threads(), left_out.data(), value);
    bool ok = NC::gt_is_one(value);
    for (size_t i = 0; ok && i < count; i++) ok = left_out[i] == 0;      // a point off its curve, a degenerate line schedule
    *all_ok = ok ? 1 : 0;
  } catch (const std::exception& e) {
    return fail(ZKHIP_ERR_STATE, e.what());
  }
  return ZKHIP_OK;
}

int zkhip_nested_verifier_last_degenerate(const zkhip_nested_verifier* v, size_t* out) {
  if (!v || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  *out = v->last_degenerate;
  return ZKHIP_OK;
}

int zkhip_internal_nested_verify_all_value(int route, zkhip_nested_verifier* v, const uint64_t* nested_inputs, const uint64_t* nested_proofs,
                                           size_t count, const uint64_t* rho, uint64_t out[72]) {
  if (route != 0 && route != 1) return fail(ZKHIP_ERR_ARG, "route 0 (host) or 1 (GPU)");
  if (!v || !out || (count && (!nested_proofs || !rho || (v->n_inputs && !nested_inputs)))) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  int rc = nested_combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  try {
    if (route == 1 && count) {
      BIND(v);
      return nested_verify_all_device(v, nested_inputs, nested_proofs, count, rho, v->checked, nullptr, out);
    }
    NC::CombineKey key;
    if ((rc = handle_combine_key(v, &key)) != ZKHIP_OK) return rc;
    std::vector<uint8_t> refused, left_out(count);
    if (v->checked) {                                // the checked route's refusals, on the host: such a proof is left out
      namespace K = zkhip::nested_key;
      refused.resize(count);
      for (size_t i = 0; i < count; i++) {
        const uint64_t* pr = nested_proofs + i * 48;
        const uint8_t e[4] = {(uint8_t)K::point_check_host(pr, false), (uint8_t)K::point_check_host(pr + 12, true), (uint8_t)K::point_check_host(pr + 36, false),
                              (uint8_t)K::inputs_check_host(nested_inputs + i * v->n_inputs * 6, v->n_inputs)};
        refused[i] = verify_refusal(e);
      }
    }
    NC::verify_all_host(key, nested_inputs, nested_proofs, count, rho, v->checked ? refused.data() : nullptr, host_route_threads(), left_out.data(), out);
  } catch (const std::exception& e) {
    return fail(ZKHIP_ERR_STATE, e.what());
  }
  return ZKHIP_OK;
}
int zkhip_internal_nested_verify_all_finish_ms(const zkhip_nested_verifier* v, double* ms) {
  if (!v || !ms) return fail(ZKHIP_ERR_ARG, "null pointer");
  *ms = v->finish_ms;
  return ZKHIP_OK;
}

void zkhip_nested_verifier_free(zkhip_nested_verifier* v) {
  if (!v) return;
  if (bind_dev(v->device) == ZKHIP_OK) nested_ctx_free(v->ctx);
  delete v;
}

int zkhip_internal_fq12_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
  BIND_CUR();
  if (op < 0 || op > 2 || (n && (!a || !b || !out)) || n > (1u << 20)) return fail(ZKHIP_ERR_ARG, "op 0 (mul), 1 (sqr) or 2 (mul_line), at most 2^20 sets");
  if (n == 0) return ZKHIP_OK;
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return nested_fq12_selftest(op, a, b, n, out, t_err, sizeof t_err);
}

int zkhip_internal_nested_pairing_product(int route, const uint64_t* g1, const uint64_t* g2, size_t pairs_per_product, size_t count, uint64_t* out) {
  if ((route != 0 && route != 1) || pairs_per_product < 1 || pairs_per_product > 4) return fail(ZKHIP_ERR_ARG, "route 0 (host) or 1 (GPU), 1 .. 4 pairs per product");
  if (count && (!g1 || !g2 || !out)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (count == 0) return ZKHIP_OK;
  const size_t np = pairs_per_product;
  try {
    for (size_t i = 0; i < count * np; i++)
      if (!g1_on_curve(C::g1_from<NF>(g1 + i * 12, false)) || !g2_on_curve(C::g2_from<NF>(g2 + i * 24, false)))
        return fail(ZKHIP_ERR_ARG, "a point is off its curve");
    if (route == 0) {
      for (size_t i = 0; i < count; i++) {
        std::vector<C::G2<NF>> Qs;
        for (size_t p = 0; p < np; p++) Qs.push_back(C::g2_from<NF>(g2 + (i * np + p) * 24, false));
        const std::vector<C::G2Lines<NF>> lines = C::g2_precompute<NF>(Qs);
        std::vector<C::MillerPair<NF>> ps;
        for (size_t p = 0; p < np; p++) ps.push_back({&lines[p], C::g1_from<NF>(g1 + (i * np + p) * 12, false)});
        const C::Fq12<NF> v = C::final_exponentiation(C::multi_miller_loop(ps));
        for (int k = 0; k < 12; k++) v.c[k].v.to_limbs(out + i * 72 + k * 6);
      }
      return ZKHIP_OK;
    }
  } catch (const std::exception& e) {
    return fail(ZKHIP_ERR_STATE, e.what());
  }
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called");
  BIND_CUR();
  const NestedKeyData kd = consts_only();
  NestedCtx* ctx = nullptr;
  int rc = nested_ctx_new(&kd, &ctx, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  std::vector<uint8_t> status(count);
  rc = nested_products(ctx, g1, g2, (int)np, count, out, status.data(), t_err, sizeof t_err);
  nested_ctx_free(ctx);
  if (rc != ZKHIP_OK) return rc;
  for (size_t i = 0; i < count; i++)
    if (status[i]) return fail(ZKHIP_ERR_STATE, "the line schedule of a G2 point is degenerate (a slope denominator is zero)");
  return ZKHIP_OK;
}

}  // extern "C"
