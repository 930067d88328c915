// C ABI (include/zkhip.h): Groth16 verification - on the host, and in batches on the device (pairing.hip).
#include <string.h>

#include "api_internal.hpp"
#include "device_buffer.hpp"
#include "ec.cuh"
#include "pairing_host.hpp"
#include "pairing.cuh"
#include "pairing.h"
#include "pairing_locate.hpp"

using namespace zkhip::api;

#pragma GCC visibility push(hidden)      // this file's own helpers and handle structs

struct zkhip_verifier {
  PairingCtx* ctx;
  int device;
  std::vector<host::LocateTraceNode> trace;      // of the last located call (zkhip_internal_locate_trace)
};

// ---- Groth16 verification in batches on the device (pairing.hip)
static int verifier_new(const uint64_t* vk_alpha_g1, const uint64_t* vk_beta_g2, const uint64_t* vk_delta_g2, const uint64_t* vk_abc, size_t n_inputs,
                        bool checked, zkhip_verifier** out) {
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called (the pairing kernels are the only batch verifier)");
  BIND_CUR();
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  PairingCtx* ctx = nullptr;
  const int rc = pairing_ctx_new(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs, checked, &ctx, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  *out = new zkhip_verifier{ctx, cur_dev(), {}};
  return ZKHIP_OK;
}

// the scalars of a combined batch: the caller's (none zero), or count x 16 bytes from the OS into `own`
static int combine_scalars(const uint64_t* rho, size_t count, std::vector<uint64_t>& own, const uint64_t** out) {
  if (rho) {
    for (size_t i = 0; i < count; i++) if ((rho[i * 2] | rho[i * 2 + 1]) == 0) return fail(ZKHIP_ERR_ARG, "a combination scalar is zero");
    *out = rho;
    return ZKHIP_OK;
  }
  own.resize(count * 2);
  if (!host::draw_rho(own.data(), count)) return fail(ZKHIP_ERR_STATE, "getrandom failed: no scalars for the combination, and no weaker generator stands in");
  *out = own.data();
  return ZKHIP_OK;
}

// the combined check on the host alone: the reduced value.  skip: null, or the proofs left out.
static void verify_all_host(const host::CombineKey& key, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                            const uint8_t* skip, uint64_t* value) {
  using namespace host;
  const unsigned hw = std::thread::hardware_concurrency();
  CombineSums sums(key.n_inputs);
  Fq6 product = Fq6::one();
  HJac s_c = HJac::infinity();
  combined_proofs_host(key.n_inputs, inputs, proofs, count, rho, skip, hw > 16 ? 16 : hw, product, s_c, sums);
  fq6_to_limbs(combined_value(key, sums, s_c, product), value);
}

static void add_locate_stats(zkhip_locate_stats& sum, const zkhip_locate_stats& s) {
  sum.chunks_failed += s.chunks_failed; sum.rounds += s.rounds; sum.node_tests += s.node_tests; sum.finish_proofs += s.finish_proofs;
  sum.invalid += s.invalid; sum.descent_ms += s.descent_ms; sum.finish_ms += s.finish_ms;
}

// The located route on the host alone, cut into located batches.  left_out: null, or per proof the byte a proof that is left out
// everywhere gets (0: it takes part).  bytes: the verdicts are status bytes (ACCEPT 0 / REJECT 1), else 1 / 0.  The per-proof route of
// the host is verify_one_host, the proofs dealt to the threads of a round.
static int located_host(const host::CombineKey& key, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                        const uint8_t* left_out, bool bytes, uint8_t* verdict, zkhip_locate_stats* stats, std::vector<host::LocateTraceNode>* trace,
                        uint64_t* value_out = nullptr) {
  using namespace host;
  const uint8_t accept = bytes ? (uint8_t)ZKHIP_VERIFY_ACCEPT : 1, reject = bytes ? (uint8_t)ZKHIP_VERIFY_REJECT : 0;
  const unsigned threads = locate_threads();
  const size_t ni = key.n_inputs;
  zkhip_locate_stats sum = zkhip_locate_stats();
  const int rc = for_each_chunk(count, PAIRING_LOCATE_MAX, [&](size_t lo, size_t m) -> int {
    const uint64_t *in = inputs + lo * ni * 6, *pr = proofs + lo * 72;
    const uint8_t* skip = left_out ? left_out + lo : nullptr;
    std::vector<uint8_t> state;
    zkhip_locate_stats s;
    uint64_t value[72];
    auto finish = [&](const std::vector<size_t>& list) -> int {
      const unsigned nt = threads > list.size() ? (unsigned)list.size() : threads;
      auto work = [&](unsigned t) {
        for (size_t i = t; i < list.size(); i += nt)
          if (!skip || !skip[list[i]]) verdict[lo + list[i]] = verify_one_host(key, in + list[i] * ni * 6, pr + list[i] * 72) ? accept : reject;
      };
      std::vector<std::thread> pool;
      for (unsigned t = 1; t < nt; t++) pool.emplace_back(work, t);
      work(0);
      for (auto& th : pool) th.join();
      return 0;
    };
    for (size_t i = 0; i < m; i++) verdict[lo + i] = skip && skip[i] ? skip[i] : accept;
    const int r = located_batch_host(key, in, pr, m, rho + lo * 2, skip, threads, LOCATE_COST, finish, state, s, trace, value);
    if (r) return r;
    for (size_t i = 0; i < m; i++)
      if (state[i] == locate::INVALID) verdict[lo + i] = reject;
    for (size_t i = 0; i < m; i++) s.invalid += verdict[lo + i] == reject && (!skip || !skip[i]);
    add_locate_stats(sum, s);
    if (value_out) memcpy(value_out, value, sizeof value);
    return ZKHIP_OK;
  });
  if (stats) *stats = sum;
  return rc;
}

#pragma GCC visibility pop

extern "C" {

int zkhip_groth16_verify(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                         const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs, const uint64_t proof_affine[72],
                         int* ok) {
  using namespace host;
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc || !proof_affine || !ok || (n_inputs && !inputs))
    return fail(ZKHIP_ERR_ARG, "null pointer");
  auto aff = [](const uint64_t* p) { return HJac::from_affine(HFq::from_limbs(p), HFq::from_limbs(p + 12)); };
  // well-formedness first: a proof or a key with a point off its curve is rejected before any pairing arithmetic
  if (!proof_on_curve(proof_affine) || !key_on_curve(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs)) { *ok = 0; return ZKHIP_OK; }
  // acc = ABC_0 + sum x_i ABC_i
  HJac acc = aff(vk_abc);
  for (size_t i = 0; i < n_inputs; i++) {
    uint64_t k[6];
    HFr::from_limbs(inputs + i * 6).to_canonical(k);
    acc = acc.add(aff(vk_abc + (i + 1) * 24).mul_canonical(k, 6));
  }
  uint64_t acc_aff[24], neg_g2[24], neg_beta[24], neg_delta[24];
  HFq x, y;
  acc.to_affine(x, y); x.to_limbs(acc_aff); y.to_limbs(acc_aff + 12);
  neg_g2_generator(neg_g2); neg_point_abi(vk_beta_g2, neg_beta); neg_point_abi(vk_delta_g2, neg_delta);
  std::vector<const uint64_t*> p1 = {proof_affine, acc_aff, vk_alpha_g1, proof_affine + 48};
  std::vector<const uint64_t*> p2 = {proof_affine + 24, neg_g2, neg_beta, neg_delta};
  *ok = pairing_product_is_one(p1, p2) ? 1 : 0;
  return ZKHIP_OK;
}

// ---- the combined check on the host alone (pairing_host.hpp): the route zkhip_verifier_verify_all is pinned on
int zkhip_groth16_verify_all(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24], const uint64_t* vk_abc,
                             size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, const uint64_t* rho, int* all_ok) {
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc || !all_ok) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (count == 0) { *all_ok = 1; return ZKHIP_OK; }
  if (!proofs_affine || (n_inputs && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  const int rc = combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  // well-formedness first, as zkhip_groth16_verify: a point off its curve fails the batch before any pairing arithmetic
  bool wf = host::key_on_curve(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs);
  for (size_t i = 0; i < count && wf; i++) wf = host::proof_on_curve(proofs_affine + i * 72);
  if (!wf) { *all_ok = 0; return ZKHIP_OK; }
  uint64_t neg_g2[24], neg_beta[24], neg_delta[24], value[72];
  host::neg_g2_generator(neg_g2); host::neg_point_abi(vk_beta_g2, neg_beta); host::neg_point_abi(vk_delta_g2, neg_delta);
  const host::CombineKey key = {vk_alpha_g1, neg_g2, neg_beta, neg_delta, vk_abc, n_inputs};
  verify_all_host(key, inputs, proofs_affine, count, rho, nullptr, value);
  *all_ok = host::gt_is_one(value) ? 1 : 0;
  return ZKHIP_OK;
}

// ---- located batches on the host alone (pairing_locate.hpp): the route zkhip_verifier_verify_batch_located is pinned on
int zkhip_groth16_verify_batch_located(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24], const uint64_t* vk_abc,
                                       size_t n_inputs, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, const uint64_t* rho,
                                       uint8_t* ok, zkhip_locate_stats* stats) {
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (stats) *stats = zkhip_locate_stats();
  if (count == 0) return ZKHIP_OK;
  if (!proofs_affine || !ok || (n_inputs && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  int rc = combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  // well-formedness first, as zkhip_groth16_verify: a point off its curve never enters the pairing arithmetic
  if (!host::key_on_curve(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs)) { memset(ok, 0, count); return ZKHIP_OK; }
  std::vector<uint8_t> off(count);
  for (size_t i = 0; i < count; i++) off[i] = host::proof_on_curve(proofs_affine + i * 72) ? 0 : 0xFF;
  uint64_t neg_g2[24], neg_beta[24], neg_delta[24];
  host::neg_g2_generator(neg_g2); host::neg_point_abi(vk_beta_g2, neg_beta); host::neg_point_abi(vk_delta_g2, neg_delta);
  const host::CombineKey key = {vk_alpha_g1, neg_g2, neg_beta, neg_delta, vk_abc, n_inputs};
  if ((rc = located_host(key, inputs, proofs_affine, count, rho, off.data(), false, ok, stats, nullptr)) != ZKHIP_OK) return fail(rc, "located batch");
  for (size_t i = 0; i < count; i++) if (off[i]) ok[i] = 0;
  return ZKHIP_OK;
}

// ---- the checks of the checked verifier on the host (pairing_host.hpp point_check_host): no device
int zkhip_bw6_761_point_check(const uint64_t p[24], int g2, int* code) {
  if (!p || !code) return fail(ZKHIP_ERR_ARG, "null pointer");
  *code = host::point_check_host(p, g2 != 0);
  return ZKHIP_OK;
}

int zkhip_groth16_verify_checked(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24],
                                 const uint64_t* vk_abc, const uint64_t* inputs, size_t n_inputs, const uint64_t proof_affine[72],
                                 uint8_t* status) {
  if (!vk_alpha_g1 || !vk_beta_g2 || !vk_delta_g2 || !vk_abc || !proof_affine || !status || (n_inputs && !inputs))
    return fail(ZKHIP_ERR_ARG, "null pointer");
  const uint64_t* key[3] = {vk_alpha_g1, vk_beta_g2, vk_delta_g2};
  for (size_t i = 0; i < n_inputs + 4; i++) {      // the order and the words of the device route's key check
    const int code = host::point_check_host(i < 3 ? key[i] : vk_abc + (i - 3) * 24, i == 1 || i == 2);
    if (!code) continue;
    pairing_key_refusal(i, code, t_err, sizeof t_err);
    return ZKHIP_ERR_ARG;
  }
  uint8_t e[4];
  host::proof_check_codes_host(proof_affine, inputs, n_inputs, e);
  if ((*status = verify_refusal(e)) != 0) return ZKHIP_OK;
  int ok = 0;
  const int rc = zkhip_groth16_verify(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, inputs, n_inputs, proof_affine, &ok);
  if (rc != ZKHIP_OK) return rc;
  *status = ok ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_REJECT;
  return ZKHIP_OK;
}

int zkhip_verifier_new(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24], const uint64_t* vk_abc,
                       size_t n_inputs, zkhip_verifier** out) {
  return verifier_new(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs, false, out);
}
int zkhip_verifier_new_checked(const uint64_t vk_alpha_g1[24], const uint64_t vk_beta_g2[24], const uint64_t vk_delta_g2[24], const uint64_t* vk_abc,
                               size_t n_inputs, zkhip_verifier** out) {
  return verifier_new(vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs, true, out);
}
size_t zkhip_verifier_num_inputs(const zkhip_verifier* v) { return v ? pairing_ctx_num_inputs(v->ctx) : 0; }
int zkhip_verifier_verify_batch(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, uint8_t* ok) {
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  if (count == 0) return ZKHIP_OK;
  if (!proofs_affine || !ok || (pairing_ctx_num_inputs(v->ctx) && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(v);
  return pairing_verify_batch(v->ctx, inputs, proofs_affine, count, false, ok, t_err, sizeof t_err);
}
int zkhip_verifier_verify_batch_checked(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, uint8_t* status) {
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  if (!pairing_ctx_checked(v->ctx)) return fail(ZKHIP_ERR_STATE, "checked batches need a handle of zkhip_verifier_new_checked");
  if (count == 0) return ZKHIP_OK;
  if (!proofs_affine || !status || (pairing_ctx_num_inputs(v->ctx) && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(v);
  return pairing_verify_batch(v->ctx, inputs, proofs_affine, count, true, status, t_err, sizeof t_err);
}
int zkhip_verifier_verify_all(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, const uint64_t* rho,
                              int* all_ok, uint8_t* status) {
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  if (!all_ok) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (status && !pairing_ctx_checked(v->ctx)) return fail(ZKHIP_ERR_STATE, "a per-proof status needs a handle of zkhip_verifier_new_checked");
  if (count == 0) { *all_ok = 1; return ZKHIP_OK; }
  if (!proofs_affine || (pairing_ctx_num_inputs(v->ctx) && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  int rc = combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  BIND(v);
  uint64_t value[72];
  if ((rc = pairing_verify_all(v->ctx, inputs, proofs_affine, count, rho, status != nullptr, status, value, t_err, sizeof t_err)) != ZKHIP_OK) return rc;
  bool ok = host::gt_is_one(value);
  for (size_t i = 0; status && ok && i < count; i++) ok = status[i] == 0;      // a refused proof is left out of the product and fails the batch
  *all_ok = ok ? 1 : 0;
  return ZKHIP_OK;
}
int zkhip_internal_verify_batch_located(int route, zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                                        const uint64_t* rho, uint8_t* verdict, zkhip_locate_stats* stats, uint64_t* value) {
  if (route != 0 && route != 1) return fail(ZKHIP_ERR_ARG, "route 0 (host) or 1 (GPU)");
  if (!v) return fail(ZKHIP_ERR_ARG, "null verifier");
  zkhip_locate_stats sum = zkhip_locate_stats();
  if (stats) *stats = sum;
  v->trace.clear();
  if (count == 0) return ZKHIP_OK;
  const size_t ni = pairing_ctx_num_inputs(v->ctx);
  if (!proofs_affine || !verdict || (ni && !inputs)) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  int rc = combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  const bool checked = pairing_ctx_checked(v->ctx);
  if (route == 0) {
    host::CombineKey key;
    key.n_inputs = ni;
    pairing_ctx_key(v->ctx, &key.alpha, &key.neg_g2, &key.neg_beta, &key.neg_delta, &key.abc);
    std::vector<uint8_t> refused;
    if (checked) {                                 // the checked route's refusals, on the host: such a proof is left out
      refused.resize(count);
      for (size_t i = 0; i < count; i++) {
        uint8_t e[4];
        host::proof_check_codes_host(proofs_affine + i * 72, inputs + i * ni * 6, ni, e);
        refused[i] = verify_refusal(e);
      }
    }
    if ((rc = located_host(key, inputs, proofs_affine, count, rho, checked ? refused.data() : nullptr, checked, verdict, stats, &v->trace, value)) != ZKHIP_OK)
      return fail(rc, "located batch");
    return ZKHIP_OK;
  }
  BIND(v);
  rc = for_each_chunk(count, PAIRING_LOCATE_MAX, [&](size_t lo, size_t m) -> int {      // a batch above the bound: consecutive located batches
    zkhip_locate_stats s;
    uint64_t piece[72];
    const int r = pairing_verify_located(v->ctx, inputs + lo * ni * 6, proofs_affine + lo * 72, m, rho + lo * 2, checked, verdict + lo, &s, piece, &v->trace,
                                         t_err, sizeof t_err);
    if (r == ZKHIP_OK) add_locate_stats(sum, s);
    if (r == ZKHIP_OK && value) memcpy(value, piece, sizeof piece);
    return r;
  });
  if (stats) *stats = sum;
  return rc;
}
int zkhip_verifier_verify_batch_located(zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count, const uint64_t* rho,
                                        uint8_t* verdict, zkhip_locate_stats* stats) {
  return zkhip_internal_verify_batch_located(1, v, inputs, proofs_affine, count, rho, verdict, stats, nullptr);
}
int zkhip_internal_locate_trace(const zkhip_verifier* v, zkhip_locate_node* out, size_t cap, size_t* count) {
  if (!v || !count) return fail(ZKHIP_ERR_ARG, "null pointer");
  *count = v->trace.size();
  for (size_t i = 0; out && i < v->trace.size() && i < cap; i++) {
    const host::LocateTraceNode& t = v->trace[i];
    out[i].chunk = t.node.chunk; out[i].level = t.node.level; out[i].passed = t.passed ? 1 : 0; out[i].reserved = 0;
    out[i].index = t.node.index;
    memcpy(out[i].value, t.value, sizeof t.value);
  }
  return ZKHIP_OK;
}
void zkhip_verifier_free(zkhip_verifier* v) {
  if (!v) return;
  if (bind_dev(v->device) == ZKHIP_OK) pairing_ctx_free(v->ctx);
  delete v;
}

int zkhip_internal_fq6_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
  BIND_CUR();
  if (op < 0 || op > 2 || (n && (!a || !b || !out)) || n > (1u << 20)) return fail(ZKHIP_ERR_ARG, "op 0 (mul), 1 (sqr) or 2 (mul_line), at most 2^20 sets");
  if (n == 0) return ZKHIP_OK;
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return pairing_fq6_selftest(op, a, b, n, out, t_err, sizeof t_err);
}

int zkhip_internal_pairing_product(int route, const uint64_t* g1, const uint64_t* g2, size_t pairs_per_product, size_t count, uint64_t* out) {
  if ((route != 0 && route != 1) || pairs_per_product < 1 || pairs_per_product > 4) return fail(ZKHIP_ERR_ARG, "route 0 (host) or 1 (GPU), 1 .. 4 pairs per product");
  if (count && (!g1 || !g2 || !out)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (count == 0) return ZKHIP_OK;
  if (route == 0) {
    for (size_t i = 0; i < count; i++) {
      std::vector<const uint64_t*> p1, p2;
      for (size_t p = 0; p < pairs_per_product; p++) { p1.push_back(g1 + (i * pairs_per_product + p) * 24); p2.push_back(g2 + (i * pairs_per_product + p) * 24); }
      const host::Fq6 v = host::pairing_product_value(p1, p2);
      for (int k = 0; k < 6; k++) v.c[k].to_limbs(out + i * 72 + k * 12);
    }
    return ZKHIP_OK;
  }
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called");
  BIND_CUR();
  PairingCtx* ctx = nullptr;
  int rc = pairing_ctx_new(nullptr, nullptr, nullptr, nullptr, 0, false, &ctx, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  rc = pairing_products(ctx, g1, g2, (int)pairs_per_product, count, out, t_err, sizeof t_err);
  pairing_ctx_free(ctx);
  return rc;
}

int zkhip_internal_verify_all_value(int route, zkhip_verifier* v, const uint64_t* inputs, const uint64_t* proofs_affine, size_t count,
                                    const uint64_t* rho, uint64_t out[72]) {
  if (route != 0 && route != 1) return fail(ZKHIP_ERR_ARG, "route 0 (host) or 1 (GPU)");
  if (!v || !out || (count && (!proofs_affine || !rho || (pairing_ctx_num_inputs(v->ctx) && !inputs)))) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::vector<uint64_t> own;
  int rc = combine_scalars(rho, count, own, &rho);
  if (rc != ZKHIP_OK) return rc;
  const bool checked = pairing_ctx_checked(v->ctx);
  if (route == 1 && count) {
    BIND(v);
    return pairing_verify_all(v->ctx, inputs, proofs_affine, count, rho, checked, nullptr, out, t_err, sizeof t_err);
  }
  host::CombineKey key;
  key.n_inputs = pairing_ctx_num_inputs(v->ctx);
  pairing_ctx_key(v->ctx, &key.alpha, &key.neg_g2, &key.neg_beta, &key.neg_delta, &key.abc);
  std::vector<uint8_t> skip;
  if (checked) {                                   // the checked route's refusals, on the host: such a proof is left out
    skip.resize(count);
    for (size_t i = 0; i < count; i++) {
      uint8_t e[4];
      host::proof_check_codes_host(proofs_affine + i * 72, inputs + i * key.n_inputs * 6, key.n_inputs, e);
      skip[i] = verify_refusal(e);
    }
  }
  verify_all_host(key, inputs, proofs_affine, count, rho, checked ? skip.data() : nullptr, out);
  return ZKHIP_OK;
}
int zkhip_internal_verify_all_finish_ms(const zkhip_verifier* v, double* ms) {
  if (!v || !ms) return fail(ZKHIP_ERR_ARG, "null pointer");
  *ms = pairing_ctx_last_finish_ms(v->ctx);
  return ZKHIP_OK;
}

}  // extern "C"
