// C ABI (include/zkhip.h): NTT, the constraint-system handle and its evaluation domain, the QAP map.
#include "api_internal.hpp"
#include "domain.hpp"
#include "ntt.h"

using namespace zkhip::api;

extern "C" {

int zkhip_ntt_dev(void* d_data, unsigned log_d, int dir, int coset) {
  BIND_CUR();
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  if (!d_data) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (log_d > 22) return fail(ZKHIP_ERR_ARG, "log_d must be <= 22");
  return ntt_dev_abi((uint64_t*)d_data, (int)log_d, dir != 0, coset != 0, t_err, sizeof t_err);
}

int zkhip_ntt(uint64_t* data, unsigned log_d, int dir, int coset) {
  BIND_CUR();
  if (!data) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (log_d > 22) return fail(ZKHIP_ERR_ARG, "log_d must be <= 22");
  size_t bytes = ((size_t)48) << log_d;
  Scratch sc;
  void* d = nullptr;
  API_HIP(sc.alloc(&d, bytes));
  API_HIP(hipMemcpy(d, data, bytes, hipMemcpyHostToDevice));
  int rc = zkhip_ntt_dev(d, log_d, dir, coset);
  if (rc == ZKHIP_OK) API_HIP(hipMemcpy(data, d, bytes, hipMemcpyDeviceToHost));
  return rc;
}

int zkhip_r1cs_upload_ex(const zkhip_r1cs_desc* d, size_t domain_size, zkhip_r1cs** out) {
  BIND_CUR();
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  if (!d || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  R1csDev* dev = nullptr;
  int rc = r1cs_upload(d, domain_size, &dev, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  *out = new zkhip_r1cs{dev, cur_dev()};
  return ZKHIP_OK;
}
int zkhip_r1cs_upload(const zkhip_r1cs_desc* d, zkhip_r1cs** out) { return zkhip_r1cs_upload_ex(d, 0, out); }   // the reference's forced power of two

int zkhip_r1cs_set_domain(zkhip_r1cs* r, size_t domain_size) {
  if (!r) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(r);
  std::lock_guard<std::mutex> lk(g.dev[r->device].mu);
  return r1cs_set_domain(r->dev, domain_size, t_err, sizeof t_err);
}

void zkhip_r1cs_free(zkhip_r1cs* r) {
  if (!r) return;
  (void)bind_dev(r->device);
  r1cs_free(r->dev);
  delete r;
}

unsigned zkhip_r1cs_log_domain(const zkhip_r1cs* r) { return r ? (unsigned)r->dev->log_d : 0; }
size_t zkhip_r1cs_domain_size(const zkhip_r1cs* r) { return r ? r->dev->d : 0; }
size_t zkhip_domain_size(size_t min_size) { return host::forced_domain_size(min_size); }
size_t zkhip_step_domain_size(size_t min_size) { return host::eval_domain_size(min_size); }
int zkhip_domain_is_valid(size_t domain_size) { return host::is_valid_domain(domain_size) ? 1 : 0; }

int zkhip_r1cs_is_satisfied(zkhip_r1cs* r, const uint64_t* z, int* ok) {
  if (!r || !z || !ok) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(r);
  std::lock_guard<std::mutex> lk(g.dev[r->device].mu);
  Scratch sc;
  uint64_t* dz = nullptr;
  API_HIP(sc.alloc((void**)&dz, r->dev->n_vars * 48));
  API_HIP(hipMemcpy(dz, z, r->dev->n_vars * 48, hipMemcpyHostToDevice));
  return r1cs_is_satisfied_dev(r->dev, dz, 0, ok, t_err, sizeof t_err);
}

int zkhip_qap_h(zkhip_r1cs* r, const uint64_t* z, uint64_t* h_out) {
  if (!r || !z || !h_out) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(r);
  std::lock_guard<std::mutex> lk(g.dev[r->device].mu);
  size_t d = r->dev->d;
  Scratch sc;
  uint64_t *dz = nullptr, *dh = nullptr;
  API_HIP(sc.alloc((void**)&dz, r->dev->n_vars * 48));
  API_HIP(sc.alloc((void**)&dh, d * 48));
  API_HIP(hipMemcpy(dz, z, r->dev->n_vars * 48, hipMemcpyHostToDevice));
  int rc = qap_h_dev(r->dev, dz, 0, t_err, sizeof t_err);
  if (rc == ZKHIP_OK) {
    fr_dev_to_abi(r->dev->bufA, dh, d, 0);
    API_HIP(hipMemcpy(h_out, dh, d * 48, hipMemcpyDeviceToHost));
  }
  return rc;
}

int zkhip_measure_ntt(unsigned log_d, int dir, int coset, int batch, int reps, double* ms_per_transform) {
  BIND_CUR();
  if (!ms_per_transform) return fail(ZKHIP_ERR_ARG, "null pointer");
  return ntt_measure((int)log_d, dir, coset, batch, reps, ms_per_transform, t_err, sizeof t_err);
}

// Test hooks of the transform passes in device layout (ntt.hip ntt_packed_hook, one_each_max)
int zkhip_internal_ntt_packed(void* data, int form, int nbuf, unsigned log_d, int dir, int coset, int in_transposed) {
  BIND_CUR();
  if (!data) return fail(ZKHIP_ERR_ARG, "null pointer");
  if ((form != 0 && form != 1) || nbuf < 1 || nbuf > 3 || log_d > 22 || (dir != 0 && dir != 1) || (coset != 0 && coset != 1) || (in_transposed != 0 && in_transposed != 1))
    return fail(ZKHIP_ERR_ARG, "form, dir, coset, in_transposed 0 or 1; 1 to 3 vectors; log_d <= 22");
  if (!dir && coset && in_transposed && log_d >= 12) return fail(ZKHIP_ERR_ARG, "ntt: a forward coset transform takes its input in natural order");
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return ntt_packed_hook(data, form, nbuf, (int)log_d, dir, coset, in_transposed, t_err, sizeof t_err);
}
int zkhip_internal_ntt_set_one_each_max(int log_d_max) {
  if (ntt_set_one_each_max(log_d_max) != ZKHIP_OK) return fail(ZKHIP_ERR_ARG, "log_d_max must be in [-1, 22]");
  return ZKHIP_OK;
}

}  // extern "C"
