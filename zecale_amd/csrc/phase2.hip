// C ABI (include/zkhip.h): phase-2 contributions - zkhip_keypair_contribute / zkhip_phase2_verify on the device, their _host forms on
// the host alone.
//
// THE CUT.  A contribution re-randomises delta: delta' = s delta in both groups, and every point of h_query and l_query is multiplied
// by s^-1 - up to 2^22 scalar multiplications per vector, ALL BY THE SAME SCALAR.  One lane per point of a staged chunk (key_check.hip's
// pattern: raw ABI limbs in by 16-byte loads, 24 ABI limbs out, all zero in is all zero out).  The host splits s^-1 once along G1's
// endomorphism, s^-1 = k1 + k2 lambda with |k1|, |k2| < 2^190, and recodes both halves into signed binary digits (phase2.cuh); every
// lane reads the same two digits at the same index, so a wave walks one chain: about 190 doublings, an addition of +-P or
// +-phi(P) = +-(omega x, y) at about a third of the positions for each half, one inversion.  k_common_scalar_mul has no LDS and no
// barrier.  (The signed-binary baseline over all of s^-1, 377 doublings, is the <false> instance: built only with
// -DZKHIP_PHASE2_BOTH_FORMS, for tools/phase2_ab.py, which measured it at 1.43 x the kept form's launch time.)  The digit array is the
// secret: it is cleared on the device and on the host before the call returns, on every path.
// The five single points, the proof of knowledge and the transcript hash are host work (microseconds to milliseconds).
// Verification reuses the key check: k_key_point_check / k_key_codes_reduce for the new points (dev_check_element), the MSM engine for
// the two sums of the ratio relation (dev_combination), pairing products on the host in parallel threads.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <string.h>
#include <sys/random.h>

#include <atomic>
#include <thread>
#include <vector>

#include "api_internal.hpp"
#include "combine_scalars.hpp"
#include "device_buffer.hpp"
#include "domain.hpp"
#include "key_check_internal.hpp"
#include "pairing_host.hpp"
#include "phase2.cuh"
#include "sha256.hpp"

using namespace zkhip::api;

namespace zkhip {

// ---- out[t] = k pts[t] for the recoded scalar k (digits, the same array for every lane); n points of 24 raw ABI limbs, 16-byte aligned
template <bool ENDO>
__global__ void __launch_bounds__(64) k_common_scalar_mul(const uint64_t* __restrict__ pts, size_t n, const int8_t* __restrict__ digits, int n_digits,
                                                          uint64_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const ulonglong2* src = reinterpret_cast<const ulonglong2*>(pts + t * 24);
  uint64_t p[24], o[24];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const ulonglong2 v = src[k];
    p[2 * k] = v.x;
    p[2 * k + 1] = v.y;
  }
  if (ENDO) common_scalar_mul_glv(p, digits, n_digits, o);
  else common_scalar_mul(p, digits, n_digits, o);
  ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + t * 24);
#pragma unroll
  for (int k = 0; k < 12; k++) dst[k] = make_ulonglong2(o[2 * k], o[2 * k + 1]);
}

}  // namespace zkhip

#pragma GCC visibility push(hidden)      // this file's own helpers
namespace {

using namespace zkhip::host;
using namespace zkhip::keycheck;

const char POK_TAG[] = "zkhip phase2 pok v1";        // hashed without their terminating zero
const char LINK_TAG[] = "zkhip phase2 link v1";

thread_local double t_last_ms[8] = {0};     // zkhip_internal_phase2_last_ms

// overwrite a secret so that the compiler keeps the stores
void wipe(void* p, size_t bytes) {
  volatile uint8_t* v = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < bytes; i++) v[i] = 0;
}

// the secrets of one contribution - s, k, s^-1 in every form this file holds them, c s, and the digits -; cleared when the call leaves,
// whichever way.  (What the host's scalar multiplications keep on their own stack frames while they run is not reached from here.)
struct Secrets {
  uint64_t s_m[6], k_m[6], s_can[6], k_can[6], sinv_can[6];
  HFr S, K, Sinv, cS;      // the same as field elements, and c s of the response
  int8_t digits[PHASE2_DIGIT_BUFFER];
  int n_digits = 0;
  ~Secrets() { wipe(this, sizeof *this); }
};

// a non-zero element of Fr from the OS, as six words below r (any such words are the Montgomery form of a uniform element)
bool draw_scalar(uint64_t out[6]) {
  for (;;) {
    size_t got = 0;
    while (got < 48) {
      const ssize_t n = getrandom(reinterpret_cast<char*>(out) + got, 48 - got, 0);
      if (n < 0 && errno == EINTR) continue;
      if (n <= 0) return false;
      got += (size_t)n;
    }
    out[5] &= ((uint64_t)1 << (377 - 320)) - 1;      // r has 377 bits: a draw of 377 bits is below r with probability > 1/2
    uint64_t nz = 0;
    for (int i = 0; i < 6; i++) nz |= out[i];
    if (nz && !HFr::geq_p(out)) return true;
  }
}

void point_mul(const uint64_t* p, const uint64_t k_can[6], uint64_t out[24]) {
  const HJac q = jac_from_limbs(p).mul_canonical(k_can, 6);
  if (q.is_inf()) memset(out, 0, 192);
  else jac_to_limbs(q, out);
}

// the Fiat-Shamir challenge: the first 16 bytes, little endian, of SHA-256(tag | prev_digest | delta_g1 | delta_g1' | T)
void pok_challenge(const uint8_t prev[32], const uint64_t* delta_g1, const uint64_t* delta_g1_new, const uint64_t* commit, uint64_t c[6]) {
  Sha256 h;
  uint8_t d[32];
  h.update(POK_TAG, sizeof POK_TAG - 1);
  h.update(prev, 32);
  h.update(delta_g1, 192);           // (24 ABI limbs, little endian: their bytes in memory)
  h.update(delta_g1_new, 192);
  h.update(commit, 192);
  h.finish(d);
  memset(c, 0, 48);
  memcpy(c, d, 16);
}

void link_digest(const uint8_t prev[32], const zkhip_phase2_contribution* rec, uint8_t out[32]) {
  Sha256 h;
  h.update(LINK_TAG, sizeof LINK_TAG - 1);
  h.update(prev, 32);
  h.update(rec->delta_g1, 192);
  h.update(rec->delta_g2, 192);
  h.update(rec->pok_commit, 192);
  h.update(rec->pok_response, 48);
  h.finish(out);
}

int check_desc(const zkhip_crs_desc* d) {
  if (!d->alpha_g1 || !d->beta_g1 || !d->beta_g2 || !d->delta_g1 || !d->delta_g2) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (d->n_vars < d->n_primary + 1 || d->domain_size < 1 || !is_valid_domain(d->domain_size)) return fail(ZKHIP_ERR_ARG, "phase 2: implausible sizes");
  if (d->n_vars >= ((size_t)1 << 30) || d->domain_size >= ((size_t)1 << 30)) return fail(ZKHIP_ERR_ARG, "phase 2: a vector of 2^30 points or more");
  if (!d->a_query || !d->b_g2_query || !d->b_g1_query) return fail(ZKHIP_ERR_ARG, "null pointer");
  if ((d->domain_size > 1 && !d->h_query) || (d->n_vars > d->n_primary + 1 && !d->l_query)) return fail(ZKHIP_ERR_ARG, "null pointer");
  return ZKHIP_OK;
}

// ---- out[i] = k in[i], i < n, on the host: the points dealt to up to 16 threads
void host_scale(const uint64_t* in, size_t n, const uint64_t k_can[6], uint64_t* out) {
  unsigned threads = std::thread::hardware_concurrency();
  if (threads > 16) threads = 16;
  if (threads < 1 || n < 32) threads = 1;
  auto work = [&](unsigned t) {
    for (size_t i = t; i < n; i += threads) {
      if (is_infinity(in + i * 24)) memset(out + i * 24, 0, 192);
      else point_mul(in + i * 24, k_can, out + i * 24);
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
}

// ---- which form of the kernel the device route runs.  The endomorphism form is the faster one (profiles/phase2.txt) and the only one
// in a normal build; -DZKHIP_PHASE2_BOTH_FORMS builds the baseline beside it for tools/phase2_ab.py, chosen by zkhip_internal_phase2_set_form.
enum { PHASE2_FORM_DEFAULT = 0, PHASE2_FORM_BASELINE = 1, PHASE2_FORM_ENDO = 2 };
std::atomic<int> g_form{PHASE2_FORM_DEFAULT};
int kernel_form() {
#ifdef ZKHIP_PHASE2_BOTH_FORMS
  if (g_form.load() == PHASE2_FORM_BASELINE) return PHASE2_FORM_BASELINE;
#endif
  return PHASE2_FORM_ENDO;
}
void launch_form(bool endo, unsigned blocks, hipStream_t st, const uint64_t* in, size_t m, const int8_t* digits, int n_digits, uint64_t* out) {
#ifdef ZKHIP_PHASE2_BOTH_FORMS
  if (!endo) { hipLaunchKernelGGL(k_common_scalar_mul<false>, dim3(blocks), dim3(64), 0, st, in, m, digits, n_digits, out); return; }
#endif
  (void)endo;
  hipLaunchKernelGGL(k_common_scalar_mul<true>, dim3(blocks), dim3(64), 0, st, in, m, digits, n_digits, out);
}

// ---- the same on the device, chunk by chunk on one stream.  The digit buffer is cleared when this goes out of scope.
struct Phase2Dev {
  DeviceStream st;
  DeviceBuffer<uint64_t> d_in, d_out;
  DeviceBuffer<int8_t> d_digits;
  std::vector<hipEvent_t> ev;
  ~Phase2Dev() {
    if (d_digits.get() && st.s) {
      (void)hipMemsetAsync(d_digits.get(), 0, PHASE2_DIGIT_BUFFER, st);
      (void)hipStreamSynchronize(st);
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

int scale_open(Phase2Dev& w, const Secrets& sec) {
  char* errbuf = t_err;
  const size_t errlen = sizeof t_err;
  ZK_HIP_TRY("phase 2", w.st.create());
  ZK_HIP_TRY("phase 2", w.d_digits.reserve(PHASE2_DIGIT_BUFFER));
  ZK_HIP_TRY("phase 2", hipMemcpyAsync(w.d_digits.get(), sec.digits, PHASE2_DIGIT_BUFFER, hipMemcpyHostToDevice, w.st));
  ZK_HIP_TRY("phase 2", hipStreamSynchronize(w.st));      // (the source is the caller's stack)
  return ZKHIP_OK;
}

int dev_scale(Phase2Dev& w, const uint64_t* in, size_t n, int n_digits, bool endo, size_t chunk, uint64_t* out, double* longest_ms, double* sum_ms) {
  char* errbuf = t_err;
  const size_t errlen = sizeof t_err;
  if (n == 0) return ZKHIP_OK;
  const size_t cap = n < chunk ? n : chunk;
  ZK_HIP_TRY("phase 2", w.d_in.reserve(cap * 24));
  ZK_HIP_TRY("phase 2", w.d_out.reserve(cap * 24));
  size_t launches = 0;
  int rc = for_each_chunk(n, chunk, [&](size_t lo, size_t m) -> int {
    while (w.ev.size() < 2 * (launches + 1)) {
      hipEvent_t e;
      ZK_HIP_TRY("phase 2", hipEventCreate(&e));
      w.ev.push_back(e);
    }
    ZK_HIP_TRY("phase 2", hipMemcpyAsync(w.d_in.get(), in + lo * 24, m * 192, hipMemcpyHostToDevice, w.st));
    ZK_HIP_TRY("phase 2", hipEventRecord(w.ev[2 * launches], w.st));
    launch_form(endo, blocks_for(m, 64), w.st, w.d_in.get(), m, w.d_digits.get(), n_digits, w.d_out.get());
    ZK_HIP_TRY("phase 2", hipGetLastError());
    ZK_HIP_TRY("phase 2", hipEventRecord(w.ev[2 * launches + 1], w.st));
    ZK_HIP_TRY("phase 2", hipMemcpyAsync(out + lo * 24, w.d_out.get(), m * 192, hipMemcpyDeviceToHost, w.st));
    launches++;
    return ZKHIP_OK;
  });
  if (rc != ZKHIP_OK) { (void)hipStreamSynchronize(w.st); return rc; }
  ZK_HIP_TRY("phase 2", hipStreamSynchronize(w.st));
  for (size_t k = 0; k < launches; k++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, w.ev[2 * k], w.ev[2 * k + 1]) != hipSuccess) continue;
    *sum_ms += ms;
    if (ms > *longest_ms) *longest_ms = ms;
  }
  return ZKHIP_OK;
}

int contribute(const zkhip_keypair* before, const uint64_t* s, const uint64_t* k, const uint8_t* prev, zkhip_keypair** after,
               zkhip_phase2_contribution* rec, uint8_t* new_digest, bool device) {
  if (!before || !prev || !after || !rec || !new_digest) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (before->n_vars && before->A.empty())
    return fail(ZKHIP_ERR_ARG, "this keypair holds no query vectors (zkhip_groth16_setup_slice keeps the slice on the device): nothing to contribute to");
  if (is_infinity(before->delta_g1.data()) || is_infinity(before->delta_g2.data())) return fail(ZKHIP_ERR_ARG, "phase 2: delta at infinity");
  Secrets sec;
  double ms[8] = {0};
  const double t_all = now_ms();
  if (s) memcpy(sec.s_m, s, 48);
  else if (!draw_scalar(sec.s_m)) return fail(ZKHIP_ERR_STATE, "getrandom failed: no secret for the contribution, and no weaker generator stands in");
  if (k) memcpy(sec.k_m, k, 48);
  else if (!draw_scalar(sec.k_m)) return fail(ZKHIP_ERR_STATE, "getrandom failed: no nonce for the proof of knowledge, and no weaker generator stands in");
  sec.S = HFr::from_limbs(sec.s_m);
  sec.K = HFr::from_limbs(sec.k_m);
  if (HFr::geq_p(sec.s_m) || HFr::geq_p(sec.k_m) || sec.S.is_zero() || sec.K.is_zero())
    return fail(ZKHIP_ERR_ARG, "phase 2: s and k are non-zero scalars below r");
  sec.S.to_canonical(sec.s_can);
  sec.K.to_canonical(sec.k_can);
  sec.Sinv = sec.S.inv();
  sec.Sinv.to_canonical(sec.sinv_can);
  const bool endo = device && kernel_form() == PHASE2_FORM_ENDO;
  if (device) sec.n_digits = endo ? phase2_glv_recode(sec.sinv_can, sec.digits) : phase2_naf_recode(sec.sinv_can, sec.digits);      // (the host route reads no digits)
  if (sec.n_digits < 0) return fail(ZKHIP_ERR_STATE, "phase 2: the decomposition of s^-1 left its bound");

  std::unique_ptr<zkhip_keypair> kp;
  double t_part = now_ms();
  try {
    kp.reset(new zkhip_keypair(*before));
  } catch (const std::bad_alloc&) {
    return fail(ZKHIP_ERR_ARG, "phase 2: out of host memory for the new key");
  }
  ms[4] = now_ms() - t_part;      // the copy of the key
  t_part = now_ms();
  point_mul(before->delta_g1.data(), sec.s_can, kp->delta_g1.data());
  point_mul(before->delta_g2.data(), sec.s_can, kp->delta_g2.data());

  ms[5] = now_ms() - t_part;      // delta' in both groups
  const size_t nh = before->H.size() / 24, nl = before->L.size() / 24;
  if (device) {
    Phase2Dev w;
    int rc = scale_open(w, sec);
    const size_t chunk = key_check_chunk(chunk_hook());
    double t0 = now_ms();
    if (rc == ZKHIP_OK) rc = dev_scale(w, before->H.data(), nh, sec.n_digits, endo, chunk, kp->H.data(), &ms[0], &ms[7]);
    ms[1] = now_ms() - t0;
    t0 = now_ms();
    if (rc == ZKHIP_OK) rc = dev_scale(w, before->L.data(), nl, sec.n_digits, endo, chunk, kp->L.data(), &ms[0], &ms[7]);
    ms[2] = now_ms() - t0;
    if (rc != ZKHIP_OK) return rc;
  } else {
    double t0 = now_ms();
    host_scale(before->H.data(), nh, sec.sinv_can, kp->H.data());
    ms[1] = now_ms() - t0;
    t0 = now_ms();
    host_scale(before->L.data(), nl, sec.sinv_can, kp->L.data());
    ms[2] = now_ms() - t0;
  }

  // the record: delta', the commitment T = k delta_g1, the response z = k + c s
  t_part = now_ms();
  memcpy(rec->delta_g1, kp->delta_g1.data(), 192);
  memcpy(rec->delta_g2, kp->delta_g2.data(), 192);
  point_mul(before->delta_g1.data(), sec.k_can, rec->pok_commit);
  uint64_t c[6];
  pok_challenge(prev, before->delta_g1.data(), rec->delta_g1, rec->pok_commit, c);
  sec.cS = HFr::from_canonical(c) * sec.S;
  (sec.K + sec.cS).to_canonical(rec->pok_response);
  link_digest(prev, rec, new_digest);
  *after = kp.release();
  ms[6] = now_ms() - t_part;      // the commitment, the response and the two hashes
  ms[3] = now_ms() - t_all;
  memcpy(t_last_ms, ms, sizeof ms);
  return ZKHIP_OK;
}

// [z] delta_g1 == T + [c] delta_g1'
// (delta_g1_new: the NEW KEY's, which step 2 has checked; a record that names another one is reported under `changed`)
bool pok_holds(const uint64_t* delta_g1, const uint64_t* delta_g1_new, const zkhip_phase2_contribution* rec, const uint8_t prev[32]) {
  if (HFr::geq_p(rec->pok_response)) return false;
  uint64_t c[6];
  pok_challenge(prev, delta_g1, delta_g1_new, rec->pok_commit, c);
  const HJac lhs = jac_from_limbs(delta_g1).mul_canonical(rec->pok_response, 6);
  const HJac rhs = jac_from_limbs(rec->pok_commit).add(jac_from_limbs(delta_g1_new).mul_canonical(c, 6));
  if (lhs.is_inf() || rhs.is_inf()) return lhs.is_inf() && rhs.is_inf();
  uint64_t a[24], b[24];
  jac_to_limbs(lhs, a);
  jac_to_limbs(rhs, b);
  return memcmp(a, b, 192) == 0;
}

// S = sum rho_i (H | L)_i: the two vectors' sums, added on the host
int combination(const zkhip_crs_desc* d, const uint64_t* rho, const std::vector<uint64_t>& wide_h, const std::vector<uint64_t>& wide_l, bool device,
                uint64_t out[24]) {
  const size_t nh = d->domain_size - 1, nl = d->n_vars - d->n_primary - 1;
  uint64_t sh[24] = {0}, sl[24] = {0};
  if (device) {
    int rc;
    if (nh && (rc = dev_combination(d->h_query, wide_h, nh, sh)) != ZKHIP_OK) return rc;
    if (nl && (rc = dev_combination(d->l_query, wide_l, nl, sl)) != ZKHIP_OK) return rc;
  } else {
    if (nh) host_combination(d->h_query, rho, nh, sh);
    if (nl) host_combination(d->l_query, rho + nh * 2, nl, sl);
  }
  HJac s = HJac::infinity();
  if (!is_infinity(sh)) s = s.add(jac_from_limbs(sh));
  if (!is_infinity(sl)) s = s.add(jac_from_limbs(sl));
  if (s.is_inf()) memset(out, 0, 192);
  else jac_to_limbs(s, out);
  return ZKHIP_OK;
}

int verify(const zkhip_crs_desc* b, const zkhip_crs_desc* a, const zkhip_phase2_contribution* rec, const uint8_t* prev, const uint64_t* rho,
           zkhip_phase2_report* out, uint8_t* new_digest, bool device) {
  if (!b || !a || !rec || !prev || !out || !new_digest) return fail(ZKHIP_ERR_ARG, "null pointer");
  int rc;
  if ((rc = check_desc(b)) != ZKHIP_OK || (rc = check_desc(a)) != ZKHIP_OK) return rc;
  const size_t m = b->n_vars, nh = b->domain_size - 1, nl = b->n_vars - b->n_primary - 1;
  if (rho)
    for (size_t i = 0; i < nh + nl; i++) if ((rho[i * 2] | rho[i * 2 + 1]) == 0) return fail(ZKHIP_ERR_ARG, "a combination scalar is zero");
  memset(out, 0, sizeof *out);
  zkhip_key_element_report* reps[5] = {&out->delta_g1, &out->delta_g2, &out->h, &out->l, &out->pok_commit};
  for (auto* r : reps) r->first_refused = (size_t)-1;
  out->infinity_mismatch_first = (size_t)-1;
  double ms[8] = {0};
  const double t_all = now_ms();

  // 1. unchanged
  if (a->n_vars != b->n_vars || a->n_primary != b->n_primary || a->domain_size != b->domain_size) {
    out->changed = (int)(1u << 31);        // nothing else can be compared index by index: the report ends here
    memcpy(t_last_ms, ms, sizeof ms);
    return ZKHIP_OK;
  }
  double t0 = now_ms();
  auto differs = [&](int bit, const uint64_t* x, const uint64_t* y, size_t n) { if (n && memcmp(x, y, n * 192) != 0) out->changed |= 1 << bit; };
  differs(ZKHIP_KEY_ALPHA_G1, b->alpha_g1, a->alpha_g1, 1);
  differs(ZKHIP_KEY_BETA_G1, b->beta_g1, a->beta_g1, 1);
  differs(ZKHIP_KEY_BETA_G2, b->beta_g2, a->beta_g2, 1);
  differs(ZKHIP_KEY_A, b->a_query, a->a_query, m);
  differs(ZKHIP_KEY_B_G2, b->b_g2_query, a->b_g2_query, m);
  differs(ZKHIP_KEY_B_G1, b->b_g1_query, a->b_g1_query, m);
  differs(ZKHIP_KEY_DELTA_G1, rec->delta_g1, a->delta_g1, 1);      // the record's delta' is the new key's
  differs(ZKHIP_KEY_DELTA_G2, rec->delta_g2, a->delta_g2, 1);
  ms[1] = now_ms() - t0;

  // 2. points
  const Element el[5] = {{a->delta_g1, 1, false}, {a->delta_g2, 1, true}, {a->h_query, nh, false}, {a->l_query, nl, false}, {rec->pok_commit, 1, false}};
  t0 = now_ms();
  if (device) {
    KeyCheckDev w;
    if ((rc = dev_open(w)) != ZKHIP_OK) return rc;
    const size_t chunk = key_check_chunk(chunk_hook());
    for (int k = 0; k < 5; k++)
      if ((rc = dev_check_element(w, el[k], chunk, reps[k], &ms[0])) != ZKHIP_OK) return rc;
  } else {
    for (int k = 0; k < 5; k++) host_check_element(el[k], reps[k]);
  }
  ms[4] = now_ms() - t0;
  auto clean = [&](int k) { return reps[k]->first_refused == (size_t)-1; };
  auto finite = [&](int k) { return reps[k]->infinity == 0; };
  t0 = now_ms();
  for (size_t i = 0; i < nh && !out->infinity_mismatch; i++)
    if (is_infinity(b->h_query + i * 24) != is_infinity(a->h_query + i * 24)) { out->infinity_mismatch = ZKHIP_KEY_H; out->infinity_mismatch_first = i; }
  for (size_t i = 0; i < nl && !out->infinity_mismatch; i++)
    if (is_infinity(b->l_query + i * 24) != is_infinity(a->l_query + i * 24)) { out->infinity_mismatch = ZKHIP_KEY_L; out->infinity_mismatch_first = i; }
  ms[2] = now_ms() - t0;
  bool points_ok = !out->infinity_mismatch && finite(0) && finite(1) && finite(4);
  for (int k = 0; k < 5; k++) points_ok = points_ok && clean(k);

  // 3 - 5. relations
  const bool eval_pair = clean(0) && clean(1) && finite(0) && finite(1);
  const bool eval_ratio = points_ok;
  const bool eval_pok = clean(0) && clean(4) && finite(0) && finite(4);
  uint64_t s_old[24], s_new[24], neg_old[24];
  if (eval_ratio) {
    std::vector<uint64_t> own;
    if (!rho) {
      own.resize((nh + nl) * 2);
      if (!draw_rho(own.data(), nh + nl)) return fail(ZKHIP_ERR_STATE, "getrandom failed: no scalars for the combination, and no weaker generator stands in");
      rho = own.data();
    }
    std::vector<uint64_t> wide_h, wide_l;      // the MSM engine's six-word scalars, one vector per base set
    if (device) {
      wide_h.assign(nh * 6, 0);
      wide_l.assign(nl * 6, 0);
      for (size_t i = 0; i < nh; i++) { wide_h[i * 6] = rho[i * 2]; wide_h[i * 6 + 1] = rho[i * 2 + 1]; }
      for (size_t i = 0; i < nl; i++) { wide_l[i * 6] = rho[(nh + i) * 2]; wide_l[i * 6 + 1] = rho[(nh + i) * 2 + 1]; }
    }
    t0 = now_ms();
    if ((rc = combination(b, rho, wide_h, wide_l, device, s_old)) != ZKHIP_OK || (rc = combination(a, rho, wide_h, wide_l, device, s_new)) != ZKHIP_OK) return rc;
    ms[5] = now_ms() - t0;
    neg_point_abi(s_old, neg_old);
  }
  t0 = now_ms();
  bool fails[3] = {false, false, false};
  {
    std::vector<std::thread> pool;
    if (eval_pair) pool.emplace_back([&] { fails[0] = !same_multiple(a->delta_g1, a->delta_g2); });
    if (eval_ratio) pool.emplace_back([&] { fails[1] = !pairing_product_is_one({s_new, neg_old}, {a->delta_g2, b->delta_g2}); });
    if (eval_pok) pool.emplace_back([&] { fails[2] = !pok_holds(b->delta_g1, a->delta_g1, rec, prev); });
    for (auto& th : pool) th.join();
  }
  const bool evaluated[3] = {eval_pair, eval_ratio, eval_pok};
  for (int k = 0; k < 3; k++) {
    if (evaluated[k]) out->relations_evaluated |= 1 << k;
    if (fails[k]) out->relations |= 1 << k;
  }
  ms[6] = now_ms() - t0;

  out->ok = (out->changed == 0 && points_ok && out->relations == 0 && out->relations_evaluated == 7) ? 1 : 0;
  if (out->ok) link_digest(prev, rec, new_digest);
  ms[3] = now_ms() - t_all;
  memcpy(t_last_ms, ms, sizeof ms);
  return ZKHIP_OK;
}

}  // namespace
#pragma GCC visibility pop

extern "C" {

int zkhip_keypair_contribute(const zkhip_keypair* before, const uint64_t s[6], const uint64_t k[6], const uint8_t prev_digest[32], zkhip_keypair** after,
                             zkhip_phase2_contribution* rec, uint8_t new_digest[32]) {
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called (zkhip_keypair_contribute_host is the route without a device)");
  BIND_CUR();
  return contribute(before, s, k, prev_digest, after, rec, new_digest, true);
}

int zkhip_keypair_contribute_host(const zkhip_keypair* before, const uint64_t s[6], const uint64_t k[6], const uint8_t prev_digest[32],
                                  zkhip_keypair** after, zkhip_phase2_contribution* rec, uint8_t new_digest[32]) {
  return contribute(before, s, k, prev_digest, after, rec, new_digest, false);
}

int zkhip_phase2_verify(const zkhip_crs_desc* before, const zkhip_crs_desc* after, const zkhip_phase2_contribution* rec, const uint8_t prev_digest[32],
                        const uint64_t* rho, zkhip_phase2_report* out, uint8_t new_digest[32]) {
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called (zkhip_phase2_verify_host is the route without a device)");
  BIND_CUR();
  return verify(before, after, rec, prev_digest, rho, out, new_digest, true);
}

int zkhip_phase2_verify_host(const zkhip_crs_desc* before, const zkhip_crs_desc* after, const zkhip_phase2_contribution* rec, const uint8_t prev_digest[32],
                             const uint64_t* rho, zkhip_phase2_report* out, uint8_t new_digest[32]) {
  return verify(before, after, rec, prev_digest, rho, out, new_digest, false);
}

int zkhip_internal_phase2_set_form(int form) {
  if (form < PHASE2_FORM_DEFAULT || form > PHASE2_FORM_ENDO) return fail(ZKHIP_ERR_ARG, "phase 2: form is 0 (default), 1 (baseline) or 2 (endomorphism)");
#ifndef ZKHIP_PHASE2_BOTH_FORMS
  if (form == PHASE2_FORM_BASELINE) return fail(ZKHIP_ERR_STATE, "phase 2: the baseline kernel is not in this build (-DZKHIP_PHASE2_BOTH_FORMS)");
#endif
  g_form.store(form);
  return ZKHIP_OK;
}

int zkhip_internal_phase2_last_ms(double out_ms[8]) {
  if (!out_ms) return fail(ZKHIP_ERR_ARG, "null pointer");
  memcpy(out_ms, t_last_ms, sizeof t_last_ms);
  return ZKHIP_OK;
}

}  // extern "C"
