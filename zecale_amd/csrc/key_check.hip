// C ABI (include/zkhip.h): the key check - zkhip_crs_check on the device, zkhip_crs_check_host on the host alone.
//
// THE CUT.  A proving key is five single points and five query vectors of up to 2^22 points (plus the verification key's ABC); what
// costs is [r] P for every one of them, 377 doublings and 135 additions of complete XYZZ formulas = 5.1 k Fq products per point
// (pairing.cuh point_check, the lane body of the checked verifier, unchanged).  One lane per point of a staged chunk of ONE element, so
// a launch holds one kind of point and every lane walks the same bits of r: the only divergence is a lane that leaves at its first
// failure.  k_key_point_check has no LDS and no barrier; it reads the raw ABI limbs with 16-byte loads and writes one byte per point.
// k_key_codes_reduce folds a chunk's bytes into five counters and the smallest refused index (atomicMin on one word that carries the
// code in its two low bits), accumulated over the chunks of the element on the device: the host waits ONCE per element.
// The pair relations are three pairing products of two pairs each on the host (pairing_host.hpp); the B relation's two sums are MSMs
// over plain base sets (the existing engine, canonical 128-bit scalars zero-extended) or, on the host route, scalar multiplications.
// The structure check is a host loop over column occupancy (the rule of api_key.hip setup_scalars, stated in zkhip.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "api_internal.hpp"
#include "device_buffer.hpp"
#include "domain.hpp"
#include "ec.cuh"
#include "key_check_internal.hpp"
#include "pairing.cuh"
#include "pairing_host.hpp"

using namespace zkhip::api;

namespace zkhip {

constexpr uint8_t KEY_CODE_INFINITY = 0x80;       // k_key_point_check's byte for a point that passes as the point at infinity
constexpr uint32_t KEY_FIRST_NONE = 0xFFFFFFFFu;  // no refused point: above every (index << 2 | code - 2), index < 2^30

// ---- encoding, curve and order of `n` points of one element (pts: n x 24 raw ABI limbs, 16-byte aligned), one lane per point
__global__ void __launch_bounds__(64) k_key_point_check(const uint64_t* __restrict__ pts, size_t n, int g2, const uint64_t* __restrict__ r_order,
                                                        uint8_t* __restrict__ codes) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const ulonglong2* src = reinterpret_cast<const ulonglong2*>(pts + t * 24);
  uint64_t p[24];
  uint64_t nz = 0;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const ulonglong2 v = src[k];
    p[2 * k] = v.x;
    p[2 * k + 1] = v.y;
    nz |= v.x | v.y;
  }
  const int code = point_check(p, g2 != 0, r_order);
  codes[t] = (uint8_t)(code == ZKHIP_VERIFY_ACCEPT && nz == 0 ? KEY_CODE_INFINITY : code);
}

// ---- a chunk's codes -> the element's counters.  base: the index of the chunk's first point in its element (< 2^30 with n).
__global__ void __launch_bounds__(256) k_key_codes_reduce(const uint8_t* __restrict__ codes, size_t n, uint32_t base, KeyCheckCounters* __restrict__ out) {
  __shared__ unsigned int s_cnt[256][4];
  __shared__ uint32_t s_first[256];
  unsigned int cnt[4] = {0, 0, 0, 0};      // infinity, ENCODING, OFF_CURVE, NOT_ORDER_R
  uint32_t first = KEY_FIRST_NONE;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t c = codes[i];
    if (c == KEY_CODE_INFINITY) cnt[0]++;
    else if (c >= ZKHIP_VERIFY_ENCODING && c <= ZKHIP_VERIFY_NOT_ORDER_R) {
      cnt[c - ZKHIP_VERIFY_ENCODING + 1]++;
      const uint32_t w = ((base + (uint32_t)i) << 2) | (uint32_t)(c - ZKHIP_VERIFY_ENCODING);
      first = w < first ? w : first;
    }
  }
  for (int k = 0; k < 4; k++) s_cnt[threadIdx.x][k] = cnt[k];
  s_first[threadIdx.x] = first;
  __syncthreads();
  for (unsigned int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      for (int k = 0; k < 4; k++) s_cnt[threadIdx.x][k] += s_cnt[threadIdx.x + s][k];
      const uint32_t o = s_first[threadIdx.x + s];
      if (o < s_first[threadIdx.x]) s_first[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (s_cnt[0][0]) atomicAdd(&out->infinity, (unsigned long long)s_cnt[0][0]);
    for (int k = 0; k < 3; k++) if (s_cnt[0][k + 1]) atomicAdd(&out->refused[k], (unsigned long long)s_cnt[0][k + 1]);
    if (blockIdx.x == 0) atomicAdd(&out->points, (unsigned long long)n);
    if (s_first[0] != KEY_FIRST_NONE) atomicMin(&out->first, s_first[0]);
  }
}

}  // namespace zkhip

#pragma GCC visibility push(hidden)      // this file's own helpers, and those phase2.hip shares (key_check_internal.hpp)
namespace zkhip {
namespace keycheck {

using namespace zkhip::host;

static std::atomic<size_t> g_chunk_hook{0};                 // zkhip_internal_key_check_set_chunk
static thread_local double t_last_ms[4 + ZKHIP_KEY_ELEMENTS] = {0};     // zkhip_internal_key_check_last_ms

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
size_t chunk_hook() { return g_chunk_hook.load(); }

void key_elements(const zkhip_crs_desc* d, const uint64_t* vk_abc, Element e[ZKHIP_KEY_ELEMENTS]) {
  const size_t m = d->n_vars, l = d->n_primary;
  e[ZKHIP_KEY_ALPHA_G1] = {d->alpha_g1, 1, false};
  e[ZKHIP_KEY_BETA_G1] = {d->beta_g1, 1, false};
  e[ZKHIP_KEY_BETA_G2] = {d->beta_g2, 1, true};
  e[ZKHIP_KEY_DELTA_G1] = {d->delta_g1, 1, false};
  e[ZKHIP_KEY_DELTA_G2] = {d->delta_g2, 1, true};
  e[ZKHIP_KEY_A] = {d->a_query, m, false};
  e[ZKHIP_KEY_B_G2] = {d->b_g2_query, m, true};
  e[ZKHIP_KEY_B_G1] = {d->b_g1_query, m, false};
  e[ZKHIP_KEY_H] = {d->h_query, d->domain_size - 1, false};
  e[ZKHIP_KEY_L] = {d->l_query, m - l - 1, false};
  e[ZKHIP_KEY_VK_ABC] = {vk_abc, vk_abc ? l + 1 : 0, false};
}

int check_args(const zkhip_crs_desc* d, const zkhip_r1cs_desc* cs, const uint64_t* rho, zkhip_key_report* out) {
  if (!d || !out || !d->alpha_g1 || !d->beta_g1 || !d->beta_g2 || !d->delta_g1 || !d->delta_g2) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (d->n_vars < d->n_primary + 1 || d->domain_size < 1 || !is_valid_domain(d->domain_size)) return fail(ZKHIP_ERR_ARG, "key check: implausible sizes");
  if (d->n_vars >= ((size_t)1 << 30) || d->domain_size >= ((size_t)1 << 30)) return fail(ZKHIP_ERR_ARG, "key check: a vector of 2^30 points or more");
  if (!d->a_query || !d->b_g2_query || !d->b_g1_query) return fail(ZKHIP_ERR_ARG, "null pointer");
  if ((d->domain_size > 1 && !d->h_query) || (d->n_vars > d->n_primary + 1 && !d->l_query)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (cs && (!cs->a_row_ptr || !cs->b_row_ptr || !cs->c_row_ptr)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (rho)
    for (size_t i = 0; i < d->n_vars; i++) if ((rho[i * 2] | rho[i * 2 + 1]) == 0) return fail(ZKHIP_ERR_ARG, "a combination scalar is zero");
  return ZKHIP_OK;
}

bool is_infinity(const uint64_t* p) {
  uint64_t nz = 0;
  for (int k = 0; k < 24; k++) nz |= p[k];
  return nz == 0;
}

// ---- the point checks of one element on the host (pairing_host.hpp point_check_host), the points dealt to up to 16 threads
void host_check_element(const Element& el, zkhip_key_element_report* rep) {
  std::vector<uint8_t> codes(el.n);
  unsigned threads = std::thread::hardware_concurrency();
  if (threads > 16) threads = 16;
  if (threads < 1 || el.n < 32) threads = 1;
  auto work = [&](unsigned t) { for (size_t i = t; i < el.n; i += threads) codes[i] = (uint8_t)point_check_host(el.p + i * 24, el.g2); };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  rep->points = el.n;
  for (size_t i = 0; i < el.n; i++) {
    if (!codes[i]) { if (is_infinity(el.p + i * 24)) rep->infinity++; continue; }
    rep->refused[codes[i] - ZKHIP_VERIFY_ENCODING]++;
    if (rep->first_refused == (size_t)-1) { rep->first_refused = i; rep->first_code = codes[i]; }
  }
}

// ---- the same on the device: the element's points staged chunk by chunk, one wait per element
int dev_open(KeyCheckDev& w) {
  char* errbuf = t_err;
  const size_t errlen = sizeof t_err;
  ZK_HIP_TRY("key check", w.st.create());
  ZK_HIP_TRY("key check", w.d_r.reserve(6));
  ZK_HIP_TRY("key check", w.d_cnt.reserve(1));
  ZK_HIP_TRY("key check", hipMemcpyAsync(w.d_r.get(), FqParams::R_ORDER64, 48, hipMemcpyHostToDevice, w.st));
  return ZKHIP_OK;
}

int dev_check_element(KeyCheckDev& w, const Element& el, size_t chunk, zkhip_key_element_report* rep, double* longest_ms) {
  char* errbuf = t_err;
  const size_t errlen = sizeof t_err;
  rep->points = el.n;
  if (el.n == 0) return ZKHIP_OK;
  const size_t cap = el.n < chunk ? el.n : chunk;
  ZK_HIP_TRY("key check", w.d_pts.reserve(cap * 24));
  ZK_HIP_TRY("key check", w.d_codes.reserve(cap));
  KeyCheckCounters cnt = {};
  cnt.first = KEY_FIRST_NONE;
  ZK_HIP_TRY("key check", hipMemcpyAsync(w.d_cnt.get(), &cnt, sizeof cnt, hipMemcpyHostToDevice, w.st));
  size_t launches = 0;
  int rc = for_each_chunk(el.n, chunk, [&](size_t lo, size_t m) -> int {
    while (w.ev.size() < 2 * (launches + 1)) {
      hipEvent_t e;
      ZK_HIP_TRY("key check", hipEventCreate(&e));
      w.ev.push_back(e);
    }
    ZK_HIP_TRY("key check", hipMemcpyAsync(w.d_pts.get(), el.p + lo * 24, m * 192, hipMemcpyHostToDevice, w.st));
    ZK_HIP_TRY("key check", hipEventRecord(w.ev[2 * launches], w.st));
    hipLaunchKernelGGL(k_key_point_check, dim3(blocks_for(m, 64)), dim3(64), 0, w.st, w.d_pts.get(), m, el.g2 ? 1 : 0, w.d_r.get(), w.d_codes.get());
    ZK_HIP_TRY("key check", hipGetLastError());
    ZK_HIP_TRY("key check", hipEventRecord(w.ev[2 * launches + 1], w.st));
    const unsigned blocks = blocks_for(m, 256) < 64 ? blocks_for(m, 256) : 64;
    hipLaunchKernelGGL(k_key_codes_reduce, dim3(blocks), dim3(256), 0, w.st, w.d_codes.get(), m, (uint32_t)lo, w.d_cnt.get());
    ZK_HIP_TRY("key check", hipGetLastError());
    launches++;
    return ZKHIP_OK;
  });
  if (rc != ZKHIP_OK) { (void)hipStreamSynchronize(w.st); return rc; }
  ZK_HIP_TRY("key check", hipMemcpyAsync(&cnt, w.d_cnt.get(), sizeof cnt, hipMemcpyDeviceToHost, w.st));
  ZK_HIP_TRY("key check", hipStreamSynchronize(w.st));
  for (size_t k = 0; k < launches; k++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, w.ev[2 * k], w.ev[2 * k + 1]) == hipSuccess && ms > *longest_ms) *longest_ms = ms;
  }
  if (cnt.points != el.n) return fail(ZKHIP_ERR_HIP, "key check: the device counted other points than the element has");
  rep->infinity = (size_t)cnt.infinity;
  for (int k = 0; k < 3; k++) rep->refused[k] = (size_t)cnt.refused[k];
  if (cnt.first != KEY_FIRST_NONE) {
    rep->first_refused = cnt.first >> 2;
    rep->first_code = (int)(cnt.first & 3u) + ZKHIP_VERIFY_ENCODING;
  }
  return ZKHIP_OK;
}

// ---- pairs.  t(P1, g2) t(-g1, P2) == 1: P1 and P2 are the same multiple of their generators
bool same_multiple(const uint64_t* p1, const uint64_t* p2) {
  uint64_t g1[24], g2[24], neg_g1[24];
  memcpy(g1, FqParams::G1_GEN_X64, 96); memcpy(g1 + 12, FqParams::G1_GEN_Y64, 96);
  memcpy(g2, FqParams::G2_GEN_X64, 96); memcpy(g2 + 12, FqParams::G2_GEN_Y64, 96);
  neg_point_abi(g1, neg_g1);
  // (a pair with a member at infinity contributes one: infinity on one side only leaves the other side's pairing, which is not one)
  return pairing_product_is_one({p1, neg_g1}, {g2, p2});
}

// S = sum rho_i P_i on the host, the terms dealt to up to 16 threads
void host_combination(const uint64_t* pts, const uint64_t* rho, size_t n, uint64_t out[24]) {
  unsigned threads = std::thread::hardware_concurrency();
  if (threads > 16) threads = 16;
  if (threads < 1 || n < 32) threads = 1;
  std::vector<HJac> part(threads, HJac::infinity());
  auto work = [&](unsigned t) {
    for (size_t i = t; i < n; i += threads) {
      if (is_infinity(pts + i * 24)) continue;
      part[t] = part[t].add(jac_from_limbs(pts + i * 24).mul_canonical(rho + i * 2, 2));
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  HJac s = HJac::infinity();
  for (unsigned t = 0; t < threads; t++) s = s.add(part[t]);
  if (s.is_inf()) memset(out, 0, 192);
  else jac_to_limbs(s, out);
}

// the same through the MSM engine: a plain base set, canonical scalars zero-extended to six words
int dev_combination(const uint64_t* pts, const std::vector<uint64_t>& scalars, size_t n, uint64_t out[24]) {
  zkhip_bases* b = nullptr;
  int rc = zkhip_bases_upload(pts, n, &b);
  if (rc != ZKHIP_OK) return rc;
  uint64_t jac[36];
  rc = zkhip_msm(b, 0, scalars.data(), n, 0, jac);
  zkhip_bases_free(b);
  if (rc != ZKHIP_OK) return rc;
  const HFq Z = HFq::from_limbs(jac + 24);
  if (Z.is_zero()) { memset(out, 0, 192); return ZKHIP_OK; }
  return zkhip_jac_to_affine(jac, out);
}

// ---- structure: lengths, and a base at infinity exactly where the setup's polynomial is identically zero (zkhip.h states the rule;
// api_key.hip setup_scalars is where it comes from: At gets the input-consistency rows for variables 0 .. l, L is beta A + alpha B + C)
void check_structure(const zkhip_crs_desc* d, const uint64_t* vk_abc, const zkhip_r1cs_desc* cs, zkhip_key_report* out) {
  auto disagree = [&](int element, size_t index) { if (!out->structure) { out->structure = element; out->structure_first = index; } };
  const size_t m = cs->n_vars, l = cs->n_primary, n = cs->n_constraints;
  if (d->n_vars != m) disagree(ZKHIP_KEY_A, (size_t)-1);
  if (d->n_primary != l) disagree(ZKHIP_KEY_L, (size_t)-1);
  if (d->domain_size < n + l + 1) disagree(ZKHIP_KEY_H, (size_t)-1);
  if (out->structure) return;
  std::vector<uint8_t> occ(m, 0);        // bit 0: column of A holds a non-zero coefficient, bit 1: of B, bit 2: of C
  auto occupancy = [&](const uint32_t* rp, const uint32_t* col, const uint64_t* val, uint8_t bit) {
    for (uint32_t k = 0; k < rp[n]; k++) {
      uint64_t nz = 0;
      for (int j = 0; j < 6; j++) nz |= val[(size_t)k * 6 + j];
      if (nz && col[k] < m) occ[col[k]] |= bit;
    }
  };
  occupancy(cs->a_row_ptr, cs->a_col, cs->a_val, 1);
  occupancy(cs->b_row_ptr, cs->b_col, cs->b_val, 2);
  occupancy(cs->c_row_ptr, cs->c_col, cs->c_val, 4);
  // in report order: A, B-G2, B-G1, H, L, vk_abc - the first element that disagrees is reported, at its first index
  for (size_t i = 0; i < m && !out->structure; i++)
    if (is_infinity(d->a_query + i * 24) != (i > l && !(occ[i] & 1))) disagree(ZKHIP_KEY_A, i);
  for (size_t i = 0; i < m && !out->structure; i++)
    if (is_infinity(d->b_g2_query + i * 24) != !(occ[i] & 2)) disagree(ZKHIP_KEY_B_G2, i);
  for (size_t i = 0; i < m && !out->structure; i++)
    if (is_infinity(d->b_g1_query + i * 24) != !(occ[i] & 2)) disagree(ZKHIP_KEY_B_G1, i);
  for (size_t i = 0; i + 1 < d->domain_size && !out->structure; i++)
    if (is_infinity(d->h_query + i * 24)) disagree(ZKHIP_KEY_H, i);
  for (size_t i = l + 1; i < m && !out->structure; i++)
    if (is_infinity(d->l_query + (i - l - 1) * 24) != (occ[i] == 0)) disagree(ZKHIP_KEY_L, i - l - 1);
  for (size_t i = 0; vk_abc && i <= l && !out->structure; i++)
    if (is_infinity(vk_abc + i * 24)) disagree(ZKHIP_KEY_VK_ABC, i);
}

int crs_check(const zkhip_crs_desc* d, const uint64_t* vk_abc, const zkhip_r1cs_desc* cs, const uint64_t* rho, zkhip_key_report* out, bool device) {
  int rc = check_args(d, cs, rho, out);
  if (rc != ZKHIP_OK) return rc;
  memset(out, 0, sizeof *out);
  for (auto& e : out->e) e.first_refused = (size_t)-1;
  out->b_infinity_mismatch = out->structure_first = (size_t)-1;
  Element el[ZKHIP_KEY_ELEMENTS];
  key_elements(d, vk_abc, el);
  double ms[4 + ZKHIP_KEY_ELEMENTS] = {0};      // zkhip_internal_key_check_last_ms

  // 1. points
  double t0 = now_ms();
  if (device) {
    KeyCheckDev w;
    if ((rc = dev_open(w)) != ZKHIP_OK) return rc;
    const size_t chunk = key_check_chunk(g_chunk_hook.load());
    for (int k = 0; k < ZKHIP_KEY_ELEMENTS; k++) {
      const double te = now_ms();
      if ((rc = dev_check_element(w, el[k], chunk, &out->e[k], &ms[0])) != ZKHIP_OK) return rc;
      ms[4 + k] = now_ms() - te;
    }
  } else {
    for (int k = 0; k < ZKHIP_KEY_ELEMENTS; k++) {
      const double te = now_ms();
      host_check_element(el[k], &out->e[k]);
      ms[4 + k] = now_ms() - te;
    }
  }
  ms[1] = now_ms() - t0;
  auto clean = [&](int k) { return out->e[k].first_refused == (size_t)-1; };

  // 2. pairs
  for (size_t i = 0; i < d->n_vars; i++)
    if (is_infinity(d->b_g1_query + i * 24) != is_infinity(d->b_g2_query + i * 24)) { out->b_infinity_mismatch = i; break; }
  uint64_t s1[24], s2[24];
  const bool b_clean = clean(ZKHIP_KEY_B_G1) && clean(ZKHIP_KEY_B_G2);
  if (b_clean) {
    std::vector<uint64_t> own;
    if (!rho) {
      own.resize(d->n_vars * 2);
      if (!draw_rho(own.data(), d->n_vars)) return fail(ZKHIP_ERR_STATE, "getrandom failed: no scalars for the combination, and no weaker generator stands in");
      rho = own.data();
    }
    t0 = now_ms();
    if (device) {
      std::vector<uint64_t> wide(d->n_vars * 6, 0);
      for (size_t i = 0; i < d->n_vars; i++) { wide[i * 6] = rho[i * 2]; wide[i * 6 + 1] = rho[i * 2 + 1]; }
      if ((rc = dev_combination(d->b_g1_query, wide, d->n_vars, s1)) != ZKHIP_OK || (rc = dev_combination(d->b_g2_query, wide, d->n_vars, s2)) != ZKHIP_OK)
        return rc;
    } else {
      host_combination(d->b_g1_query, rho, d->n_vars, s1);
      host_combination(d->b_g2_query, rho, d->n_vars, s2);
    }
    ms[2] = now_ms() - t0;
  }
  t0 = now_ms();
  struct { int bit; bool evaluated; const uint64_t *p1, *p2; } rel[3] = {
      {1, clean(ZKHIP_KEY_BETA_G1) && clean(ZKHIP_KEY_BETA_G2), d->beta_g1, d->beta_g2},
      {2, clean(ZKHIP_KEY_DELTA_G1) && clean(ZKHIP_KEY_DELTA_G2), d->delta_g1, d->delta_g2},
      {4, b_clean, s1, s2}};
  bool fails[3] = {false, false, false};
  {
    std::vector<std::thread> pool;
    for (int k = 0; k < 3; k++)
      if (rel[k].evaluated) pool.emplace_back([&, k] { fails[k] = !same_multiple(rel[k].p1, rel[k].p2); });
    for (auto& th : pool) th.join();
  }
  for (int k = 0; k < 3; k++) {
    if (rel[k].evaluated) out->pairs_evaluated |= rel[k].bit;
    if (fails[k]) out->pairs |= rel[k].bit;
  }
  ms[3] = now_ms() - t0;

  // 3. structure
  if (cs) check_structure(d, vk_abc, cs, out);

  bool ok = out->pairs == 0 && out->pairs_evaluated == 7 && out->b_infinity_mismatch == (size_t)-1 && out->structure == 0;
  for (int k = 0; k < ZKHIP_KEY_ELEMENTS; k++) ok = ok && clean(k);
  out->ok = ok ? 1 : 0;
  memcpy(t_last_ms, ms, sizeof ms);
  return ZKHIP_OK;
}

}  // namespace keycheck
}  // namespace zkhip
#pragma GCC visibility pop

using namespace zkhip::keycheck;

extern "C" {

int zkhip_crs_check(const zkhip_crs_desc* key, const uint64_t* vk_abc, const zkhip_r1cs_desc* cs, const uint64_t* rho, zkhip_key_report* out) {
  if (cur_dev() < 0) return fail(ZKHIP_ERR_NO_DEVICE, "zkhip_init not called (zkhip_crs_check_host is the route without a device)");
  BIND_CUR();
  return crs_check(key, vk_abc, cs, rho, out, true);
}

int zkhip_crs_check_host(const zkhip_crs_desc* key, const uint64_t* vk_abc, const zkhip_r1cs_desc* cs, const uint64_t* rho, zkhip_key_report* out) {
  return crs_check(key, vk_abc, cs, rho, out, false);
}

int zkhip_internal_key_check_set_chunk(size_t points) {
  if (points >= ((size_t)1 << 30)) return fail(ZKHIP_ERR_ARG, "key check: a chunk of 2^30 points or more");
  g_chunk_hook.store(points);
  return ZKHIP_OK;
}

int zkhip_internal_key_check_last_ms(double out_ms[4 + ZKHIP_KEY_ELEMENTS]) {
  if (!out_ms) return fail(ZKHIP_ERR_ARG, "null pointer");
  memcpy(out_ms, t_last_ms, sizeof t_last_ms);
  return ZKHIP_OK;
}

}  // extern "C"
