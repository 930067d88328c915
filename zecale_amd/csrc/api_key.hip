// C ABI (include/zkhip.h): proving keys - options, upload (whole and slice), the trusted setup, the keypair and its file.
#include <math.h>
#include <string.h>

#include "api_internal.hpp"
#include "domain.hpp"

using namespace zkhip::api;

#pragma GCC visibility push(hidden)      // this file's own helpers and handle structs

// The options of a key, resolved once at upload against the process-wide defaults (zkhip_set_*), then carried by the handle:
// two threads loading keys with different options never see each other's choice.
struct ResolvedOpts { int precompute, naf, window, batch, model; };
static ResolvedOpts resolve_opts(const zkhip_key_opts* o) {
  ResolvedOpts r;
  r.precompute = (o && o->precompute >= 0) ? (o->precompute ? 1 : 0) : g.crs_tables.load();
  r.naf = (o && o->table_naf >= 0) ? (o->table_naf ? 1 : 0) : -1;                  // -1: naf_tables_wanted() decides
  r.window = (o && o->window > 0) ? o->window : g.forced_c.load();
  r.batch = (o && o->batch_msms >= 0) ? (o->batch_msms ? 1 : 0) : g.batch_msms.load();
  r.model = (o && o->table_model == 1) ? 1 : 0;
  if (r.model && r.naf < 0) r.naf = 0;      // Edwards tables have one level per window, whatever the process-wide default says
  return r;
}
// what an upload refuses before it allocates anything (zkhip.h: the rules of zkhip_key_opts)
static int check_opts(const zkhip_key_opts* o) {
  if (!o) return ZKHIP_OK;
  if (o->window < 0 || (o->window > 0 && (o->window < 4 || o->window > 22)))
    return fail(ZKHIP_ERR_ARG, "zkhip_key_opts.window must be 0 (automatic) or in [4, 22]");
  if (o->table_model != 0 && o->table_model != 1) return fail(ZKHIP_ERR_ARG, "zkhip_key_opts.table_model must be 0 (XYZZ) or 1 (Edwards)");
  if (o->table_model == 1 && !resolve_opts(o).precompute) return fail(ZKHIP_ERR_ARG, "zkhip_key_opts.table_model = 1 needs window tables (precompute)");
  if (o->table_model == 1 && o->table_naf > 0)
    return fail(ZKHIP_ERR_ARG, "zkhip_key_opts.table_model = 1 with table_naf = 1: Edwards tables have one level per window");
  return ZKHIP_OK;
}

// one window size for the whole key (the prover's MSM contexts are shared by the five query vectors)
static int crs_build_tables(zkhip_crs* c, const ResolvedOpts& o) {
  c->batch_msms = o.batch;
  if (!o.precompute) return ZKHIP_OK;
  zkhip_bases* all[5] = {c->A, c->B2, c->B1, c->H, c->L};
  size_t total = 0, finite = 0, maxlen = 0;
  // (the window follows the longest vector's FINITE bases: a slice cut by finite terms - zkhip_key_partition - can be long and
  //  mostly infinity; a whole key's longest vector is H or L, all finite: unchanged)
  for (zkhip_bases* b : all) { total += b->len; finite += b->n_finite; if (b->n_finite > maxlen) maxlen = b->n_finite; }
  if (maxlen == 0) maxlen = c->A->len > c->H->len ? c->A->len : c->H->len;
  // one kind of table for the whole key; an explicit request for the larger kind still respects the memory guard
  const int naf = (o.naf >= 0 ? (o.naf && naf_tables_fit(total)) : naf_tables_wanted(total)) ? 1 : 0;
  int tc = o.window ? o.window : auto_table_window(maxlen);
  if (!o.window && naf && finite > 0) {
    // every-bit-position tables leave the window free of the table's layout: the five MSMs of a proof share one launch sequence,
    // so what counts is the key's FINITE bases together - additions ~ finite * 378 / (c + 2), bucket reduction ~ 5 * 2^(c-1).
    // Measured in a stream of proofs (tools/acc_probe.py --prove-stream): 176 k bases (the wrapping key) c = 14 / 15 / 16 ->
    // 363 / 372-378 / 367 proofs/s; 370 k bases (nine inputs per nested proof) c = 15 / 16 / 17 -> 182 / 192 / 190.5.
    const double copt = log2((double)finite) - 2.45;
    tc = (int)(copt + 0.5);
    if (tc < 9) tc = 9;
    if (tc > 20) tc = 20;
  }
  // the Edwards form for the four G1 vectors of a key that asks for it, never for B-G2 (its curve has no rational 2-torsion)
  const bool edw = o.model == 1 && !naf;
  for (zkhip_bases* b : all) {
    int rc = bases_precompute_mode(b, tc, naf, edw && b != c->B2);
    if (rc != ZKHIP_OK) return rc;
  }
  if (edw) {
    // all four or none: a vector that was refused (a point not of order r, the memory guard) leaves an ordinary XYZZ key
    zkhip_bases* g1[4] = {c->A, c->B1, c->H, c->L};
    bool all_edw = true, any = false;
    for (zkhip_bases* b : g1) { if (b->len && !b->d_edw) all_edw = false; if (b->d_edw) any = true; }
    if (all_edw && any) c->table_model = 1;
    else for (zkhip_bases* b : g1) if (b->d_edw) { (void)hipFree(b->d_edw); b->d_edw = nullptr; }
  }
  return ZKHIP_OK;
}

static int crs_upload_impl(const zkhip_crs_desc* d, size_t a_lo, size_t a_len, size_t h_lo, size_t h_len, size_t l_lo, size_t l_len,
                           const zkhip_key_opts* opts, zkhip_crs** out) {
  { int rc_ = check_opts(opts); if (rc_ != ZKHIP_OK) return rc_; }
  zkhip_crs* c = new zkhip_crs();
  c->device = cur_dev();
  c->n_vars = d->n_vars; c->n_primary = d->n_primary; c->domain_size = d->domain_size;
  memcpy(c->alpha_g1, d->alpha_g1, 192); memcpy(c->beta_g1, d->beta_g1, 192); memcpy(c->beta_g2, d->beta_g2, 192);
  memcpy(c->delta_g1, d->delta_g1, 192); memcpy(c->delta_g2, d->delta_g2, 192);
  int rc;
  if ((rc = zkhip_bases_upload(d->a_query + a_lo * 24, a_len, &c->A)) == ZKHIP_OK &&
      (rc = zkhip_bases_upload(d->b_g2_query + a_lo * 24, a_len, &c->B2)) == ZKHIP_OK &&
      (rc = zkhip_bases_upload(d->b_g1_query + a_lo * 24, a_len, &c->B1)) == ZKHIP_OK &&
      (rc = zkhip_bases_upload(d->h_query + h_lo * 24, h_len, &c->H)) == ZKHIP_OK &&
      (rc = zkhip_bases_upload(d->l_query + l_lo * 24, l_len, &c->L)) == ZKHIP_OK)
    rc = crs_build_tables(c, resolve_opts(opts));
  if (rc != ZKHIP_OK) { zkhip_crs_free(c); return rc; }     // frees what was uploaded so far (null members are skipped)
  *out = c;
  return ZKHIP_OK;
}

// The exponents of a key (host): QAP polynomials at tau through the Lagrange basis of the key's domain (one batch inversion), then
// the five query vectors' scalars.  Shared by the whole-key setup and the slice setup below.
namespace {
struct SetupScalars {
  size_t n = 0, m = 0, l = 0, d = 0;
  std::vector<host::HFr> At, Bt, hs, ls, abc, single;      // single: alpha, beta, delta
};
int setup_scalars(const zkhip_r1cs_desc* cs, const uint64_t tau_m[6], const uint64_t alpha_m[6], const uint64_t beta_m[6],
                  const uint64_t delta_m[6], size_t domain_size, SetupScalars& o) {
  using namespace host;
  const size_t n = cs->n_constraints, m = cs->n_vars, l = cs->n_primary;
  if (m < l + 1) return fail(ZKHIP_ERR_ARG, "bad sizes");
  // the evaluation domain (domain.hpp): 0 = the power of two libzeth's groth16_snark forces (the reference's keys), ZKHIP_DOMAIN_STEP =
  // libfqfft's unforced choice (a power of two or 2^k + 2^r), else a valid size at least n + l + 1
  const size_t d = resolve_domain(n + l + 1, domain_size);
  if (!d) return fail(ZKHIP_ERR_ARG, "setup: the evaluation domain is not a power of two or 2^k + 2^r, or smaller than n + l + 1");
  if (d > ((size_t)1 << 22)) return fail(ZKHIP_ERR_ARG, "domain larger than 2^22");
  HFr tau = HFr::from_limbs(tau_m), alpha = HFr::from_limbs(alpha_m), beta = HFr::from_limbs(beta_m), delta = HFr::from_limbs(delta_m);
  if (delta.is_zero()) return fail(ZKHIP_ERR_ARG, "delta must be invertible");
  // Lagrange basis at tau, one batch inversion
  const EvalDomain dom(d);
  const HFr Zt = dom.vanishing(tau);
  std::vector<HFr> Lg;
  if (!dom.lagrange_at(tau, Lg)) return fail(ZKHIP_ERR_ARG, "tau lies in the evaluation domain");
  o.n = n; o.m = m; o.l = l; o.d = d;
  o.At.assign(m, HFr::zero()); o.Bt.assign(m, HFr::zero());
  std::vector<HFr> Ct(m, HFr::zero());
  auto accumulate = [&](const uint32_t* rp, const uint32_t* col, const uint64_t* val, std::vector<HFr>& out_) {
    for (size_t j = 0; j < n; j++)
      for (uint32_t k = rp[j]; k < rp[j + 1]; k++) out_[col[k]] = out_[col[k]] + HFr::from_limbs(val + (size_t)k * 6) * Lg[j];
  };
  accumulate(cs->a_row_ptr, cs->a_col, cs->a_val, o.At);
  accumulate(cs->b_row_ptr, cs->b_col, cs->b_val, o.Bt);
  accumulate(cs->c_row_ptr, cs->c_col, cs->c_val, Ct);
  for (size_t k = 0; k <= l; k++) o.At[k] = o.At[k] + Lg[n + k];          // input-consistency rows
  const HFr delta_inv = delta.inv();
  o.hs.resize(d - 1); o.ls.resize(m - l - 1); o.abc.resize(l + 1); o.single.resize(3);
  HFr t = Zt * delta_inv;
  for (size_t j = 0; j + 1 < d; j++) { o.hs[j] = t; t = t * tau; }
  for (size_t i = l + 1; i < m; i++) o.ls[i - l - 1] = (beta * o.At[i] + alpha * o.Bt[i] + Ct[i]) * delta_inv;
  for (size_t i = 0; i <= l; i++) o.abc[i] = beta * o.At[i] + alpha * o.Bt[i] + Ct[i];
  o.single[0] = alpha; o.single[1] = beta; o.single[2] = delta;
  return ZKHIP_OK;
}
std::vector<uint64_t> pack_scalars(const host::HFr* v, size_t count) {
  std::vector<uint64_t> o(count * 6);
  for (size_t i = 0; i < count; i++) v[i].to_limbs(&o[i * 6]);
  return o;
}
void generators(uint64_t g1[24], uint64_t g2[24]) {
  memcpy(g1, FqParams::G1_GEN_X64, 96); memcpy(g1 + 12, FqParams::G1_GEN_Y64, 96);
  memcpy(g2, FqParams::G2_GEN_X64, 96); memcpy(g2 + 12, FqParams::G2_GEN_Y64, 96);
}
}  // namespace

// ---- keypair file (the role of wsnarkT::keypair_write_bytes / keypair_read_bytes, aggregator_server.cpp:77-94).  The
// reference's byte format is defined in the absent libzeth, so this is the library's own container: a 64-byte header
// ("ZKHIPKP1", sizes) followed by the limb arrays exactly as they cross the C ABI (Montgomery u64 limbs, little-endian),
// and a 64-bit FNV-1a checksum of everything before it.  Host code, no device needed.
namespace {
const char KP_MAGIC[8] = {'Z', 'K', 'H', 'I', 'P', 'K', 'P', '1'};
uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}
}  // namespace

#pragma GCC visibility pop

extern "C" {

int zkhip_set_crs_precompute(int on) { g.crs_tables.store(on ? 1 : 0); return ZKHIP_OK; }
int zkhip_set_batch_msms(int on) { g.batch_msms.store(on ? 1 : 0); return ZKHIP_OK; }

int zkhip_crs_upload_ex(const zkhip_crs_desc* d, const zkhip_key_opts* opts, zkhip_crs** out) {
  BIND_CUR();
  if (!d || !out || !d->alpha_g1 || !d->beta_g1 || !d->beta_g2 || !d->delta_g1 || !d->delta_g2)
    return fail(ZKHIP_ERR_ARG, "null pointer");
  if (d->n_vars < d->n_primary + 1 || d->domain_size < 1) return fail(ZKHIP_ERR_ARG, "bad sizes");
  if (!host::is_valid_domain(d->domain_size)) return fail(ZKHIP_ERR_ARG, "proving key: domain_size is neither a power of two nor 2^k + 2^r");
  return crs_upload_impl(d, 0, d->n_vars, 0, d->domain_size - 1, 0, d->n_vars - d->n_primary - 1, opts, out);
}
int zkhip_crs_upload(const zkhip_crs_desc* d, zkhip_crs** out) { return zkhip_crs_upload_ex(d, nullptr, out); }

int zkhip_crs_upload_slice_ex(const zkhip_crs_desc* d, size_t a_lo, size_t a_len, size_t h_lo, size_t h_len, size_t l_lo, size_t l_len,
                              const zkhip_key_opts* opts, zkhip_crs** out) {
  BIND_CUR();
  if (!d || !out || !d->alpha_g1 || !d->beta_g1 || !d->beta_g2 || !d->delta_g1 || !d->delta_g2) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (d->n_vars < d->n_primary + 1 || d->domain_size < 1) return fail(ZKHIP_ERR_ARG, "bad sizes");
  if (!host::is_valid_domain(d->domain_size)) return fail(ZKHIP_ERR_ARG, "proving key: domain_size is neither a power of two nor 2^k + 2^r");
  if (a_lo + a_len > d->n_vars || h_lo + h_len > d->domain_size - 1 || l_lo + l_len > d->n_vars - d->n_primary - 1)
    return fail(ZKHIP_ERR_ARG, "slice out of range");
  return crs_upload_impl(d, a_lo, a_len, h_lo, h_len, l_lo, l_len, opts, out);
}
int zkhip_crs_upload_slice(const zkhip_crs_desc* d, size_t a_lo, size_t a_len, size_t h_lo, size_t h_len, size_t l_lo, size_t l_len,
                           zkhip_crs** out) {
  return zkhip_crs_upload_slice_ex(d, a_lo, a_len, h_lo, h_len, l_lo, l_len, nullptr, out);
}

int zkhip_crs_table_window(const zkhip_crs* c) { return (c && c->A) ? c->A->table_c : 0; }
int zkhip_crs_device(const zkhip_crs* c) { return c ? c->device : -1; }
int zkhip_crs_table_kind(const zkhip_crs* c) { return (c && c->A && c->A->table_c) ? (c->A->table_naf ? 2 : 1) : 0; }
int zkhip_crs_table_model(const zkhip_crs* c) { return c ? c->table_model : 0; }
int zkhip_crs_finite_terms(const zkhip_crs* c, size_t out[5]) {
  if (!c || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  const zkhip_bases* all[5] = {c->A, c->B2, c->B1, c->H, c->L};
  for (int k = 0; k < 5; k++) out[k] = all[k] ? all[k]->n_finite : 0;
  return ZKHIP_OK;
}

void zkhip_crs_free(zkhip_crs* c) {
  if (!c) return;
  (void)bind_dev(c->device);
  zkhip_bases_free(c->A); zkhip_bases_free(c->B2); zkhip_bases_free(c->B1); zkhip_bases_free(c->H); zkhip_bases_free(c->L);
  delete c;
}

int zkhip_groth16_setup(const zkhip_r1cs_desc* cs, const uint64_t tau_m[6], const uint64_t alpha_m[6], const uint64_t beta_m[6],
                        const uint64_t delta_m[6], zkhip_keypair** out) {
  return zkhip_groth16_setup_ex(cs, tau_m, alpha_m, beta_m, delta_m, 0, out);     // the reference's forced power-of-two domain
}

int zkhip_groth16_setup_ex(const zkhip_r1cs_desc* cs, const uint64_t tau_m[6], const uint64_t alpha_m[6], const uint64_t beta_m[6],
                           const uint64_t delta_m[6], size_t domain_size, zkhip_keypair** out) {
  using namespace host;
  BIND_CUR();
  if (!cs || !tau_m || !alpha_m || !beta_m || !delta_m || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  SetupScalars sc;
  int rc = setup_scalars(cs, tau_m, alpha_m, beta_m, delta_m, domain_size, sc);
  if (rc != ZKHIP_OK) return rc;
  uint64_t g1[24], g2[24];
  generators(g1, g2);
  zkhip_keypair* kp = new zkhip_keypair();
  kp->n_vars = sc.m; kp->n_primary = sc.l; kp->domain_size = sc.d;
  auto fb = [&](const uint64_t* base, const std::vector<HFr>& v, std::vector<uint64_t>& dst) -> int {
    dst.assign(v.size() * 24, 0);
    if (v.empty()) return ZKHIP_OK;
    std::vector<uint64_t> s = pack_scalars(v.data(), v.size());
    return zkhip_fixed_base_mul(base, s.data(), v.size(), 1, dst.data());
  };
  std::vector<uint64_t> s1, s2;
  if ((rc = fb(g1, sc.single, s1)) != ZKHIP_OK || (rc = fb(g2, sc.single, s2)) != ZKHIP_OK || (rc = fb(g1, sc.At, kp->A)) != ZKHIP_OK ||
      (rc = fb(g2, sc.Bt, kp->B2)) != ZKHIP_OK || (rc = fb(g1, sc.Bt, kp->B1)) != ZKHIP_OK || (rc = fb(g1, sc.hs, kp->H)) != ZKHIP_OK ||
      (rc = fb(g1, sc.ls, kp->L)) != ZKHIP_OK || (rc = fb(g1, sc.abc, kp->ABC)) != ZKHIP_OK) {
    delete kp;
    return rc;
  }
  kp->alpha_g1.assign(s1.begin(), s1.begin() + 24); kp->beta_g1.assign(s1.begin() + 24, s1.begin() + 48);
  kp->delta_g1.assign(s1.begin() + 48, s1.begin() + 72);
  kp->beta_g2.assign(s2.begin() + 24, s2.begin() + 48); kp->delta_g2.assign(s2.begin() + 48, s2.begin() + 72);
  *out = kp;
  return ZKHIP_OK;
}

// One rank's share of a trusted setup (BASELINE configs[3]: the key pre-partitioned over the GPUs of a node).  Every rank evaluates
// the exponents (host: seconds at 2^22), cuts the three index ranges by FINITE terms exactly as zkhip_key_partition would cut the
// finished key - an exponent of zero IS a base at infinity - and then multiplies ONLY its own slice: an N-th of the fixed-base work,
// the points go from k_fixed_base_mul's output straight into the slice's base sets and window tables without leaving the device
// (round 6, VERDICT r5 item 4: until then every rank generated the whole key, copied its 4 GB to the host twice and uploaded an
// N-th).  *vk_out: a keypair WITHOUT queries (verification half and the five constants a prover's tail needs).
int zkhip_groth16_setup_slice(const zkhip_r1cs_desc* cs, const uint64_t tau_m[6], const uint64_t alpha_m[6], const uint64_t beta_m[6],
                              const uint64_t delta_m[6], size_t domain_size, int parts, int part, const zkhip_key_opts* opts,
                              zkhip_crs** slice_out, size_t ranges[6], zkhip_keypair** vk_out) {
  using namespace host;
  BIND_CUR();
  if (!cs || !tau_m || !alpha_m || !beta_m || !delta_m || !slice_out || !ranges) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (parts < 1 || parts > 64 || part < 0 || part >= parts) return fail(ZKHIP_ERR_ARG, "setup_slice: part must be in [0, parts), parts in [1, 64]");
  { int rc_ = check_opts(opts); if (rc_ != ZKHIP_OK) return rc_; }
  SetupScalars sc;
  int rc = setup_scalars(cs, tau_m, alpha_m, beta_m, delta_m, domain_size, sc);
  if (rc != ZKHIP_OK) return rc;
  // the cuts of zkhip_key_partition, from the exponents: weight of index i = its finite bases among A, B-G2, B-G1
  std::vector<size_t> ca(parts + 1), chh(parts + 1), cl(parts + 1);
  {
    std::vector<uint32_t> w(sc.m);
    for (size_t i = 0; i < sc.m; i++) w[i] = (sc.At[i].is_zero() ? 0u : 1u) + (sc.Bt[i].is_zero() ? 0u : 2u);
    zkhip_internal_cuts_by_weight(w.data(), w.size(), (size_t)parts, ca.data());
    w.assign(sc.hs.size(), 0);
    for (size_t i = 0; i < sc.hs.size(); i++) w[i] = sc.hs[i].is_zero() ? 0u : 1u;
    zkhip_internal_cuts_by_weight(w.data(), w.size(), (size_t)parts, chh.data());
    w.assign(sc.ls.size(), 0);
    for (size_t i = 0; i < sc.ls.size(); i++) w[i] = sc.ls[i].is_zero() ? 0u : 1u;
    zkhip_internal_cuts_by_weight(w.data(), w.size(), (size_t)parts, cl.data());
  }
  const size_t a_lo = ca[part], a_len = ca[part + 1] - ca[part], h_lo = chh[part], h_len = chh[part + 1] - chh[part],
               l_lo = cl[part], l_len = cl[part + 1] - cl[part];
  ranges[0] = a_lo; ranges[1] = a_lo + a_len; ranges[2] = h_lo; ranges[3] = h_lo + h_len; ranges[4] = l_lo; ranges[5] = l_lo + l_len;
  uint64_t g1[24], g2[24];
  generators(g1, g2);
  // the constants and the verification half (l + 1 + 6 products): through the host, they are needed there
  std::unique_ptr<zkhip_keypair> kp(new zkhip_keypair());
  kp->n_vars = sc.m; kp->n_primary = sc.l; kp->domain_size = sc.d;
  {
    std::vector<uint64_t> s1(72), s2(72), ps = pack_scalars(sc.single.data(), 3), pa = pack_scalars(sc.abc.data(), sc.abc.size());
    kp->ABC.assign(sc.abc.size() * 24, 0);
    if ((rc = zkhip_fixed_base_mul(g1, ps.data(), 3, 1, s1.data())) != ZKHIP_OK || (rc = zkhip_fixed_base_mul(g2, ps.data(), 3, 1, s2.data())) != ZKHIP_OK ||
        (rc = zkhip_fixed_base_mul(g1, pa.data(), sc.abc.size(), 1, kp->ABC.data())) != ZKHIP_OK)
      return rc;
    kp->alpha_g1.assign(s1.begin(), s1.begin() + 24); kp->beta_g1.assign(s1.begin() + 24, s1.begin() + 48);
    kp->delta_g1.assign(s1.begin() + 48, s1.begin() + 72);
    kp->beta_g2.assign(s2.begin() + 24, s2.begin() + 48); kp->delta_g2.assign(s2.begin() + 48, s2.begin() + 72);
  }
  // the slice's five query vectors: exponents up, products on the device, straight into base sets
  zkhip_crs* c = new zkhip_crs();
  c->device = cur_dev();
  c->n_vars = sc.m; c->n_primary = sc.l; c->domain_size = sc.d;
  memcpy(c->alpha_g1, kp->alpha_g1.data(), 192); memcpy(c->beta_g1, kp->beta_g1.data(), 192); memcpy(c->beta_g2, kp->beta_g2.data(), 192);
  memcpy(c->delta_g1, kp->delta_g1.data(), 192); memcpy(c->delta_g2, kp->delta_g2.data(), 192);
  auto query = [&](const uint64_t* base, const HFr* v, size_t count, zkhip_bases** dst) -> int {
    if (!count) return zkhip_bases_upload_dev(nullptr, 0, dst);
    Scratch scr;
    void *ds = nullptr, *dp = nullptr;
    API_HIP(scr.alloc(&ds, count * 48));
    API_HIP(scr.alloc(&dp, count * 192));
    {
      const std::vector<uint64_t> s = pack_scalars(v, count);
      API_HIP(hipMemcpy(ds, s.data(), count * 48, hipMemcpyHostToDevice));
    }
    int r = zkhip_fixed_base_mul_dev(base, ds, count, 1, dp);
    if (r == ZKHIP_OK) r = zkhip_bases_upload_dev(dp, count, dst);
    return r;
  };
  if ((rc = query(g1, sc.At.data() + a_lo, a_len, &c->A)) == ZKHIP_OK && (rc = query(g2, sc.Bt.data() + a_lo, a_len, &c->B2)) == ZKHIP_OK &&
      (rc = query(g1, sc.Bt.data() + a_lo, a_len, &c->B1)) == ZKHIP_OK && (rc = query(g1, sc.hs.data() + h_lo, h_len, &c->H)) == ZKHIP_OK &&
      (rc = query(g1, sc.ls.data() + l_lo, l_len, &c->L)) == ZKHIP_OK)
    rc = crs_build_tables(c, resolve_opts(opts));
  if (rc != ZKHIP_OK) { zkhip_crs_free(c); return rc; }
  *slice_out = c;
  if (vk_out) *vk_out = kp.release();
  return ZKHIP_OK;
}

int zkhip_keypair_crs_desc(const zkhip_keypair* kp, zkhip_crs_desc* o) {
  if (!kp || !o) return ZKHIP_ERR_ARG;
  o->n_vars = kp->n_vars; o->n_primary = kp->n_primary; o->domain_size = kp->domain_size;
  o->alpha_g1 = kp->alpha_g1.data(); o->beta_g1 = kp->beta_g1.data(); o->beta_g2 = kp->beta_g2.data();
  o->delta_g1 = kp->delta_g1.data(); o->delta_g2 = kp->delta_g2.data();
  o->a_query = kp->A.data(); o->b_g2_query = kp->B2.data(); o->b_g1_query = kp->B1.data(); o->h_query = kp->H.data(); o->l_query = kp->L.data();
  return ZKHIP_OK;
}

size_t zkhip_keypair_vk(const zkhip_keypair* kp, uint64_t alpha_g1[24], uint64_t beta_g2[24], uint64_t delta_g2[24], const uint64_t** abc) {
  if (!kp || !alpha_g1 || !beta_g2 || !delta_g2 || !abc) return 0;
  memcpy(alpha_g1, kp->alpha_g1.data(), 192); memcpy(beta_g2, kp->beta_g2.data(), 192); memcpy(delta_g2, kp->delta_g2.data(), 192);
  *abc = kp->ABC.data();
  return kp->n_primary + 1;
}

int zkhip_keypair_write(const zkhip_keypair* kp, const char* path) {
  if (!kp || !path) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (kp->A.size() != kp->n_vars * 24 || kp->H.size() != (kp->domain_size - 1) * 24)
    return fail(ZKHIP_ERR_ARG, "this keypair holds no query vectors (zkhip_groth16_setup_slice keeps the slice on the device): nothing to write");
  FILE* f = fopen(path, "wb");
  if (!f) return fail(ZKHIP_ERR_ARG, "cannot open the keypair file for writing");
  uint64_t hdr[8] = {0, (uint64_t)kp->n_vars, (uint64_t)kp->n_primary, (uint64_t)kp->domain_size, 0, 0, 0, 0};
  memcpy(&hdr[0], KP_MAGIC, 8);
  uint64_t h = 0xcbf29ce484222325ull;
  bool ok = fwrite(hdr, 8, 8, f) == 8;
  h = fnv1a(h, hdr, sizeof hdr);
  const std::vector<uint64_t>* parts[] = {&kp->alpha_g1, &kp->beta_g1, &kp->beta_g2, &kp->delta_g1, &kp->delta_g2, &kp->A, &kp->B2, &kp->B1, &kp->H, &kp->L, &kp->ABC};
  for (const auto* v : parts) {
    ok = ok && fwrite(v->data(), 8, v->size(), f) == v->size();
    h = fnv1a(h, v->data(), v->size() * 8);
  }
  ok = ok && fwrite(&h, 8, 1, f) == 1;
  ok = (fclose(f) == 0) && ok;
  return ok ? ZKHIP_OK : fail(ZKHIP_ERR_ARG, "short write on the keypair file");
}

int zkhip_keypair_read(const char* path, zkhip_keypair** out) {
  if (!path || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  FILE* f = fopen(path, "rb");
  if (!f) return fail(ZKHIP_ERR_ARG, "cannot open the keypair file");
  uint64_t hdr[8];
  if (fread(hdr, 8, 8, f) != 8 || memcmp(&hdr[0], KP_MAGIC, 8) != 0) { fclose(f); return fail(ZKHIP_ERR_ARG, "not a keypair file (bad magic)"); }
  const uint64_t m = hdr[1], l = hdr[2], d = hdr[3];
  // the prover's domains stop at 2^22 points; a key has at most that many variables (one constraint defines at most one)
  // (the domain is one that get_evaluation_domain can return: a power of two or 2^k + 2^r - a fixed point of eval_domain_size)
  if (m < l + 1 || d < 1 || host::eval_domain_size((size_t)d) != d || m > ((uint64_t)1 << 23) || d > ((uint64_t)1 << 22)) { fclose(f); return fail(ZKHIP_ERR_ARG, "keypair file: implausible sizes"); }
  // the header fixes the file's length: check it before any allocation is sized by it
  {
    const uint64_t pts = 5 + 3 * m + (d - 1) + (m - l - 1) + (l + 1), want = 64 + 8 * 24 * pts + 8;
    long here = ftell(f);
    bool okl = here == 64 && fseek(f, 0, SEEK_END) == 0 && (uint64_t)ftell(f) == want && fseek(f, here, SEEK_SET) == 0;
    if (!okl) { fclose(f); return fail(ZKHIP_ERR_ARG, "keypair file truncated or corrupted (length does not match its header)"); }
  }
  zkhip_keypair* kp = nullptr;
  try {
  kp = new zkhip_keypair();
  kp->n_vars = m; kp->n_primary = l; kp->domain_size = d;
  struct { std::vector<uint64_t>* v; size_t pts; } parts[] = {{&kp->alpha_g1, 1}, {&kp->beta_g1, 1}, {&kp->beta_g2, 1}, {&kp->delta_g1, 1}, {&kp->delta_g2, 1},
                                                              {&kp->A, m}, {&kp->B2, m}, {&kp->B1, m}, {&kp->H, d - 1}, {&kp->L, m - l - 1}, {&kp->ABC, l + 1}};
  uint64_t h = fnv1a(0xcbf29ce484222325ull, hdr, sizeof hdr), stored = 0;
  bool ok = true;
  for (auto& p : parts) {
    p.v->resize(p.pts * 24);
    ok = ok && fread(p.v->data(), 8, p.v->size(), f) == p.v->size();
    if (!ok) break;
    h = fnv1a(h, p.v->data(), p.v->size() * 8);
  }
  ok = ok && fread(&stored, 8, 1, f) == 1 && stored == h;
  fclose(f);
  if (!ok) { delete kp; return fail(ZKHIP_ERR_ARG, "keypair file truncated or corrupted (checksum)"); }
  *out = kp;
  return ZKHIP_OK;
  } catch (const std::exception& e) {       // std::bad_alloc: no exception crosses the C ABI
    fclose(f);
    delete kp;
    snprintf(t_err, sizeof t_err, "keypair file: %s", e.what());
    return ZKHIP_ERR_ARG;
  }
}

void zkhip_keypair_free(zkhip_keypair* kp) { delete kp; }

}  // extern "C"
