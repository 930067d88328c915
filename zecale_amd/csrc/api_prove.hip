// C ABI (include/zkhip.h): Groth16 proofs - the five MSMs' strategies, the host tail, the plain entry points and zkhip_prover.
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <thread>

#include "api_internal.hpp"
#include "wait.h"

using namespace zkhip::api;

#pragma GCC visibility push(hidden)      // this file's own helpers and handle structs

// ---- prover instances: one proof in flight each, several instances per GPU -------------------------------------------
struct zkhip_prover {
  int device;
  const zkhip_crs* crs;
  R1csDev* rd;          // own copy of the constraint system + QAP work buffers
  ProveState ps;
  std::mutex mu;
  bool slice = false;                    // crs is a slice of the key (zkhip_prover_new_slice): partial sums only
  size_t a_lo = 0, h_lo = 0, l_lo = 0;   // where the slice starts in the A / B, H and L queries
  bool checked = false;                  // zkhip_prover_set_checked: rd runs the checking variants, a refused input gets no proof
  int refusal_kind = 0;                  // of the last proof: 0 none, else ZKHIP_REFUSAL_*
  size_t refusal_index = 0;
};

// a checked prover after prove_partial: the flag words the QAP map's stream left on the host (qap.h) -> the smallest kind that applies
// and its smallest index.  The words are complete: every strategy has waited for that stream's part of the proof.
static int prover_refusal(zkhip_prover* p) {
  static const char* const what[ZK_CHK_WORDS] = {"an assignment entry is not below r", "z[0] is not the constant ONE",
                                                 "the assignment does not satisfy a constraint",
                                                 "the masked assignment is non-zero at one of the application's constant positions"};
  for (int k = 0; k < ZK_CHK_WORDS; k++) {
    const uint32_t w = p->rd->chk_host[k];
    if (w == ZK_CHK_NONE) continue;
    p->refusal_kind = k + 1;               // ZKHIP_REFUSAL_ENCODING .. _APP_MASK, in the order of the words
    p->refusal_index = w;
    snprintf(t_err, sizeof t_err, "checked prover: %s (index %u); no proof was written", what[k], w);
    return ZKHIP_ERR_REFUSED;
  }
  return ZKHIP_OK;
}

// the proof's key and (for a host assignment) its masking
static int app_check(const zkhip_aggregator_app* app, const zkhip_crs* crs, const uint64_t* z_host) {
  if (app->crs != crs) return fail(ZKHIP_ERR_ARG, "this application handle was made for another proving key");
  if (z_host)
    for (uint32_t i : app->s_idx) {
      const uint64_t* w = z_host + (size_t)i * 6;
      if (w[0] | w[1] | w[2] | w[3] | w[4] | w[5])
        return fail(ZKHIP_ERR_ARG, "assignment is not masked: a non-zero value at one of the application's constant positions (zkhip_aggregator_witness_app / zkhip_aggregator_app_mask)");
    }
  return ZKHIP_OK;
}
// A, B-G2, B-G1 and L sums of a masked proof += the application's cached points (H is untouched)
static void app_add_points(const zkhip_aggregator_app* app, uint64_t sums[180]) {
  using namespace host;
  auto jac = [](const uint64_t* p) { HJac q; q.X = HFq::from_limbs(p); q.Y = HFq::from_limbs(p + 12); q.Z = HFq::from_limbs(p + 24); return q; };
  static const int slot[4] = {0, 1, 2, 4};
  for (int k = 0; k < 4; k++) {
    uint64_t* s = sums + 36 * slot[k];
    const HJac t = jac(s).add(jac(app->points + 36 * k));
    t.X.to_limbs(s); t.Y.to_limbs(s + 12); t.Z.to_limbs(s + 24);
  }
}

// The proving key is authoritative for the evaluation domain (a reference key of the wrapping circuit says 65,536, a key generated
// here with ZKHIP_DOMAIN_STEP says 49,152): a shared constraint-system handle that sits on another domain is moved to the key's -
// its matrices stay, the domain's buffers are rebuilt (once: the next proof with this key finds it there).  A key whose domain is
// too small for the system, or not a domain at all, is refused.  Caller holds the device's mutex.
static int follow_key_domain(const zkhip_crs* crs, R1csDev* rd) {
  if (crs->n_vars != rd->n_vars || crs->n_primary != rd->n_primary) return fail(ZKHIP_ERR_ARG, "proving key and constraint system do not match");
  if (crs->domain_size == rd->d) return ZKHIP_OK;
  if (crs->domain_size == 0 || crs->domain_size == (size_t)-1) return fail(ZKHIP_ERR_ARG, "proving key without a domain size");
  return r1cs_set_domain(rd, crs->domain_size, t_err, sizeof t_err);
}

// 0 (default): a proof's five MSMs are one launch sequence; 1 / 2: the split form (see prove_partial).  ZKHIP_PROVE_SPLIT / zkhip_set_prove_split.
static std::atomic<int> g_prove_split{[] { const char* e = getenv("ZKHIP_PROVE_SPLIT"); const int v = e ? atoi(e) : 0; return v < 0 || v > 2 ? 0 : v; }()};
// the cheap argument and size checks of a proof, before anything is started for it (the tail's scalar multiplications used to
// be spawned before them)
static int prove_check(const zkhip_crs* crs, const R1csDev* rd, size_t a_lo, size_t h_lo, size_t l_lo) {
  const size_t m = rd->n_vars, l = rd->n_primary, d = rd->d;
  const size_t a_len = crs->A->len, h_len = crs->H->len, l_len = crs->L->len;
  if (crs->n_vars != m || crs->n_primary != l) return fail(ZKHIP_ERR_ARG, "proving key and constraint system do not match");
  if (crs->domain_size != d) return fail(ZKHIP_ERR_ARG, "the constraint system handle is not on the proving key's evaluation domain");
  if (crs->B2->len != a_len || crs->B1->len != a_len || a_lo + a_len > m || h_lo + h_len > d - 1 || l_lo + l_len > m - l - 1)
    return fail(ZKHIP_ERR_ARG, "key slice out of range");
  const int tc = crs->A->table_c;
  if (crs->B2->table_naf != crs->A->table_naf || crs->B1->table_naf != crs->A->table_naf || crs->H->table_naf != crs->A->table_naf ||
      crs->L->table_naf != crs->A->table_naf)
    return fail(ZKHIP_ERR_ARG, "the five query vectors of a proving key must share one kind of table");
  if (crs->B2->table_c != tc || crs->B1->table_c != tc || crs->H->table_c != tc || crs->L->table_c != tc)
    return fail(ZKHIP_ERR_ARG, "the five query vectors of a proving key must share one table window");
  return ZKHIP_OK;
}

using clk = std::chrono::steady_clock;
static double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// One MSM of a proof over the first len bases of a query vector.  The finite-bases bound counts only for a WHOLE vector.
static MsmJob query_job(const zkhip_bases* b, const uint64_t* scalars, size_t len, int scalars_mode) {
  return MsmJob{b->d_pts, b->d_inf, scalars, len, scalars_mode, b->len, len == b->len ? b->n_finite : 0};
}
// what a proof's strategies share: its state, its inputs, and the five MSMs in the order of `sums` - A, B-G2, B-G1, H, L
struct ProofRun {
  ProveState& ps;
  R1csDev* rd;
  const uint64_t *z_host, *dz, *d_z_app;   // z_host: null when the assignment is already on the device (dz)
  int tc, naf;                             // the key's table window (0: plain) and kind
  clk::time_point t0;                      // start of the phase being timed
  uint64_t* sums;
  MsmJob jobs[5];
};
static void proof_jobs(const zkhip_crs* crs, const R1csDev* rd, const uint64_t* dz, size_t a_lo, size_t h_lo, size_t l_lo, MsmJob jobs[5]) {
  const uint64_t *za = dz + a_lo * 6, *zl = dz + (rd->n_primary + 1 + l_lo) * 6, *h = (const uint64_t*)rd->bufA + h_lo * 6;
  jobs[0] = query_job(crs->A, za, crs->A->len, 1); jobs[1] = query_job(crs->B2, za, crs->A->len, 1); jobs[2] = query_job(crs->B1, za, crs->A->len, 1);
  jobs[3] = query_job(crs->H, h, crs->H->len, 2); jobs[4] = query_job(crs->L, zl, crs->L->len, 1);    // (h: the QAP map's output, packed device form)
  // a key on the Edwards model: its four G1 jobs bring their Edwards tables (B-G2 has none)
  if (crs->table_model) { jobs[0].edw = crs->A->d_edw; jobs[2].edw = crs->B1->d_edw; jobs[3].edw = crs->H->d_edw; jobs[4].edw = crs->L->d_edw; }
}
// a key on the Edwards model (prove_edwards): the four G1 jobs A, B-G1, H, L of one launch sequence; maxlen of their plan
static void g1_jobs(const MsmJob jobs[5], MsmJob g1[4]) { g1[0] = jobs[0]; g1[1] = jobs[2]; g1[2] = jobs[3]; g1[3] = jobs[4]; }
static size_t jobs_maxlen(const MsmJob* jobs, int K) {
  size_t m = 1;
  for (int k = 0; k < K; k++) if (jobs[k].n > m) m = jobs[k].n;
  return m;
}
static size_t jobs_terms(const MsmJob* jobs, int K) {
  size_t t = 0;
  for (int k = 0; k < K; k++) t += msm_job_terms(jobs[k]);
  return t ? t : 1;
}
// a strategy's answer when its plan does not fit the engine's 32-bit entry positions (ensure_ctx: ZKHIP_ERR_ARG) and nothing has been
// enqueued: the next strategy decides.  Never leaves prove_partial.
constexpr int ZK_PLAN_UNFIT = 1;

// OPTION, off by default (ZKHIP_PROVE_SPLIT=1; =2: without the gate between the two accumulations) - a proof that is alone on the
// chip as TWO launch sequences (round 6): four of the five MSMs - A, B-G2, B-G1, L - need only the assignment, so
// their sort and accumulation start as soon as z is on the device, on their own plan, while the QAP map runs beside them on the
// prover's stream; the H MSM follows on a second plan behind an event on h, and the bucket reduction of the first sequence runs
// under its accumulation.  Same group elements, bit-identical proofs (the partitioned and serial tests pass with it on).
// MEASURED AND NOT ADOPTED (profiles/r06_split_proof_ab.txt, one box, tools/partition_model.py): one 2^20 proof alone 50.0 ms as one
// sequence, 52.0 split (49.8-50.5 without the gate); one rank of an eight-way 2^22 key 38.6 -> 39.8 ms; an eighth of a 2^20 key
// 12.4 -> 13.5-14.8 ms.  The map is not idle time to hide: at 2^22 its seven FFTs and three SpMVs fill the chip (9.4 ms of
// multiplier and HBM work) and share the accumulation's issue slots when run beside it - the two accumulation launches together
// take 44 ms where the single one takes 37 - and every launch sequence brings its own one-fill tail, stitching and reduction chain.
static int prove_split(ProofRun& p, bool gated) {
  ProveState& ps = p.ps;
  const MsmJob jz[4] = {p.jobs[0], p.jobs[1], p.jobs[2], p.jobs[4]}, &jh = p.jobs[3];
  MsmCtx *cz = &ps.ctx[ZK_CTX_Z], *ch = &ps.ctx[ZK_CTX_H];
  const size_t max_z = jz[0].n > jz[3].n ? jz[0].n : jz[3].n;
  int rc = ensure_ctx(cz, ps.lane[ZK_CTX_Z], max_z ? max_z : 1, p.tc, 4, p.naf, jobs_terms(jz, 4));
  if (rc == ZKHIP_OK) rc = ensure_ctx(ch, ps.lane[ZK_CTX_H], jh.n, p.tc, 1, p.naf, jobs_terms(&jh, 1));
  if (rc != ZKHIP_OK) return rc == ZKHIP_ERR_ARG ? ZK_PLAN_UNFIT : rc;
  if (!ps.ev_up) API_HIP(hipEventCreateWithFlags(&ps.ev_up, hipEventDisableTiming));
  if (!ps.ev_qap) API_HIP(hipEventCreateWithFlags(&ps.ev_qap, hipEventDisableTiming));
  if (p.z_host) API_HIP(hipMemcpyAsync(ps.dz, p.z_host, p.rd->n_vars * 48, hipMemcpyHostToDevice, ps.st));
  API_HIP(hipEventRecord(ps.ev_up, ps.st));
  API_HIP(hipStreamWaitEvent(ps.lane[ZK_CTX_Z].main, ps.ev_up, 0));
  ps.ms[0] = ms_since(p.t0);
  const auto tl0 = p.t0 = clk::now();
  if ((rc = msm_launch_multi(cz, 4, jz)) != ZKHIP_OK) return ctx_fail(rc, cz);
  rc = qap_h_dev(p.rd, p.dz, ps.st, t_err, sizeof t_err, p.d_z_app);
  if (rc == ZKHIP_OK) {
    hipError_t e = hipEventRecord(ps.ev_qap, ps.st);
    if (e == hipSuccess) e = hipStreamWaitEvent(ps.lane[ZK_CTX_H].main, ps.ev_qap, 0);
    if (e != hipSuccess) { snprintf(t_err, sizeof t_err, "split proof: %s", hipGetErrorString(e)); rc = ZKHIP_ERR_HIP; }
  }
  if (rc == ZKHIP_OK) {
    ch->acc_gate = gated ? ps.lane[ZK_CTX_Z].ev_acc1 : nullptr;        // H's accumulation starts when the first one has ended
    if ((rc = msm_launch_multi(ch, 1, &jh)) != ZKHIP_OK) (void)ctx_fail(rc, ch);
    ch->acc_gate = nullptr;
  }
  ps.ms[1] = ms_since(p.t0);                      // (enqueueing the QAP map and both sequences: the phases overlap on the device)
  // whatever was enqueued is collected on every exit (a pending plan would refuse the next proof); the first error is reported
  uint64_t sz[4 * 36];
  const int rc_z = msm_finish_multi(cz, 4, sz);
  const int rc_h = rc == ZKHIP_OK ? msm_finish_multi(ch, 1, p.sums + 108) : ZKHIP_OK;
  if (rc == ZKHIP_OK && rc_z != ZKHIP_OK) rc = ctx_fail(rc_z, cz);
  if (rc == ZKHIP_OK && rc_h != ZKHIP_OK) rc = ctx_fail(rc_h, ch);
  if (rc != ZKHIP_OK) { (void)hipStreamSynchronize(ps.st); return rc; }
  memcpy(p.sums, sz, 3 * 36 * 8); memcpy(p.sums + 144, sz + 108, 36 * 8);
  for (int j = 0; j < 5; j++) ps.ms[2 + j] = ms_since(tl0);
  note_last_acc(ps, cz);                          // (two accumulation launches: the sum of their times)
  ps.last_accumulate_ms += ch->last_accumulate_ms; ps.last_acc_ctx2 = ch;
  ps.split_last = true;
  return ZKHIP_OK;
}
// the assignment to the device and the QAP map on stream qst; a chained proof does not wait for either
static int prove_upload_and_map(ProofRun& p, hipStream_t qst, bool chain) {
  ProveState& ps = p.ps;
  auto host_waits = [&]() -> int {      // (the MSM contexts run on their own streams; a chained proof's MSMs follow on qst)
    if (!chain) { API_HIP(hipEventRecord(ps.ev_st, qst)); API_HIP(zk_event_wait(ps.ev_st)); }
    return ZKHIP_OK;
  };
  int rc = ZKHIP_OK;
  if (p.z_host) {
    API_HIP(hipMemcpyAsync(ps.dz, p.z_host, p.rd->n_vars * 48, hipMemcpyHostToDevice, qst));
    if ((rc = host_waits()) != ZKHIP_OK) return rc;
  }
  ps.ms[0] = ms_since(p.t0);
  p.t0 = clk::now();
  // (an application's constants - d_z_app - are part of the assignment the QAP map sees; the MSMs over z run on the masked
  //  vector: a zero scalar produces no bucket entry, the constants' share of A, B and L is the application's four cached points)
  if ((rc = qap_h_dev(p.rd, p.dz, qst, t_err, sizeof t_err, p.d_z_app)) == ZKHIP_OK) rc = host_waits();
  ps.ms[1] = ms_since(p.t0);
  return rc;
}
// Table-backed key: the five MSMs share ONE launch sequence (one sort, one accumulation launch over all five entry lists, one
// reduction chain with a bucket window per MSM) - a fifth of the launches, five times the lanes in each.
static int prove_batched(ProofRun& p, size_t maxlen, bool chain) {
  ProveState& ps = p.ps;
  MsmCtx* cx = &ps.ctx[ZK_MSM_SLOTS];
  const size_t total = jobs_terms(p.jobs, 5);
  int rc = ensure_ctx(cx, ps.lane[ZK_MSM_SLOTS], maxlen, p.tc, 5, p.naf, total);
  if (rc == ZKHIP_ERR_ARG) {
    // (a silent performance cliff) the plan's 32-bit entry positions / slice weights do not hold this key's terms at
    // this window: said once per process, then one launch sequence per MSM
    static std::atomic<bool> told{false};
    if (!told.exchange(true))
      fprintf(stderr, "zkhip: the five MSMs of this key do not fit ONE launch sequence (window %d, %zu terms: 32-bit slice weights); "
                      "using one sequence per MSM - a larger table window (zkhip_key_opts.window) avoids this\n", p.tc, total);
    return ZK_PLAN_UNFIT;
  }
  if (rc != ZKHIP_OK) return rc;
  if (ps.quad_below) { cx->quad_below = ps.quad_below; cx->one_stream = 1; }
  const auto tl0 = clk::now();
  if ((rc = msm_launch_multi(cx, 5, p.jobs)) == ZKHIP_OK) rc = msm_finish_multi(cx, 5, p.sums);
  if (rc != ZKHIP_OK) {
    // (a chained proof's stream also carried the upload and the QAP map: their failure surfaces here)
    snprintf(t_err, sizeof t_err, "%s%s", cx->errbuf, chain ? " [chained proof: this stream also carried the upload of the assignment and the QAP map]" : "");
    return rc;
  }
  for (int j = 0; j < 5; j++) ps.ms[2 + j] = ms_since(tl0);
  note_last_acc(ps, cx);
  return ZKHIP_OK;
}
// A key on the Edwards model (zkhip_key_opts.table_model = 1): the four G1 MSMs - A, B-G1, H, L - are ONE launch sequence that adds on
// G1's 2-isogenous Edwards curve (a K = 4 plan on the context of the batched proofs: k_accumulate_edw_multi), and B-G2, whose curve has no
// such model, is a K = 1 XYZZ sequence on a context and lane of its own.  B-G2 needs only the assignment: it is enqueued behind the
// upload (a chained proof: behind an event on the stream that carries it) and runs beside the QAP map; the G1 sequence follows the
// map.  Two plans in one proof as in prove_split, and its rules: whatever was enqueued is collected on every exit, the first error is
// reported.  Timings: ms[0] / ms[1] as in the other strategies (enqueueing times when chained; ms[1] includes enqueueing B-G2), the five
// MSM slots the time from B-G2's launch to the collection of both sequences.
static int prove_edwards(ProofRun& p, bool chain) {
  ProveState& ps = p.ps;
  MsmJob jg[4];
  g1_jobs(p.jobs, jg);
  const MsmJob& jb = p.jobs[1];
  MsmCtx *cg = &ps.ctx[ZK_MSM_SLOTS], *cb = &ps.ctx[ZK_CTX_H];
  int rc = ensure_ctx(cg, ps.lane[ZK_MSM_SLOTS], jobs_maxlen(jg, 4), p.tc, 4, 0, jobs_terms(jg, 4));
  if (rc == ZKHIP_OK) rc = ensure_ctx(cb, ps.lane[ZK_CTX_H], jb.n ? jb.n : 1, p.tc, 1, 0, jobs_terms(&jb, 1), 0, ps.quad_below ? 1 : -1);
  if (rc != ZKHIP_OK) return rc == ZKHIP_ERR_ARG ? ZK_PLAN_UNFIT : rc;
  if (ps.quad_below) for (MsmCtx* cx : {cg, cb}) { cx->quad_below = ps.quad_below; cx->one_stream = 1; }
  if (!ps.ev_up) API_HIP(hipEventCreateWithFlags(&ps.ev_up, hipEventDisableTiming));
  hipStream_t qst = chain ? ps.lane[ZK_MSM_SLOTS].main : ps.st;
  if (p.z_host) API_HIP(hipMemcpyAsync(ps.dz, p.z_host, p.rd->n_vars * 48, hipMemcpyHostToDevice, qst));
  if (chain) {      // B-G2's stream follows the upload; the host does not wait
    API_HIP(hipEventRecord(ps.ev_up, qst));
    API_HIP(hipStreamWaitEvent(ps.lane[ZK_CTX_H].main, ps.ev_up, 0));
  } else if (p.z_host) { API_HIP(hipEventRecord(ps.ev_st, qst)); API_HIP(zk_event_wait(ps.ev_st)); }
  ps.ms[0] = ms_since(p.t0);
  const auto tl0 = p.t0 = clk::now();
  if ((rc = msm_launch_multi(cb, 1, &jb)) != ZKHIP_OK) return ctx_fail(rc, cb);
  // from here on B-G2 is in flight: every exit collects it
  bool g1_launched = false;
  if ((rc = qap_h_dev(p.rd, p.dz, qst, t_err, sizeof t_err, p.d_z_app)) == ZKHIP_OK && !chain) {
    hipError_t e = hipEventRecord(ps.ev_st, qst);
    if (e == hipSuccess) e = zk_event_wait(ps.ev_st);
    if (e != hipSuccess) { snprintf(t_err, sizeof t_err, "Edwards proof: %s", hipGetErrorString(e)); rc = ZKHIP_ERR_HIP; }
  }
  ps.ms[1] = ms_since(p.t0);
  if (rc == ZKHIP_OK) {
    if ((rc = msm_launch_multi(cg, 4, jg)) != ZKHIP_OK) (void)ctx_fail(rc, cg);
    else g1_launched = true;
  }
  const bool g1_edw = g1_launched && cg->win_edw;      // (what the launch itself decided: a silent XYZZ launch reads 0)
  uint64_t sg[4 * 36];
  const int rc_b = msm_finish_multi(cb, 1, p.sums + 36);
  const int rc_g = g1_launched ? msm_finish_multi(cg, 4, sg) : ZKHIP_OK;
  if (rc == ZKHIP_OK && rc_g != ZKHIP_OK) {
    snprintf(t_err, sizeof t_err, "%s%s", cg->errbuf, chain ? " [chained proof: this stream also carried the upload of the assignment and the QAP map]" : "");
    rc = rc_g;
  }
  if (rc == ZKHIP_OK && rc_b != ZKHIP_OK) rc = ctx_fail(rc_b, cb);
  if (rc != ZKHIP_OK) { (void)hipStreamSynchronize(qst); return rc; }
  memcpy(p.sums, sg, 36 * 8); memcpy(p.sums + 72, sg + 36, 3 * 36 * 8);      // A | (B-G2) | B-G1, H, L
  for (int j = 0; j < 5; j++) ps.ms[2 + j] = ms_since(tl0);
  note_last_acc(ps, cg);                          // (two accumulation launches: the sum of their times, the entries of both)
  ps.last_accumulate_ms += cb->last_accumulate_ms; ps.last_acc_ctx2 = cb;
  ps.edw_last = g1_edw;
  return ZKHIP_OK;
}
// One launch sequence per MSM, several in flight: while MSM j reduces its buckets (latency-bound, few lanes), MSM j+1 accumulates.
// Large circuits keep two contexts (each holds ~1.3 GB of work space at 2^20); small ones (every phase is latency-bound and the
// chip is mostly idle) run all five MSMs side by side.  These launches take only the geometry of a job - plans of K = 1 without a
// bound on the terms, no finite-bases bound - and the job's Edwards table, which only a key on the Edwards model brings: its G1 MSMs
// then go through the single-MSM Edwards kernels, B-G2 as ever.
static int prove_separate(ProofRun& p, size_t maxlen) {
  ProveState& ps = p.ps;
  const int nctx = (maxlen <= ((size_t)1 << 18)) ? 5 : 2;
  for (int k = 0, rc; k < nctx; k++) {
    if ((rc = ensure_ctx(&ps.ctx[k], ps.lane[k], maxlen, p.tc, 1, p.naf)) != ZKHIP_OK) return rc;
    if (ps.quad_below) { ps.ctx[k].quad_below = ps.quad_below; ps.ctx[k].one_stream = 1; }
  }
  clk::time_point tl[5];
  bool g1_edw = p.jobs[0].edw || p.jobs[2].edw || p.jobs[3].edw || p.jobs[4].edw;      // then: every G1 launch that had terms accumulated on the Edwards curve
  for (int j = 0; j < 5 + nctx; j++) {          // launch j, after collecting launch j - nctx from the same context
    MsmCtx* cx = &ps.ctx[j % nctx];
    int rc;
    if (j >= nctx) {
      rc = msm_finish(cx, p.sums + 36 * (j - nctx));
      ps.ms[2 + j - nctx] = ms_since(tl[j - nctx]);
      if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
    }
    if (j >= 5) continue;
    const MsmJob& job = p.jobs[j];
    tl[j] = clk::now();
    rc = msm_launch(cx, job.bases, job.inf_flags, job.scalars, job.n, job.scalars_mode, job.table_stride, job.edw);
    if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
    if (j != 1 && job.n && !cx->win_edw) g1_edw = false;
  }
  ps.edw_last = g1_edw;
  note_last_acc(ps, &ps.ctx[4 % nctx]);
  return ZKHIP_OK;
}

// The five MSMs of a proof over THIS process's slice of the proving key (the key is partitioned across the
// GPUs of a node; each rank computes partial sums, the ranks exchange 5 x 288 bytes).  Slice = [a_lo, a_lo + a_len) of
// the A / B queries (indices into z), [h_lo, h_lo + h_len) of the H query (indices into h), [l_lo, l_lo + l_len) of the
// L query (indices into z[n_primary+1 ..]).  The whole key is the slice (0, n_vars), (0, d - 1), (0, n_vars - l - 1).
// z: host assignment (uploaded here) - or d_z_ready: the assignment already in device memory, ABI form, complete (GPU witness)
static int prove_partial(ProveState& ps, const zkhip_crs* crs, R1csDev* rd, const uint64_t* z, size_t a_lo, size_t h_lo, size_t l_lo,
                         uint64_t sums[5 * 36], const uint64_t* d_z_ready = nullptr, const uint64_t* d_z_app = nullptr) {
  const size_t m = rd->n_vars;
  { int rc_ = prove_check(crs, rd, a_lo, h_lo, l_lo); if (rc_ != ZKHIP_OK) return rc_; }
  const int tc = crs->A->table_c, naf = crs->A->table_naf;
  const auto t0 = clk::now();
  if (!ps.st) {
    // (ZKHIP_QAP_STREAM_PRIO=1: the QAP map's stream at the highest priority - an experiment of the split proof)
    static const int qprio = getenv("ZKHIP_QAP_STREAM_PRIO") ? atoi(getenv("ZKHIP_QAP_STREAM_PRIO")) : 0;
    int lo = 0, hi = 0;
    if (qprio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) API_HIP(hipStreamCreateWithPriority(&ps.st, hipStreamNonBlocking, hi));
    else API_HIP(hipStreamCreateWithFlags(&ps.st, hipStreamNonBlocking));
  }
  if (!ps.ev_st) API_HIP(hipEventCreateWithFlags(&ps.ev_st, hipEventBlockingSync | hipEventDisableTiming));
  if (ps.dz_cap < m) {
    if (ps.dz) { (void)hipFree(ps.dz); ps.dz = nullptr; ps.dz_cap = 0; }
    API_HIP(hipMalloc(&ps.dz, m * 48));
    ps.dz_cap = m;
  }
  ProofRun p{ps, rd, d_z_ready ? nullptr : z, d_z_ready ? d_z_ready : ps.dz, d_z_app, tc, naf, t0, sums, {}};
  proof_jobs(crs, rd, p.dz, a_lo, h_lo, l_lo, p.jobs);
  const size_t a_len = p.jobs[0].n, h_len = p.jobs[3].n;
  const size_t maxlen = a_len > h_len ? a_len : (h_len ? h_len : 1);
  // a streaming prover whose five MSMs go through one launch sequence on ONE stream puts the upload and the QAP map on that stream
  // too: the host thread enqueues a whole proof without waiting between the phases (device side 376.8 -> 387.5 proofs/s in three
  // A/B pairs; ZKHIP_STREAM_CHAIN=0 restores the two waits, =2 chains every prover instance: +0.8 % for four 2^20 provers, not
  // adopted - the plain entry point's phase timings are the bench's one-proof-alone figures).  A chained proof's phase timings measure
  // enqueueing, not execution.
  // (only when the launch sequence's context will be used as it stands: its lane outlives a plan made again, so the clause guards no stream - it decides which proofs report enqueueing times, never a prover's first)
  static const int chain_env = getenv("ZKHIP_STREAM_CHAIN") ? atoi(getenv("ZKHIP_STREAM_CHAIN")) : 1;
  // (a key on the Edwards model: BOTH contexts of prove_edwards as they stand)
  const bool edw_key = crs->table_model == 1 && tc > 0;
  MsmJob jg[4];
  g1_jobs(p.jobs, jg);
  const bool ctx_ready = !edw_key ? ctx_reusable(&ps.ctx[ZK_MSM_SLOTS], maxlen, tc, 5, naf, jobs_terms(p.jobs, 5))
                                  : ctx_reusable(&ps.ctx[ZK_MSM_SLOTS], jobs_maxlen(jg, 4), tc, 4, 0, jobs_terms(jg, 4)) &&
                                        ctx_reusable(&ps.ctx[ZK_CTX_H], a_len ? a_len : 1, tc, 1, 0, jobs_terms(&p.jobs[1], 1));
  const bool chain = chain_env && (ps.quad_below || chain_env == 2) && tc > 0 && crs->batch_msms && ctx_ready;
  ps.chained_last = chain;
  ps.split_last = false;
  ps.edw_last = false;
  ps.last_acc_ctx2 = nullptr;
  int rc;
  if (edw_key && crs->batch_msms)      // (ZK_PLAN_UNFIT: nothing enqueued, never a chained proof - the XYZZ strategies decide)
    if ((rc = prove_edwards(p, chain)) != ZK_PLAN_UNFIT) return rc;
  const int split_env = g_prove_split.load();
  if (split_env && !edw_key && !chain && !ps.quad_below && tc > 0 && crs->batch_msms && h_len > 0 && a_len > 0)
    if ((rc = prove_split(p, split_env != 2)) != ZK_PLAN_UNFIT) return rc;
  if ((rc = prove_upload_and_map(p, chain ? ps.lane[ZK_MSM_SLOTS].main : ps.st, chain)) != ZKHIP_OK) return rc;
  if (tc > 0 && crs->batch_msms)
    if ((rc = prove_batched(p, maxlen, chain)) != ZK_PLAN_UNFIT) return rc;
  return prove_separate(p, maxlen);
}

// tail: A = alpha + evA + r delta1;  B = beta + evB + s delta;  C = evH + evL + s A + r B1 - rs delta1
// The part of the prover's tail that depends on the key and on (r, s) only - r delta1, s delta2, s delta1, rs delta1: four 377-bit
// scalar multiplications of single points - is started BEFORE the device work of a proof and collected after it (one host thread
// each, asleep on the GPU otherwise): a proof on its own then waits for ONE scalar multiplication after its MSMs (s A, r B1 side
// by side) instead of two in a row.
struct TailPre {
  bool started = false;
  uint64_t rc_[6], sc_[6], rsc_[6];
  std::future<host::HJac> rd1, sd2, sd1, rsd1;
  // A packaged_task's future does not block in its destructor (std::async's did): a proof that fails between tail_begin and
  // finish_impl must not return while a zk-tail worker still holds the key's tables.  The tasks themselves capture
  // their scalars BY VALUE, so nothing in the pool points into this object either.
  ~TailPre() {
    for (std::future<host::HJac>* f : {&rd1, &sd2, &sd1, &rsd1})
      if (f->valid()) f->wait();
  }
};
// The tail's scalar multiplications run on a small pool of host threads ("zk-tail"; round 5: rounds 2-4 started a std::async thread
// per multiplication - six thread creations per proof, 2,400 a second in a stream).  Tasks are ~0.15 ms (fixed-base, with the key's
// tables) or ~0.5 ms (s A, r B1: variable base); six threads serve the ~1.5 ms of them a proof needs at any rate one GPU sustains.
namespace {
class TailPool {
 public:
  // (never destroyed: its workers sleep on the condition variable for the life of the process, and destroying a condition variable
  //  that has waiters - what a static object's destructor would do at exit - blocks)
  static TailPool& get() { static TailPool* p = new TailPool(); return *p; }
  std::future<host::HJac> run(std::function<host::HJac()> fn) {
    auto task = std::make_shared<std::packaged_task<host::HJac()>>(std::move(fn));
    std::future<host::HJac> f = task->get_future();
    {
      std::lock_guard<std::mutex> lk(mu_);
      q_.push_back([task] { (*task)(); });
    }
    cv_.notify_one();
    return f;
  }
 private:
  TailPool() {
    const char* e = getenv("ZKHIP_TAIL_THREADS");
    int n = e ? atoi(e) : 6;
    if (n < 1 || n > 64) n = 6;
    for (int i = 0; i < n; i++) {
      std::thread([this] {
        pthread_setname_np(pthread_self(), "zk-tail");
        for (;;) {
          std::function<void()> job;
          {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return !q_.empty(); });
            job = std::move(q_.front());
            q_.pop_front();
          }
          job();
        }
      }).detach();                 // (process-lifetime workers: they sleep on the queue)
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
};
}  // namespace
struct TailScalar { uint64_t v[6]; };
static TailScalar tail_scalar(const uint64_t* k) { TailScalar t; memcpy(t.v, k, sizeof t.v); return t; }
static std::future<host::HJac> tail_smul(host::HJac p, const uint64_t* k) {
  const TailScalar kv = tail_scalar(k);
  return TailPool::get().run([p, kv]() { return p.mul_canonical(kv.v, 6); });
}
// tab: the key's fixed-base tables (null: the plain zkhip_groth16_finish, which is handed raw points: variable-base products)
static void tail_begin(TailPre& tp, const uint64_t delta_g1[24], const uint64_t delta_g2[24], const uint64_t r_m[6], const uint64_t s_m[6],
                       const TailTables* tab = nullptr) {
  using namespace host;
  HFr r = HFr::from_limbs(r_m), s = HFr::from_limbs(s_m), rs = r * s;
  r.to_canonical(tp.rc_); s.to_canonical(tp.sc_); rs.to_canonical(tp.rsc_);
  if (tab) {
    const TailScalar rc = tail_scalar(tp.rc_), sc = tail_scalar(tp.sc_), rsc = tail_scalar(tp.rsc_);
    tp.rd1 = TailPool::get().run([tab, rc] { return tab->d1.mul(rc.v); });
    tp.sd2 = TailPool::get().run([tab, sc] { return tab->d2.mul(sc.v); });
    tp.sd1 = TailPool::get().run([tab, sc] { return tab->d1.mul(sc.v); });
    tp.rsd1 = TailPool::get().run([tab, rsc] { return tab->d1.mul(rsc.v); });
  } else {
    auto aff = [](const uint64_t* p) { return HJac::from_affine(HFq::from_limbs(p), HFq::from_limbs(p + 12)); };
    const HJac d1 = aff(delta_g1), d2 = aff(delta_g2);
    tp.rd1 = tail_smul(d1, tp.rc_); tp.sd2 = tail_smul(d2, tp.sc_); tp.sd1 = tail_smul(d1, tp.sc_); tp.rsd1 = tail_smul(d1, tp.rsc_);
  }
  tp.started = true;
}
// the key's tables for r delta_1, s delta_1, r s delta_1, s delta_2 (built once, by the key's first proof)
static const TailTables* crs_tail_tables(const zkhip_crs* c) {
  std::call_once(c->tail_once, [c] {
    using namespace host;
    auto aff = [](const uint64_t* p) { return HJac::from_affine(HFq::from_limbs(p), HFq::from_limbs(p + 12)); };
    std::unique_ptr<TailTables> t(new TailTables());
    t->d1.build(aff(c->delta_g1));
    t->d2.build(aff(c->delta_g2));
    c->tail = std::move(t);
  });
  return (c->tail->d1.ok && c->tail->d2.ok) ? c->tail.get() : nullptr;       // (not ok: variable-base products in tail_begin)
}

static int finish_impl(const uint64_t alpha_g1[24], const uint64_t beta_g1[24], const uint64_t beta_g2[24], const uint64_t delta_g1[24],
                       const uint64_t delta_g2[24], const uint64_t sums_jac[180], const uint64_t r_m[6], const uint64_t s_m[6],
                       uint64_t proof_affine[72], double* tail_ms, TailPre* pre = nullptr) {
  using namespace host;
  if (!alpha_g1 || !beta_g1 || !beta_g2 || !delta_g1 || !delta_g2 || !sums_jac || !r_m || !s_m || !proof_affine) return fail(ZKHIP_ERR_ARG, "null pointer");
  auto t0 = clk::now();
  const uint64_t *evA = sums_jac, *evB2 = sums_jac + 36, *evB1 = sums_jac + 72, *evH = sums_jac + 108, *evL = sums_jac + 144;
  auto jac = [](const uint64_t* p) { HJac q; q.X = HFq::from_limbs(p); q.Y = HFq::from_limbs(p + 12); q.Z = HFq::from_limbs(p + 24); return q; };
  auto aff = [](const uint64_t* p) { return HJac::from_affine(HFq::from_limbs(p), HFq::from_limbs(p + 12)); };
  TailPre local;
  TailPre& tp = (pre && pre->started) ? *pre : local;
  if (!tp.started) tail_begin(tp, delta_g1, delta_g2, r_m, s_m);       // (the plain zkhip_groth16_finish: nothing was started ahead)
  HJac gA = jac(evA).add(aff(alpha_g1)).add(tp.rd1.get());
  auto f_sA = tail_smul(gA, tp.sc_);
  HJac gB1 = jac(evB1).add(aff(beta_g1)).add(tp.sd1.get());
  auto f_rB1 = tail_smul(gB1, tp.rc_);
  HJac gB2 = jac(evB2).add(aff(beta_g2)).add(tp.sd2.get());
  HJac gC = jac(evH).add(jac(evL)).add(f_sA.get()).add(f_rB1.get()).add(tp.rsd1.get().neg());
  HFq x, y;
  gA.to_affine(x, y); x.to_limbs(proof_affine); y.to_limbs(proof_affine + 12);
  gB2.to_affine(x, y); x.to_limbs(proof_affine + 24); y.to_limbs(proof_affine + 36);
  gC.to_affine(x, y); x.to_limbs(proof_affine + 48); y.to_limbs(proof_affine + 60);
  if (tail_ms) *tail_ms = ms_since(t0);
  return ZKHIP_OK;
}

static int prover_new_impl(const zkhip_crs* crs, const zkhip_r1cs_desc* cs, bool slice, size_t a_lo, size_t h_lo, size_t l_lo, zkhip_prover** out) {
  if (!crs || !cs || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(crs);
  R1csDev* rd = nullptr;
  {
    std::lock_guard<std::mutex> lk(g.dev[crs->device].mu);
    if (crs->n_vars != cs->n_vars || crs->n_primary != cs->n_primary) return fail(ZKHIP_ERR_ARG, "proving key and constraint system do not match");
    int rc = r1cs_upload(cs, crs->domain_size, &rd, t_err, sizeof t_err);     // the key's domain, whichever kind (domain.hpp)
    if (rc != ZKHIP_OK) return rc;
  }
  const size_t m = rd->n_vars, l = rd->n_primary, d = rd->d;
  bool ok = crs->n_vars == m && crs->n_primary == l && crs->domain_size == d;
  if (ok && !slice) ok = crs->A->len == m && crs->H->len == d - 1 && crs->L->len == m - l - 1;
  if (ok && slice) ok = a_lo + crs->A->len <= m && h_lo + crs->H->len <= d - 1 && l_lo + crs->L->len <= m - l - 1;
  if (!ok) {
    r1cs_free(rd);
    return fail(ZKHIP_ERR_ARG, slice ? "key slice out of range for this constraint system" : "proving key and constraint system do not match");
  }
  zkhip_prover* p = new zkhip_prover();
  p->device = crs->device;
  p->crs = crs; p->rd = rd;
  p->slice = slice; p->a_lo = a_lo; p->h_lo = h_lo; p->l_lo = l_lo;
  *out = p;
  return ZKHIP_OK;
}

static int prover_prove_impl(zkhip_prover* p, const uint64_t* z, const uint64_t* d_z, const uint64_t r_m[6], const uint64_t s_m[6], uint64_t proof_affine[72],
                             const zkhip_aggregator_app* app = nullptr) {
  if (!p || !r_m || !s_m || !proof_affine) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (p->slice) return fail(ZKHIP_ERR_STATE, "this prover holds a slice of the key: zkhip_prover_prove_partial");
  BIND(p);                                    // called from pipeline / application threads that never ran zkhip_init
  std::lock_guard<std::mutex> lk(p->mu);
  uint64_t sums[180];
  const zkhip_crs* c = p->crs;
  { int rc_ = prove_check(c, p->rd, 0, 0, 0); if (rc_ != ZKHIP_OK) return rc_; }
  p->refusal_kind = 0; p->refusal_index = 0;
  if (app) { int rc_ = app_check(app, c, p->checked ? nullptr : z); if (rc_ != ZKHIP_OK) return rc_; }   // (checked: the device reports the mask, with its index)
  TailPre pre;
  tail_begin(pre, c->delta_g1, c->delta_g2, r_m, s_m, crs_tail_tables(c));             // the key-only part of the tail runs under the device work
  int rc = prove_partial(p->ps, p->crs, p->rd, z, 0, 0, 0, sums, d_z, app ? app->d_z_app : nullptr);
  if (rc != ZKHIP_OK) return rc;
  if (p->checked && (rc = prover_refusal(p)) != ZKHIP_OK) return rc;      // (the MSMs of a refused proof ran; their sums are dropped)
  if (app) app_add_points(app, sums);
  return finish_impl(c->alpha_g1, c->beta_g1, c->beta_g2, c->delta_g1, c->delta_g2, sums, r_m, s_m, proof_affine, &p->ps.ms[7], &pre);
}

#pragma GCC visibility pop

extern "C" {

int zkhip_last_prove_timings(double out_ms[8]) {
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();
  if (!out_ms || dev < 0) return ZKHIP_ERR_ARG;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  memcpy(out_ms, g.dev[dev].ps.ms, sizeof g.dev[0].ps.ms);
  return ZKHIP_OK;
}

extern "C" int zkhip_set_prove_split(int mode) {
  if (mode < 0 || mode > 2) return fail(ZKHIP_ERR_ARG, "prove split: 0 (one launch sequence), 1 (two, gated) or 2 (two, not gated)");
  g_prove_split.store(mode);
  return ZKHIP_OK;
}

int zkhip_groth16_prove_partial(const zkhip_crs* crs_slice, zkhip_r1cs* r1cs, const uint64_t* z, size_t a_lo, size_t h_lo, size_t l_lo,
                                uint64_t sums_jac[180]) {
  if (!crs_slice || !r1cs || !z || !sums_jac) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (crs_slice->device != r1cs->device) return fail(ZKHIP_ERR_ARG, "proving key and constraint system live on different devices");
  BIND(crs_slice);
  std::lock_guard<std::mutex> lk(g.dev[crs_slice->device].mu);
  { int rc_ = follow_key_domain(crs_slice, r1cs->dev); if (rc_ != ZKHIP_OK) return rc_; }
  return prove_partial(g.dev[crs_slice->device].ps, crs_slice, r1cs->dev, z, a_lo, h_lo, l_lo, sums_jac);
}

int zkhip_groth16_finish(const uint64_t alpha_g1[24], const uint64_t beta_g1[24], const uint64_t beta_g2[24], const uint64_t delta_g1[24],
                         const uint64_t delta_g2[24], const uint64_t sums_jac[180], const uint64_t r_m[6], const uint64_t s_m[6],
                         uint64_t proof_affine[72]) {
  double tail_ms = 0;
  const int rc = finish_impl(alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, sums_jac, r_m, s_m, proof_affine, &tail_ms);
  const int dev = cur_dev();
  if (rc == ZKHIP_OK && dev >= 0) { std::lock_guard<std::mutex> lk(g.dev[dev].mu); g.dev[dev].ps.ms[7] = tail_ms; }
  return rc;
}

int zkhip_groth16_prove(const zkhip_crs* crs, zkhip_r1cs* r1cs, const uint64_t* z, const uint64_t r_m[6], const uint64_t s_m[6],
                        uint64_t proof_affine[72]) {
  uint64_t sums[180];
  if (!crs || !r1cs || !z || !r_m || !s_m || !proof_affine) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (crs->device != r1cs->device) return fail(ZKHIP_ERR_ARG, "proving key and constraint system live on different devices");
  BIND(crs);
  TailPre pre;
  {
    std::lock_guard<std::mutex> lk(g.dev[crs->device].mu);
    { int rc_ = follow_key_domain(crs, r1cs->dev); if (rc_ != ZKHIP_OK) return rc_; }
    const size_t m = r1cs->dev->n_vars, l = r1cs->dev->n_primary, d = r1cs->dev->d;
    if (crs->A->len != m || crs->H->len != d - 1 || crs->L->len != m - l - 1) return fail(ZKHIP_ERR_ARG, "proving key and constraint system do not match");
    { int rc_ = prove_check(crs, r1cs->dev, 0, 0, 0); if (rc_ != ZKHIP_OK) return rc_; }
    tail_begin(pre, crs->delta_g1, crs->delta_g2, r_m, s_m, crs_tail_tables(crs));       // the key-only part of the tail runs under the device work
    int rc = prove_partial(g.dev[crs->device].ps, crs, r1cs->dev, z, 0, 0, 0, sums);
    if (rc != ZKHIP_OK) return rc;
  }
  t_prove_dev = crs->device;      // zkhip_last_prove_timings reads the device of this thread's last proof
  double tail_ms = 0;
  const int rc = finish_impl(crs->alpha_g1, crs->beta_g1, crs->beta_g2, crs->delta_g1, crs->delta_g2, sums, r_m, s_m, proof_affine, &tail_ms, &pre);
  if (rc == ZKHIP_OK) { std::lock_guard<std::mutex> lk(g.dev[crs->device].mu); g.dev[crs->device].ps.ms[7] = tail_ms; }   // (two threads may prove through this entry point)
  return rc;
}

int zkhip_prover_new(const zkhip_crs* crs, const zkhip_r1cs_desc* cs, zkhip_prover** out) { return prover_new_impl(crs, cs, false, 0, 0, 0, out); }
int zkhip_prover_new_slice(const zkhip_crs* crs_slice, const zkhip_r1cs_desc* cs, size_t a_lo, size_t h_lo, size_t l_lo, zkhip_prover** out) {
  return prover_new_impl(crs_slice, cs, true, a_lo, h_lo, l_lo, out);
}

void zkhip_prover_free(zkhip_prover* p) {
  if (!p) return;
  (void)bind_dev(p->device);
  p->ps.release();
  r1cs_free(p->rd);
  delete p;
}

int zkhip_prover_prove(zkhip_prover* p, const uint64_t* z, const uint64_t r_m[6], const uint64_t s_m[6], uint64_t proof_affine[72]) {
  if (!z) return fail(ZKHIP_ERR_ARG, "null pointer");
  return prover_prove_impl(p, z, nullptr, r_m, s_m, proof_affine);
}
int zkhip_prover_prove_dev(zkhip_prover* p, const void* d_z, const uint64_t r_m[6], const uint64_t s_m[6], uint64_t proof_affine[72]) {
  if (!d_z) return fail(ZKHIP_ERR_ARG, "null pointer");
  return prover_prove_impl(p, nullptr, (const uint64_t*)d_z, r_m, s_m, proof_affine);
}
int zkhip_prover_prove_partial(zkhip_prover* p, const uint64_t* z, uint64_t sums_jac[180]) {
  if (!p || !z || !sums_jac) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(p);
  std::lock_guard<std::mutex> lk(p->mu);
  return prove_partial(p->ps, p->crs, p->rd, z, p->a_lo, p->h_lo, p->l_lo, sums_jac);
}

int zkhip_prover_prove_app(zkhip_prover* p, const zkhip_aggregator_app* app, const uint64_t* z_masked, const uint64_t r_m[6], const uint64_t s_m[6],
                           uint64_t proof_affine[72]) {
  if (!z_masked || !app) return fail(ZKHIP_ERR_ARG, "null pointer");
  return prover_prove_impl(p, z_masked, nullptr, r_m, s_m, proof_affine, app);
}
int zkhip_prover_prove_app_dev(zkhip_prover* p, const zkhip_aggregator_app* app, const void* d_z_masked, const uint64_t r_m[6], const uint64_t s_m[6],
                               uint64_t proof_affine[72]) {
  if (!d_z_masked || !app) return fail(ZKHIP_ERR_ARG, "null pointer");
  return prover_prove_impl(p, nullptr, (const uint64_t*)d_z_masked, r_m, s_m, proof_affine, app);
}

int zkhip_groth16_prove_app(const zkhip_crs* crs, zkhip_r1cs* r1cs, const zkhip_aggregator_app* app, const uint64_t* z_masked, const uint64_t r_m[6],
                            const uint64_t s_m[6], uint64_t proof_affine[72]) {
  uint64_t sums[180];
  if (!crs || !r1cs || !app || !z_masked || !r_m || !s_m || !proof_affine) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (crs->device != r1cs->device) return fail(ZKHIP_ERR_ARG, "proving key and constraint system live on different devices");
  BIND(crs);
  { int rc_ = app_check(app, crs, z_masked); if (rc_ != ZKHIP_OK) return rc_; }
  TailPre pre;
  {
    std::lock_guard<std::mutex> lk(g.dev[crs->device].mu);
    { int rc_ = follow_key_domain(crs, r1cs->dev); if (rc_ != ZKHIP_OK) return rc_; }
    { int rc_ = prove_check(crs, r1cs->dev, 0, 0, 0); if (rc_ != ZKHIP_OK) return rc_; }
    tail_begin(pre, crs->delta_g1, crs->delta_g2, r_m, s_m, crs_tail_tables(crs));
    int rc = prove_partial(g.dev[crs->device].ps, crs, r1cs->dev, z_masked, 0, 0, 0, sums, nullptr, app->d_z_app);
    if (rc != ZKHIP_OK) return rc;
  }
  app_add_points(app, sums);
  t_prove_dev = crs->device;
  double tail_ms = 0;
  const int rc = finish_impl(crs->alpha_g1, crs->beta_g1, crs->beta_g2, crs->delta_g1, crs->delta_g2, sums, r_m, s_m, proof_affine, &tail_ms, &pre);
  if (rc == ZKHIP_OK) { std::lock_guard<std::mutex> lk(g.dev[crs->device].mu); g.dev[crs->device].ps.ms[7] = tail_ms; }
  return rc;
}

// The HIP runtime spreads streams over a fixed number of hardware queues in the order they are CREATED, and kernels of streams that
// share a queue do not overlap.  A streaming prover runs a whole proof on one stream (its launch sequence's main stream); its other two
// streams idle.  Created lazily by the provers' own threads at their first proofs - thirty-two threads at once - the busy streams land
// on the queues as the race decides: a pipeline whose busy streams crowd a few queues proves 8-10 % fewer proofs/s for as long as it
// lives (round 5: 391 against 425-434 proofs/s, instance after instance in one process; same clock, 10 % less power).  A caller
// that owns several instances therefore creates the streams itself, in two passes over the instances: which = 0 the stream that will be
// busy (consecutive creations go to different queues), which = 1 the two that idle.  The busy one and the first idle one are main and side of the
// launch sequence's lane (ProveState::lane, held until release()), the other is the QAP map's; each call makes what is missing, so one after the first proof makes nothing.
int zkhip_prover_create_streams(zkhip_prover* p, int which) {
  if (!p || which < 0 || which > 1) return fail(ZKHIP_ERR_ARG, "null prover or unknown pass");
  BIND(p);
  std::lock_guard<std::mutex> lk(p->mu);
  ProveState& ps = p->ps;
  if (which == 0) API_HIP(msm_lane_create_main(&ps.lane[ZK_MSM_SLOTS]));
  else {
    API_HIP(msm_lane_create_side(&ps.lane[ZK_MSM_SLOTS]));
    if (!ps.st) API_HIP(hipStreamCreateWithFlags(&ps.st, hipStreamNonBlocking));
    if (p->crs->table_model) API_HIP(msm_lane_create_main(&ps.lane[ZK_CTX_H]));      // (a key on the Edwards model: B-G2's sequence, behind every instance's G1 stream)
  }
  return ZKHIP_OK;
}

int zkhip_prover_set_streaming(zkhip_prover* p, int on) {
  if (!p) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(p->mu);
  // measured on the wrapping circuit: 212 -> 228 proofs/s with six provers in flight, 107 -> 98 one at a time
  p->ps.quad_below = on ? 1024u : 0u;
  p->rd->spmv_log_lanes = on ? (p->rd->spmv_log_lanes_alone < 2 ? p->rd->spmv_log_lanes_alone : 2) : p->rd->spmv_log_lanes_alone;
  for (int k = 0; k < ZK_CTX_TOTAL; k++) if (p->ps.ctx[k].planned) { p->ps.ctx[k].quad_below = on ? 1024u : 65536u; p->ps.ctx[k].one_stream = on ? 1 : 0; }
  return ZKHIP_OK;
}

int zkhip_prover_set_checked(zkhip_prover* p, int on) {
  if (!p) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (p->slice) return fail(ZKHIP_ERR_STATE, "a prover over a slice of the key has no checked form");
  BIND(p);
  std::lock_guard<std::mutex> lk(p->mu);
  const int rc = r1cs_set_checked(p->rd, on, t_err, sizeof t_err);
  if (rc == ZKHIP_OK) p->checked = on != 0;
  return rc;
}
int zkhip_prover_last_refusal(zkhip_prover* p, int* kind, size_t* index) {
  if (!p || !kind || !index) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(p->mu);
  *kind = p->refusal_kind;
  *index = p->refusal_index;
  return ZKHIP_OK;
}

int zkhip_prover_last_accumulate_entries(zkhip_prover* p, uint64_t* out) {
  if (!p || !out) return fail(ZKHIP_ERR_ARG, "null argument");
  BIND(p);
  std::lock_guard<std::mutex> lk(p->mu);
  return last_entries_of(p->ps, out);
}
float zkhip_prover_last_accumulate_ms(zkhip_prover* p) {
  if (!p) return 0.f;
  std::lock_guard<std::mutex> lk(p->mu);
  return p->ps.last_accumulate_ms;
}

int zkhip_prover_timings(zkhip_prover* p, double out_ms[8]) {
  if (!p || !out_ms) return ZKHIP_ERR_ARG;
  std::lock_guard<std::mutex> lk(p->mu);
  memcpy(out_ms, p->ps.ms, sizeof p->ps.ms);
  return ZKHIP_OK;
}

// 1: p's last proof was CHAINED (a streaming prover enqueues upload, QAP map and the five MSMs on one stream and waits once): slots [0]
// and [1] of zkhip_prover_timings then hold the time it took to ENQUEUE those phases, and the MSM slots the whole device time
int zkhip_prover_timings_chained(zkhip_prover* p) {
  if (!p) return 0;
  std::lock_guard<std::mutex> lk(p->mu);
  return p->ps.chained_last ? 1 : (p->ps.split_last ? 2 : 0);
}
// 1: the last proof of the plain entry points on this thread's device ran as two launch sequences (see prove_partial): slot [1] of
// zkhip_last_prove_timings is then the time to ENQUEUE the QAP map and both sequences, the MSM slots hold the device time of all of it
int zkhip_last_prove_split(void) {
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();
  if (dev < 0) return 0;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  return g.dev[dev].ps.split_last ? 1 : 0;
}

int zkhip_prover_last_table_model(zkhip_prover* p, int* out) {
  if (!p || !out) return fail(ZKHIP_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(p->mu);
  *out = p->ps.edw_last ? 1 : 0;
  return ZKHIP_OK;
}
int zkhip_last_prove_table_model(void) {
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();
  if (dev < 0) return 0;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  return g.dev[dev].ps.edw_last ? 1 : 0;
}

// Host only (no device needed): the prover's tail on the paths a healthy proof never takes.
//  (1) `rounds` proofs that FAIL between tail_begin and finish_impl: the TailPre goes out of scope with its four tasks queued and the
//      key's tables are freed straight after - under the CPU AddressSanitizer build (tools/sanitize/asan_host_tests.sh) a task that
//      outlives either is a use-after-scope / use-after-free report (packaged_task futures do not wait in ~future);
//  (2) a delta with a small-order component: FixedBase8 must refuse the table (ok == false) and the tail must fall back to
//      variable-base products that equal k P computed directly; a healthy table must equal the variable-base product too.
// g1 / g2: points of order r (the curve generators); small: a point of small order on G1's curve ((1, 0) has order 2).
int zkhip_internal_tail_selftest(const uint64_t g1[24], const uint64_t g2[24], const uint64_t small[24], int rounds) {
  using namespace host;
  if (!g1 || !g2 || !small || rounds < 0 || rounds > 100000) return fail(ZKHIP_ERR_ARG, "tail selftest: arguments");
  auto aff = [](const uint64_t* p) { return HJac::from_affine(HFq::from_limbs(p), HFq::from_limbs(p + 12)); };
  auto same = [](const HJac& a, const HJac& b) {
    if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
    HFq ax, ay, bx, by;
    a.to_affine(ax, ay); b.to_affine(bx, by);
    uint64_t l[4][12];
    ax.to_limbs(l[0]); ay.to_limbs(l[1]); bx.to_limbs(l[2]); by.to_limbs(l[3]);
    return !memcmp(l[0], l[2], 96) && !memcmp(l[1], l[3], 96);
  };
  uint64_t r_m[6], s_m[6];
  HFr::from_u64(0x1234567u).to_limbs(r_m);
  (HFr::from_u64(0x89abcdefu) * HFr::from_u64(0xfedcba98u) * HFr::from_u64(0x76543211u)).to_limbs(s_m);
  for (int i = 0; i < rounds; i++) {
    std::unique_ptr<TailTables> tab(new TailTables());
    tab->d1.build(aff(g1));
    tab->d2.build(aff(g2));
    if (!tab->d1.ok || !tab->d2.ok) return fail(ZKHIP_ERR_STATE, "tail selftest: a prime-order table was refused");
    {
      TailPre pre;
      tail_begin(pre, g1, g2, r_m, s_m, tab.get());
    }                                            // "prove_partial failed": nobody collects the futures
    tab.reset();                                 // "the caller frees the key"
    {
      TailPre pre;
      tail_begin(pre, g1, g2, r_m, s_m);         // the variable-base form (zkhip_groth16_finish), abandoned the same way
    }
  }
  // healthy table = variable base, on a full-size scalar
  uint64_t k[6];
  HFr::from_limbs(s_m).to_canonical(k);
  FixedBase8 t1;
  t1.build(aff(g1));
  if (!t1.ok || !same(t1.mul(k), aff(g1).mul_canonical(k, 6))) return fail(ZKHIP_ERR_STATE, "tail selftest: fixed-base table differs from k P");
  // a small-order point: table refused ...
  FixedBase8 t2;
  t2.build(aff(small));
  if (t2.ok) return fail(ZKHIP_ERR_STATE, "tail selftest: the table of a small-order point was accepted");
  // ... and the tail, handed such a delta_1 through a KEY's tables (null: refused), equals the direct computation: with zero sums
  // and alpha = g1 the proof's A is g1 + r delta_1
  TailTables bad;
  bad.d1.build(aff(small)); bad.d2.build(aff(g2));
  const TailTables* usable = (bad.d1.ok && bad.d2.ok) ? &bad : nullptr;           // (what crs_tail_tables returns)
  if (usable) return fail(ZKHIP_ERR_STATE, "tail selftest: unusable tables were offered to the tail");
  uint64_t sums[180] = {0}, proof[72];
  TailPre pre;
  tail_begin(pre, small, g2, r_m, s_m, usable);
  const int rc = finish_impl(g1, g1, g2, small, g2, sums, r_m, s_m, proof, nullptr, &pre);
  if (rc != ZKHIP_OK) return rc;
  uint64_t rc_k[6];
  HFr::from_limbs(r_m).to_canonical(rc_k);
  if (!same(aff(proof), aff(g1).add(aff(small).mul_canonical(rc_k, 6)))) return fail(ZKHIP_ERR_STATE, "tail selftest: g1 + r delta_1 of a small-order delta_1 is wrong");
  return ZKHIP_OK;
}

}  // extern "C"
