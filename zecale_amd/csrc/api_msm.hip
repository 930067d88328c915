// C ABI (include/zkhip.h): base sets and their window tables, MSMs (plain, slots, handle-owned streams), fixed-base products.
#include <stdlib.h>
#include <string.h>

#include "api_internal.hpp"
#include "ec.cuh"

using namespace zkhip::api;

#pragma GCC visibility push(hidden)      // this file's own helpers and handle structs

namespace {
int auto_window(size_t n) {
  if (g.forced_c.load()) return g.forced_c.load();
  if (n <= (1u << 10)) return 8;
  if (n <= (1u << 13)) return 10;
  if (n <= (1u << 16)) return 12;
  if (n <= (1u << 18)) return 14;
  return 16;
}
// one MSM over `len` bases of b from `offset` on: slices sized by len (no finite-bases bound), the Edwards table from the same point
MsmJob single_job(const zkhip_bases* b, size_t offset, const void* d_scalars, size_t len, int scalars_mode) {
  return MsmJob{b->d_pts + offset, b->d_inf ? b->d_inf + offset : nullptr, (const uint64_t*)d_scalars, len, scalars_mode, b->len, 0, msm_edw_at(b->d_edw, offset)};
}
}  // namespace

namespace zkhip {
namespace api {
// window size of a table (one shared bucket window: the reduction is W times cheaper, so c is larger than auto_window's)
int auto_table_window(size_t n) {
  if (n <= (1u << 10)) return 9;
  if (n <= (1u << 13)) return 12;
  if (n <= (1u << 15)) return 14;
  if (n <= (1u << 17)) return 16;
  if (n <= (1u << 19)) return 18;
  if (n <= (1u << 21)) return 20;
  return 21;
}

// The plan of an MSM.  table_c = 0: plain plan with the automatic window;  > 0: merged plan (bases are a window table built for table_c)
static int plan_window(size_t n, int table_c, int plain_c) { return table_c ? table_c : (plain_c ? plain_c : auto_window(n)); }
static int plan_merged(int table_c, int naf) { return table_c ? (naf ? 2 : 1) : 0; }
// would ensure_ctx keep this context as it is (same plan, nothing pending)?  total: bound on the terms of all K jobs together (0: K * n)
bool ctx_reusable(const MsmCtx* cx, size_t n, int table_c, int K, int naf, size_t total, int plain_c) {
  if (total == 0 || total > (size_t)K * n) total = (size_t)K * n;
  return cx->planned && !cx->pending && cx->max_n >= n && cx->total_terms >= total && cx->c == plan_window(n, table_c, plain_c) &&
         cx->merged == plan_merged(table_c, naf) && cx->K == K && cx->aff_forced == msm_forced_aff_levels();
}
// lane: cx's, held by the owner of cx.  What it lacks is made here - main, then side (not for a plan that starts as one_stream: an idle stream still takes
// a place in the runtime's round over its hardware queues), then the events -; a plan made again (a longer MSM) finds everything there and stays where it ran.
int ensure_ctx(MsmCtx* cx, MsmLane& lane, size_t n, int table_c, int K, int naf, size_t total, int plain_c, int one_stream) {
  if (cx->pending) return fail(ZKHIP_ERR_STATE, "an MSM submitted on this context has not been collected (zkhip_msm_collect)");
  if (ctx_reusable(cx, n, table_c, K, naf, total, plain_c)) return ZKHIP_OK;
  if (cx->planned) msm_plan_free(cx);
  (void)msm_time_base();      // (recorded on the null stream the first time: before the lane's streams, as ever)
  API_HIP(msm_lane_create_main(&lane));
  if (!msm_one_stream(one_stream)) API_HIP(msm_lane_create_side(&lane));
  API_HIP(msm_lane_create_events(&lane));
  const int rc = msm_plan_init(cx, &lane, n, plan_window(n, table_c, plain_c), plan_merged(table_c, naf), K, total, one_stream);
  if (rc != ZKHIP_OK) { snprintf(t_err, sizeof t_err, "msm_plan_init: %s", cx->errbuf); msm_plan_free(cx); }   // (frees what the failed plan had allocated: "no plan" again)
  return rc;
}
// the last accumulation launch of ps ran on cx (zkhip_last_accumulate_ms / _interval / _entries read it back)
void note_last_acc(ProveState& ps, MsmCtx* cx) {
  ps.last_acc_ctx = cx; ps.last_accumulate_ms = cx->last_accumulate_ms;
  ps.last_acc_ctx2 = nullptr;      // (a proof of two sequences names its second plan after this call)
  ps.last_acc_interval[0] = cx->last_acc_begin_ms; ps.last_acc_interval[1] = cx->last_acc_end_ms;
}

static std::atomic<int> g_table_naf{-1};       // -1: the environment decides (default off); see naf_tables_wanted
// Which kind of table: one level per window (default), or every bit position (378 levels) with the scalars recoded in width-(c+1)
// non-adjacent form - an eighth fewer additions per scalar over the same buckets, sixteen times the table.  MEASURED (DESIGN.md
// section 5): the wrapping key (17.6 GB of tables instead of 1.2) gains 4.5 % in a stream of proofs and loses 5 % alone - its
// accumulation launch shrinks by 2 %, not 12: every addition gathers its point from a table that no longer fits the TLB's reach;
// a 2^20-point set (76 GB) LOSES 24 %.  So it is an option (zkhip_set_table_naf / ZKHIP_TABLE_NAF=1, within ZKHIP_NAF_TABLE_GB,
// default 48 GB per base set or proving key), off by default in the library (the streaming bench and the gRPC server
// switch it on for their key), tested like the default.
bool naf_tables_fit(size_t total_points) {
  static const double cap_gb = [] { const char* e = getenv("ZKHIP_NAF_TABLE_GB"); double v = e ? atof(e) : 48.0; return v > 0 ? v : 48.0; }();
  return (double)total_points * 378.0 * (double)(sizeof(AffPacked) + 1) <= cap_gb * 1e9 && total_points * 378 < ((size_t)1 << 31);
}
bool naf_tables_wanted(size_t total_points) {
  static const int env_on = [] { const char* e = getenv("ZKHIP_TABLE_NAF"); return e ? atoi(e) : 0; }();
  const int cur = g_table_naf.load();
  const int on = cur >= 0 ? cur : env_on;
  return on && naf_tables_fit(total_points);
}

int bases_precompute_mode(zkhip_bases* b, int c, int naf, bool edw) {
  if (!b) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(b);
  std::lock_guard<std::mutex> lk(g.dev[b->device].mu);
  if (b->table_c) return fail(ZKHIP_ERR_STATE, "base set already has a window table");
  if (c == 0) c = auto_table_window(b->len);
  if (c < 4 || c > 22) return fail(ZKHIP_ERR_ARG, "table window must be 0 (automatic) or in [4, 22]");
  if (b->len == 0) { b->table_c = c; b->table_naf = naf; return ZKHIP_OK; }
  const size_t levels = (size_t)msm_table_levels(c, naf);
  if (levels * b->len >= ((size_t)1 << 31)) return fail(ZKHIP_ERR_ARG, "table too large (levels * len must stay below 2^31)");
  AffPacked* tab = nullptr;
  uint8_t* tinf = nullptr;
  hipError_t e = hipMalloc(&tab, levels * b->len * sizeof(AffPacked));
  if (e == hipSuccess) e = hipMalloc(&tinf, levels * b->len);
  if (e == hipSuccess) e = hipMemcpy(tab, b->d_pts, b->len * sizeof(AffPacked), hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(tinf, b->d_inf, b->len, hipMemcpyDeviceToDevice);
  int rc = ZKHIP_OK;
  if (e != hipSuccess) { snprintf(t_err, sizeof t_err, "window table allocation: %s", hipGetErrorString(e)); rc = ZKHIP_ERR_HIP; }
  else rc = msm_table_build(tab, tinf, b->len, c, naf, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) { if (tab) (void)hipFree(tab); if (tinf) (void)hipFree(tinf); return rc; }
  (void)hipFree(b->d_pts); (void)hipFree(b->d_inf);
  b->d_pts = tab; b->d_inf = tinf; b->table_c = c; b->table_naf = naf;
  // the Edwards form (one level per window only, and not for tables forced onto batched-affine levels: their accumulation is XYZZ's).
  // It costs 1.5 x the table's memory for good (288-byte entries) and as much again while it is built (the halved table); it is built
  // only when that leaves a quarter of the device's memory free for plans and other sets.  A set that is not of order r on G1's curve
  // keeps the XYZZ path; any other failure is an error.
  if (edw && !naf && msm_forced_aff_levels() <= 0) {
    size_t mem_free = 0, mem_total = 0;
    const size_t need = levels * b->len * (sizeof(AffPacked) + 1 + 288) + ((size_t)1 << 21) * 432;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && mem_free >= need + mem_total / 4) {
      EdwPacked* et = nullptr;
      char e_err[256];
      rc = msm_table_edw(tab, tinf, b->len, c, &et, e_err, sizeof e_err);
      if (rc == ZKHIP_OK) b->d_edw = et;
      else if (rc == ZKHIP_ERR_HIP) { snprintf(t_err, sizeof t_err, "Edwards table: %s", e_err); return rc; }
      // (not an error: the set stays XYZZ and the call succeeds - but zkhip_last_error() says where to look)
      else snprintf(t_err, sizeof t_err, "Edwards table not built, the set keeps its XYZZ tables: %s - zkhip_crs_check reports which point of a key is not of order r", e_err);
    }
    (void)hipGetLastError();
  }
  return ZKHIP_OK;
}

int last_entries_of(ProveState& ps, uint64_t* out) {
  *out = 0;
  if (!ps.last_acc_ctx) return ZKHIP_OK;
  int rc = msm_last_entries(ps.last_acc_ctx, out);
  if (rc != ZKHIP_OK) return ctx_fail(rc, ps.last_acc_ctx);
  if (ps.last_acc_ctx2) {          // a split proof: two accumulation launches
    uint64_t more = 0;
    if ((rc = msm_last_entries(ps.last_acc_ctx2, &more)) != ZKHIP_OK) return ctx_fail(rc, ps.last_acc_ctx2);
    *out += more;
  }
  return ZKHIP_OK;
}
}  // namespace api
}  // namespace zkhip

static int bases_upload_dev_impl(const void* d_bases_affine, size_t len, zkhip_bases* b) {
  if (!len) return ZKHIP_OK;
  API_HIP(hipMalloc(&b->d_pts, len * sizeof(AffPacked)));
  API_HIP(hipMalloc(&b->d_inf, len));
  int rc = msm_bases_convert((const uint64_t*)d_bases_affine, len, b->d_pts, b->d_inf, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  std::vector<uint8_t> flags(len);
  API_HIP(hipMemcpy(flags.data(), b->d_inf, len, hipMemcpyDeviceToHost));
  size_t inf = 0;
  for (uint8_t f : flags) inf += f;
  b->n_finite = len - inf;
  return ZKHIP_OK;
}

// Which point model the single MSMs over a one-level-per-window table accumulate in: G1's 2-isogenous twisted
// Edwards curve (default; the table gets a second, precomputed Edwards form at precompute time), or XYZZ (ZKHIP_TABLE_MODEL=xyzz,
// zkhip_set_table_model(0): A/B runs).  A set whose points are not of order r on G1's curve (G2) stays XYZZ whatever is asked.
static std::atomic<int> g_table_model{-1};     // -1: the environment decides (default Edwards)
static bool edw_tables_wanted() {
  static const int env_model = [] { const char* e = getenv("ZKHIP_TABLE_MODEL"); return (e && strcmp(e, "xyzz") == 0) ? 0 : 1; }();
  const int cur = g_table_model.load();
  return (cur >= 0 ? cur : env_model) != 0;
}

// ---- handle-owned MSM streams ---------------------------------------------------------------------------------------------
// zkhip_msm_submit / collect above address eight PROCESS-WIDE slot numbers: two threads streaming MSMs on one device collide.  A
// zkhip_msm_stream owns its contexts (work space) and their lanes (streams, events), like a zkhip_prover: any number of them run side by side.
struct zkhip_msm_stream {
  int device = 0;
  const zkhip_bases* bases = nullptr;
  int depth = 0;
  std::vector<MsmCtx> ctx;               // (value-initialised: all zeros, no plan - msm.h)
  std::vector<MsmLane> lane;             // slot k's streams and events, from zkhip_msm_stream_new (layouts 1, 2) or its first submit to zkhip_msm_stream_free
  std::vector<uint64_t> ticket_of;       // per slot: the ticket in flight there, 0 = free
  std::vector<void*> d_stage;            // per slot: device copy of host scalars (zkhip_msm_stream_submit_host)
  std::vector<size_t> stage_cap;
  uint64_t next_ticket = 1;
  float last_accumulate_ms = 0.f, last_interval[2] = {0.f, 0.f};
  int layout = 0;                        // msm_stream_layout() when the stream was made
  std::mutex mu;
};

// How a zkhip_msm_stream places the HIP streams of its contexts on the runtime's hardware queues.  The runtime deals streams to its
// queues round robin in the order they are CREATED, and kernels of streams that share a queue do not overlap (the provers' finding:
// zkhip_prover_create_streams).  That is OBSERVED behaviour of the runtime (kernel traces, 4 queues), not a contract of HIP: the
// layouts differ in speed only, and if a runtime binds streams otherwise the gain goes and nothing else changes.
// A context's primary stream (its lane's main) carries its whole launch sequence, its secondary (side) only the column tree; the lanes are the stream's until zkhip_msm_stream_free: a slot planned again for a longer MSM stays where it is.
//   0  every context creates its pair at its first submit: p0 s0 p1 s1 .. - with an even number of queues every primary lands on
//      every second queue (profiles/msm_queues_before.txt: 16 of 20 accumulations on two of the four queues)
//   1  zkhip_msm_stream_new creates all primaries, consecutively, then all secondaries
//   2  primaries only: the contexts of a stream deeper than 1 run their whole sequence on the primary (MsmCtx::one_stream)
// ZKHIP_MSM_STREAM_LAYOUT, read once; zkhip_internal_set_msm_stream_layout overrides it for the streams made afterwards.
#define ZK_MSM_STREAM_LAYOUT_DEFAULT 1
static std::atomic<int> g_stream_layout{-1};
static int msm_stream_layout() {
  static const int env_layout = [] { const char* e = getenv("ZKHIP_MSM_STREAM_LAYOUT"); const int v = e ? atoi(e) : ZK_MSM_STREAM_LAYOUT_DEFAULT; return (v < 0 || v > 2) ? ZK_MSM_STREAM_LAYOUT_DEFAULT : v; }();
  const int cur = g_stream_layout.load();
  return cur >= 0 ? cur : env_layout;
}

static int msm_stream_submit_impl(zkhip_msm_stream* st, size_t offset, const void* d_scalars, const uint64_t* h_scalars, size_t len,
                                  int scalars_montgomery, uint64_t* ticket) {
  if (!st || !ticket || (len && !d_scalars && !h_scalars)) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(st);
  std::lock_guard<std::mutex> lk(st->mu);
  const zkhip_bases* b = st->bases;
  if (offset > b->len || len > b->len - offset) return fail(ZKHIP_ERR_ARG, "offset + len exceeds the base set");
  int slot = -1;
  for (int k = 0; k < st->depth; k++) if (!st->ticket_of[k]) { slot = k; break; }
  if (slot < 0) return fail(ZKHIP_ERR_STATE, "every slot of this stream is in flight: collect a result first");
  MsmCtx* cx = &st->ctx[slot];
  int rc = ensure_ctx(cx, st->lane[slot], len ? len : 1, b->table_c, 1, b->table_naf, 0, b->plain_c, (st->layout == 2 && st->depth > 1) ? 1 : -1);
  if (rc != ZKHIP_OK) return rc;
  if (h_scalars && len) {
    // host scalars: one asynchronous copy in front of the MSM's kernels, on the context's own stream (truly asynchronous from pinned
    // memory - zkhip_host_alloc -, staged by the runtime from pageable memory); the copies of the MSMs in flight overlap their kernels
    if (st->stage_cap[slot] < len) {
      if (st->d_stage[slot]) { (void)hipFree(st->d_stage[slot]); st->d_stage[slot] = nullptr; st->stage_cap[slot] = 0; }
      API_HIP(hipMalloc(&st->d_stage[slot], len * 48));
      st->stage_cap[slot] = len;
    }
    API_HIP(hipMemcpyAsync(st->d_stage[slot], h_scalars, len * 48, hipMemcpyHostToDevice, st->lane[slot].main));
    d_scalars = st->d_stage[slot];
  }
  const MsmJob job = single_job(b, offset, d_scalars, len, scalars_montgomery);
  if ((rc = msm_launch_multi(cx, 1, &job)) != ZKHIP_OK) return ctx_fail(rc, cx);
  st->ticket_of[slot] = st->next_ticket;
  *ticket = st->next_ticket++;
  return ZKHIP_OK;
}

#pragma GCC visibility pop

extern "C" {

int zkhip_set_msm_window(int c) {
  if (c != 0 && (c < 4 || c > 18)) return fail(ZKHIP_ERR_ARG, "window must be 0 or in [4, 18]");   // (tables: zkhip_bases_precompute takes up to 22)
  g.forced_c.store(c);
  return ZKHIP_OK;
}

int zkhip_bases_upload_dev(const void* d_bases_affine, size_t len, zkhip_bases** out) {
  BIND_CUR();
  if (!out || (len && !d_bases_affine)) return fail(ZKHIP_ERR_ARG, "null pointer");
  const int dev = cur_dev();
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  zkhip_bases* b = new zkhip_bases{nullptr, nullptr, len, 0, 0, len, dev, 0};
  int rc = bases_upload_dev_impl(d_bases_affine, len, b);
  if (rc != ZKHIP_OK) { zkhip_bases_free(b); return rc; }      // whatever was allocated before the failure
  *out = b;
  return ZKHIP_OK;
}

int zkhip_bases_upload(const uint64_t* bases_affine, size_t len, zkhip_bases** out) {
  BIND_CUR();
  if (!out || (len && !bases_affine)) return fail(ZKHIP_ERR_ARG, "null pointer");
  Scratch sc;
  void* d = nullptr;
  if (len) {
    API_HIP(sc.alloc(&d, len * 192));
    API_HIP(hipMemcpy(d, bases_affine, len * 192, hipMemcpyHostToDevice));
  }
  return zkhip_bases_upload_dev(d, len, out);
}

size_t zkhip_bases_len(const zkhip_bases* b) { return b ? b->len : 0; }

int zkhip_set_affine_levels(int levels) {
  if (levels < -1 || levels > MSM_MAX_AFF_LEVELS) return fail(ZKHIP_ERR_ARG, "levels must be -1 (automatic) or in [0, 4]");
  msm_force_aff_levels(levels);
  return ZKHIP_OK;
}
int zkhip_set_table_naf(int on) { g_table_naf.store(on < 0 ? -1 : (on ? 1 : 0)); return ZKHIP_OK; }
int zkhip_set_table_model(int model) { g_table_model.store(model < 0 ? -1 : (model ? 1 : 0)); return ZKHIP_OK; }
int zkhip_bases_table_model(const zkhip_bases* b) { return (b && b->d_edw) ? 1 : 0; }
int zkhip_bases_precompute(zkhip_bases* b, int c) {
  if (!b) return fail(ZKHIP_ERR_ARG, "null pointer");
  return bases_precompute_mode(b, c, naf_tables_wanted(b->len) ? 1 : 0, edw_tables_wanted());
}
int zkhip_bases_precompute_ex(zkhip_bases* b, int c, int table_naf) {
  if (!b) return fail(ZKHIP_ERR_ARG, "null pointer");
  const int naf = table_naf < 0 ? (naf_tables_wanted(b->len) ? 1 : 0) : ((table_naf && naf_tables_fit(b->len)) ? 1 : 0);
  return bases_precompute_mode(b, c, naf, edw_tables_wanted());
}
int zkhip_bases_table_window(const zkhip_bases* b) { return b ? b->table_c : 0; }
int zkhip_bases_set_window(zkhip_bases* b, int c) {
  if (!b) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (c != 0 && (c < 4 || c > 18)) return fail(ZKHIP_ERR_ARG, "window must be 0 (automatic) or in [4, 18]");
  std::lock_guard<std::mutex> lk(g.dev[b->device].mu);
  b->plain_c = c;
  return ZKHIP_OK;
}

void zkhip_bases_free(zkhip_bases* b) {
  if (!b) return;
  (void)bind_dev(b->device);
  if (b->d_pts) (void)hipFree(b->d_pts);
  if (b->d_inf) (void)hipFree(b->d_inf);
  if (b->d_edw) (void)hipFree(b->d_edw);
  delete b;
}

int zkhip_msm_dev(const zkhip_bases* bases, size_t offset, const void* d_scalars, size_t len, int scalars_montgomery,
                  uint64_t out_jac[36]) {
  if (!bases || !out_jac || (len && !d_scalars)) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(bases);
  ProveState& ps = g.dev[bases->device].ps;
  std::lock_guard<std::mutex> lk(g.dev[bases->device].mu);
  if (offset > bases->len || len > bases->len - offset) return fail(ZKHIP_ERR_ARG, "offset + len exceeds the base set");
  MsmCtx* cx = &ps.ctx[0];
  int rc = ensure_ctx(cx, ps.lane[0], len ? len : 1, bases->table_c, 1, bases->table_naf, 0, bases->plain_c);
  if (rc != ZKHIP_OK) return rc;
  const MsmJob job = single_job(bases, offset, d_scalars, len, scalars_montgomery);
  if ((rc = msm_launch_multi(cx, 1, &job)) == ZKHIP_OK) rc = msm_finish(cx, out_jac);
  if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
  note_last_acc(ps, cx); t_prove_dev = bases->device;
  return ZKHIP_OK;
}

// Asynchronous form: enqueue on one of the library's MSM contexts and return; collect later.  Two MSMs in flight overlap
// the latency-bound bucket reduction of one with the accumulation of the other (what the prover does between its own MSMs).
int zkhip_msm_submit(const zkhip_bases* bases, size_t offset, const void* d_scalars, size_t len, int scalars_montgomery, int slot) {
  if (!bases || (len && !d_scalars)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (slot < 0 || slot >= ZK_MSM_SLOTS) return fail(ZKHIP_ERR_ARG, "slot must be in [0, 7]");
  BIND(bases);
  ProveState& ps = g.dev[bases->device].ps;
  std::lock_guard<std::mutex> lk(g.dev[bases->device].mu);
  if (offset > bases->len || len > bases->len - offset) return fail(ZKHIP_ERR_ARG, "offset + len exceeds the base set");
  MsmCtx* cx = &ps.ctx[slot];
  if (cx->pending) return fail(ZKHIP_ERR_STATE, "slot busy: collect its result first");
  int rc = ensure_ctx(cx, ps.lane[slot], len ? len : 1, bases->table_c, 1, bases->table_naf, 0, bases->plain_c);
  if (rc != ZKHIP_OK) return rc;
  // a stream of MSMs, optionally GATED (ZKHIP_MSM_GATE=1): the accumulation of this one waits for the end of the accumulation
  // submitted before it on another slot, so that two accumulations never share the chip.  Measured (tools/gate_ab.sh, 2^20 terms,
  // eight in flight): 79.6 Mscalar/s gated against 83.7 free-running - the free overlap fills the tail of one accumulation with the
  // head of the next - so the default is off; the gate gives event-timed kernel durations that are per-launch costs.
  static const bool gate = getenv("ZKHIP_MSM_GATE") ? atoi(getenv("ZKHIP_MSM_GATE")) != 0 : false;
  const int prev = ps.last_submit_slot;
  cx->acc_gate = (gate && prev >= 0 && prev != slot && ps.ctx[prev].planned) ? ps.lane[prev].ev_acc1 : nullptr;
  const MsmJob job = single_job(bases, offset, d_scalars, len, scalars_montgomery);
  rc = msm_launch_multi(cx, 1, &job);
  cx->acc_gate = nullptr;                   // (the event belongs to another context: never kept beyond this launch)
  if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
  if (len) ps.last_submit_slot = slot;
  t_slot_dev[slot] = bases->device;         // zkhip_msm_collect(slot) has no handle: it collects where this thread submitted
  return ZKHIP_OK;
}

int zkhip_msm_collect(int slot, uint64_t out_jac[36]) {
  if (slot < 0 || slot >= ZK_MSM_SLOTS || !out_jac) return fail(ZKHIP_ERR_ARG, "bad slot or null pointer");
  const int dev = t_slot_dev[slot] >= 0 ? t_slot_dev[slot] : cur_dev();     // the device this thread submitted the slot on
  { int rc_ = bind_dev(dev); if (rc_ != ZKHIP_OK) return rc_; }
  ProveState& ps = g.dev[dev].ps;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  MsmCtx* cx = &ps.ctx[slot];
  if (!cx->pending) return fail(ZKHIP_ERR_STATE, "nothing submitted on this slot");
  const int rc = msm_finish(cx, out_jac);
  if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
  note_last_acc(ps, cx); t_prove_dev = dev;
  return ZKHIP_OK;
}

int zkhip_msm(const zkhip_bases* bases, size_t offset, const uint64_t* scalars, size_t len, int scalars_montgomery,
              uint64_t out_jac[36]) {
  if (!bases || (len && !scalars)) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(bases);
  Scratch sc;
  void* d = nullptr;
  if (len) {
    API_HIP(sc.alloc(&d, len * 48));
    API_HIP(hipMemcpy(d, scalars, len * 48, hipMemcpyHostToDevice));
    API_HIP(hipStreamSynchronize(0));     // the MSM streams are not ordered against the null stream
  }
  return zkhip_msm_dev(bases, offset, d, len, scalars_montgomery, out_jac);
}

int zkhip_msm_raw(const uint64_t* bases_affine, const uint64_t* scalars, size_t len, int scalars_montgomery,
                  uint64_t out_jac[36]) {
  zkhip_bases* b = nullptr;
  int rc = zkhip_bases_upload(bases_affine, len, &b);
  if (rc != ZKHIP_OK) return rc;
  rc = zkhip_msm(b, 0, scalars, len, scalars_montgomery, out_jac);
  zkhip_bases_free(b);
  return rc;
}

int zkhip_fixed_base_mul_dev(const uint64_t base_affine[24], const void* d_scalars, size_t len, int scalars_montgomery,
                             void* d_out_affine) {
  BIND_CUR();
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  if (!base_affine || (len && (!d_scalars || !d_out_affine))) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (len == 0) return ZKHIP_OK;
  return fixed_base_mul(base_affine, (const uint64_t*)d_scalars, len, scalars_montgomery, (uint64_t*)d_out_affine, t_err, sizeof t_err);
}

int zkhip_fixed_base_mul(const uint64_t base_affine[24], const uint64_t* scalars, size_t len, int scalars_montgomery,
                         uint64_t* out_affine) {
  BIND_CUR();
  if (len && (!scalars || !out_affine)) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (len == 0) return ZKHIP_OK;
  Scratch sc;
  void *ds = nullptr, *dp = nullptr;
  API_HIP(sc.alloc(&ds, len * 48));
  API_HIP(sc.alloc(&dp, len * 192));
  API_HIP(hipMemcpy(ds, scalars, len * 48, hipMemcpyHostToDevice));
  int rc = zkhip_fixed_base_mul_dev(base_affine, ds, len, scalars_montgomery, dp);
  if (rc == ZKHIP_OK) API_HIP(hipMemcpy(out_affine, dp, len * 192, hipMemcpyDeviceToHost));
  return rc;
}

int zkhip_last_accumulate_interval(float out_ms[2]) {
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();
  if (!out_ms || dev < 0) return ZKHIP_ERR_ARG;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  out_ms[0] = g.dev[dev].ps.last_acc_interval[0]; out_ms[1] = g.dev[dev].ps.last_acc_interval[1];
  return ZKHIP_OK;
}
int zkhip_last_accumulate_entries(uint64_t* out) {
  if (!out) return fail(ZKHIP_ERR_ARG, "null argument");
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();
  if (dev < 0) { *out = 0; return ZKHIP_OK; }
  { int rc_ = bind_dev(dev); if (rc_ != ZKHIP_OK) return rc_; }
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  return last_entries_of(g.dev[dev].ps, out);
}
float zkhip_last_accumulate_ms(void) {
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();       // where this thread's last MSM / proof ran
  if (dev < 0) return 0.f;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  return g.dev[dev].ps.last_accumulate_ms;
}
// The origin of zkhip_last_accumulate_interval's time base is recorded again, now: the values are FLOAT milliseconds since the origin,
// so a caller that compares intervals (bench.py's union of overlapping launches) re-bases at the start of its timed region.
int zkhip_reset_time_base(void) {
  BIND_CUR();
  return msm_time_base_reset();
}

int zkhip_msm_stream_new(const zkhip_bases* bases, int depth, zkhip_msm_stream** out) {
  if (!bases || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (depth < 1 || depth > 16) return fail(ZKHIP_ERR_ARG, "depth must be in [1, 16]");
  BIND(bases);
  zkhip_msm_stream* st = new zkhip_msm_stream();
  st->device = bases->device; st->bases = bases; st->depth = depth;
  st->ctx.resize(depth); st->lane.resize(depth); st->ticket_of.assign(depth, 0);
  st->d_stage.assign(depth, nullptr); st->stage_cap.assign(depth, 0);
  st->layout = msm_stream_layout();
  // two passes, as zkhip_prover_create_streams: every primary stream first - consecutive creations go to different hardware
  // queues -, then the secondaries (none when the contexts keep to their primary); layout 0 leaves both to the slots' first submits
  hipError_t e = hipSuccess;
  for (int k = 0; k < depth && st->layout && e == hipSuccess; k++) e = msm_lane_create_main(&st->lane[k]);
  for (int k = 0; k < depth && (st->layout == 1 || (st->layout == 2 && depth == 1)) && e == hipSuccess; k++) e = msm_lane_create_side(&st->lane[k]);
  if (e != hipSuccess) {
    snprintf(t_err, sizeof t_err, "zkhip_msm_stream_new: %s", hipGetErrorString(e));
    zkhip_msm_stream_free(st);
    return ZKHIP_ERR_HIP;
  }
  *out = st;
  return ZKHIP_OK;
}

void zkhip_msm_stream_free(zkhip_msm_stream* st) {
  if (!st) return;
  (void)bind_dev(st->device);
  for (MsmCtx& c : st->ctx) if (c.pending) { uint64_t drop[36]; (void)msm_finish(&c, drop); }      // never free work space or a lane under a running launch
  for (MsmCtx& c : st->ctx) if (c.planned) msm_plan_free(&c);
  for (MsmLane& l : st->lane) msm_lane_free(&l);
  for (void* p : st->d_stage) if (p) (void)hipFree(p);
  delete st;
}

int zkhip_msm_stream_submit(zkhip_msm_stream* st, size_t offset, const void* d_scalars, size_t len, int scalars_montgomery, uint64_t* ticket) {
  return msm_stream_submit_impl(st, offset, d_scalars, nullptr, len, scalars_montgomery, ticket);
}
int zkhip_msm_stream_submit_host(zkhip_msm_stream* st, size_t offset, const uint64_t* scalars, size_t len, int scalars_montgomery, uint64_t* ticket) {
  return msm_stream_submit_impl(st, offset, nullptr, scalars, len, scalars_montgomery, ticket);
}

int zkhip_msm_stream_collect(zkhip_msm_stream* st, uint64_t ticket, uint64_t out_jac[36]) {
  if (!st || !out_jac) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(st);
  std::lock_guard<std::mutex> lk(st->mu);
  int slot = -1;
  for (int k = 0; k < st->depth; k++) {
    if (!st->ticket_of[k]) continue;
    if (ticket ? st->ticket_of[k] == ticket : (slot < 0 || st->ticket_of[k] < st->ticket_of[slot])) slot = k;    // ticket 0: the oldest
  }
  if (slot < 0) return fail(ZKHIP_ERR_STATE, ticket ? "no such ticket in flight on this stream" : "nothing in flight on this stream");
  MsmCtx* cx = &st->ctx[slot];
  st->ticket_of[slot] = 0;                  // (msm_finish clears `pending` whatever it returns: the slot is free again)
  const int rc = msm_finish(cx, out_jac);
  if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
  st->last_accumulate_ms = cx->last_accumulate_ms; st->last_interval[0] = cx->last_acc_begin_ms; st->last_interval[1] = cx->last_acc_end_ms;
  return ZKHIP_OK;
}
float zkhip_msm_stream_last_accumulate_ms(zkhip_msm_stream* st) {
  if (!st) return 0.f;
  std::lock_guard<std::mutex> lk(st->mu);
  return st->last_accumulate_ms;
}
int zkhip_msm_stream_last_accumulate_interval(zkhip_msm_stream* st, float out_ms[2]) {
  if (!st || !out_ms) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(st->mu);
  out_ms[0] = st->last_interval[0]; out_ms[1] = st->last_interval[1];
  return ZKHIP_OK;
}

int zkhip_measure_fq_mul_rate(double* fq_mul_per_s) {
  BIND_CUR();
  if (!fq_mul_per_s) return fail(ZKHIP_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return msm_measure_fqmul_rate(fq_mul_per_s, t_err, sizeof t_err);
}

// Test hooks of the lockstep route of the Edwards accumulation (msm.hip k_accumulate_edw_lock)
int zkhip_internal_set_lockstep(int mode, int min_buckets) {
  msm_force_lockstep(mode, min_buckets);
  return ZKHIP_OK;
}
// Test / A-B hook of the stream layout of a zkhip_msm_stream (above)
int zkhip_internal_set_msm_stream_layout(int layout) {
  if (layout < -1 || layout > 2) return fail(ZKHIP_ERR_ARG, "layout must be -1 (the environment), 0, 1 or 2");
  g_stream_layout.store(layout);
  return ZKHIP_OK;
}
int zkhip_internal_last_acc_path(int* out) {
  if (!out) return fail(ZKHIP_ERR_ARG, "null argument");
  *out = -1;
  const int dev = t_prove_dev >= 0 ? t_prove_dev : cur_dev();
  if (dev < 0) return ZKHIP_OK;
  { int rc_ = bind_dev(dev); if (rc_ != ZKHIP_OK) return rc_; }
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  MsmCtx* cx = g.dev[dev].ps.last_acc_ctx;
  if (!cx) return ZKHIP_OK;
  const int rc = msm_last_acc_path(cx, out);
  return rc == ZKHIP_OK ? rc : ctx_fail(rc, cx);
}

// Test hook of the merged launch (msm.hip msm_launch_multi): up to four table-backed sets of one window through ONE launch sequence
int zkhip_internal_msm_multi(const zkhip_bases* const* sets, const uint64_t* const* scalars, const size_t* n, int K, int montgomery, int model,
                             int* acc_path, uint64_t* out_jac) {
  if (!sets || !scalars || !n || !acc_path || !out_jac) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (K < 1 || K > 4 || (model != 0 && model != 1)) return fail(ZKHIP_ERR_ARG, "K in 1 .. 4, model 0 (XYZZ) or 1 (Edwards)");
  for (int k = 0; k < K; k++) if (!sets[k] || (n[k] && !scalars[k])) return fail(ZKHIP_ERR_ARG, "null pointer");
  const int dev = sets[0]->device, tc = sets[0]->table_c;
  size_t max_n = 1, total = 0;
  for (int k = 0; k < K; k++) {
    const zkhip_bases* b = sets[k];
    if (b->device != dev) return fail(ZKHIP_ERR_ARG, "the sets live on different devices");
    if (!b->table_c || b->table_c != tc || b->table_naf) return fail(ZKHIP_ERR_ARG, "the sets must have one-level-per-window tables of one window");
    if (n[k] > b->len) return fail(ZKHIP_ERR_ARG, "more terms than the set has bases");
    if (model == 1 && n[k] && !b->d_edw) return fail(ZKHIP_ERR_STATE, "a set without an Edwards form cannot join an Edwards launch");
    if (n[k] > max_n) max_n = n[k];
    total += n[k];
  }
  BIND(sets[0]);
  ProveState& ps = g.dev[dev].ps;
  std::lock_guard<std::mutex> lk(g.dev[dev].mu);
  Scratch sc;
  MsmJob jobs[4];
  for (int k = 0; k < K; k++) {
    void* d = nullptr;
    if (n[k]) {
      API_HIP(sc.alloc(&d, n[k] * 48));
      API_HIP(hipMemcpy(d, scalars[k], n[k] * 48, hipMemcpyHostToDevice));
    }
    jobs[k] = single_job(sets[k], 0, d, n[k], montgomery);
    if (model == 0) jobs[k].edw = nullptr;
  }
  API_HIP(hipStreamSynchronize(0));     // the MSM streams are not ordered against the null stream
  MsmCtx* cx = &ps.ctx[ZK_CTX_Z];
  int rc = ensure_ctx(cx, ps.lane[ZK_CTX_Z], max_n, tc, K, 0, total ? total : 1);
  if (rc != ZKHIP_OK) return rc;
  if ((rc = msm_launch_multi(cx, K, jobs)) == ZKHIP_OK) rc = msm_finish_multi(cx, K, out_jac);
  if (rc == ZKHIP_OK) rc = msm_last_acc_path(cx, acc_path);
  if (rc != ZKHIP_OK) return ctx_fail(rc, cx);
  note_last_acc(ps, cx); t_prove_dev = dev;
  return ZKHIP_OK;
}

int zkhip_internal_field_selftest(int field, const uint32_t* limbs_in, size_t n, uint32_t* limbs_out) {
  BIND_CUR();
  if ((field != 0 && field != 1) || (n && (!limbs_in || !limbs_out)) || n > (1u << 20)) return fail(ZKHIP_ERR_ARG, "field 0 (Fq) or 1 (Fr), at most 2^20 cases");
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return msm_field_selftest(field, limbs_in, n, limbs_out, t_err, sizeof t_err);
}

int zkhip_internal_field_ops_selftest(int field, int op, const uint32_t* limbs_in, size_t n, uint32_t* limbs_out) {
  BIND_CUR();
  if ((field != 0 && field != 1) || (n && (!limbs_in || !limbs_out)) || n > (1u << 20)) return fail(ZKHIP_ERR_ARG, "field 0 (Fq) or 1 (Fr), at most 2^20 cases");
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return msm_field_ops_selftest(field, op, limbs_in, n, limbs_out, t_err, sizeof t_err);
}

int zkhip_internal_point_ops_selftest(int op, int mem, const uint32_t* limbs_in, size_t n, const uint32_t* table, size_t n_table, uint32_t* limbs_out) {
  BIND_CUR();
  if (n && (!limbs_in || !limbs_out)) return fail(ZKHIP_ERR_ARG, "n cases need their operands and a place for the results");
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return msm_point_ops_selftest(op, mem, limbs_in, n, table, n_table, limbs_out, t_err, sizeof t_err);
}

// Test hook of the bucket reduction's tail (msm.hip enqueue_tail)
int zkhip_internal_msm_tail(int edw, const uint64_t* items_affine, int W, unsigned N, int lo_bits, int total, uint64_t* out_jac) {
  BIND_CUR();
  if (!items_affine || !out_jac || W < 1 || W > MSM_MAX_JOBS || N < 2 || N > 2048 || (N & (N - 1)) || lo_bits < 0 || lo_bits > 11)
    return fail(ZKHIP_ERR_ARG, "W in 1 .. 5, N a power of two in 2 .. 2048, lo_bits in 0 .. 11");
  std::lock_guard<std::mutex> lk(g.dev[cur_dev()].mu);
  return msm_tail_selftest(edw, items_affine, W, N, lo_bits, total, out_jac, t_err, sizeof t_err);
}

}  // extern "C"
