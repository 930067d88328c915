// What the translation units of the C ABI (api_*.hip) share: the handle structs that cross files, the library's state and its
// error / device-binding helpers, the MSM-plan helpers.  Not visible outside the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <atomic>
#include <memory>
#include <mutex>
#include <vector>

#include "host_field.hpp"
#include "msm.h"
#include "qap.h"
#include "witness.h"

extern "C" void zkhip_internal_cuts_by_weight(const uint32_t* w, size_t n, size_t parts, size_t* cuts);      // multi_device.cpp: zkhip_key_partition's rule

using namespace zkhip;      // (this header serves the api_*.hip units only)

#pragma GCC visibility push(hidden)

struct zkhip_bases {
  AffPacked* d_pts;  // len points; after zkhip_bases_precompute: table_c > 0 and levels x len points (level w = 2^(table_c w) P)
  uint8_t* d_inf;    // 1 where the base (or its table level) is the point at infinity; same shape as d_pts
  size_t len;
  int table_c;       // 0: plain base set
  int table_naf;     // 1: the table holds EVERY bit position (378 levels): scalars are recoded in non-adjacent form (msm.h, merged == 2)
  size_t n_finite;   // bases that are not the point at infinity (counted at upload)
  int device;        // the GPU that holds them
  int plain_c = 0;   // plain base set: window of the MSMs over it (zkhip_bases_set_window; 0: by the number of terms)
  EdwPacked* d_edw = nullptr;   // zkhip_bases_precompute[_ex] of a G1 set, one level per window: the table in precomputed Edwards form
                                // (same shape as d_pts; msm.h msm_table_edw) - single MSMs over it accumulate on the Edwards curve
};

struct zkhip_r1cs {
  R1csDev* dev;
  int device;
};

struct TailTables { host::FixedBase8 d1, d2; };      // fixed-base tables of delta_1 and delta_2 for the prover's tail
struct zkhip_crs {
  size_t n_vars, n_primary, domain_size;
  zkhip_bases *A, *B2, *B1, *H, *L;
  uint64_t alpha_g1[24], beta_g1[24], beta_g2[24], delta_g1[24], delta_g2[24];
  int device;
  int batch_msms = 1;     // the five MSMs of a proof in one launch sequence (zkhip_key_opts; the key carries its own choice)
  int table_model = 0;    // 1: A, B1, H and L all have their Edwards tables (zkhip_key_opts.table_model): the G1 MSMs of a proof add in that model
  mutable std::once_flag tail_once;               // built by the key's first proof (~0.2 s of host time)
  mutable std::unique_ptr<TailTables> tail;
};

// a key pair on the host (api_key.hip makes, writes and reads them; phase2.hip makes the re-randomised one)
struct zkhip_keypair {
  size_t n_vars, n_primary, domain_size;
  std::vector<uint64_t> alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, A, B2, B1, H, L, ABC;
};

namespace zkhip {
namespace api {
// Everything one proof in flight needs on the device: a stream for the QAP map, the witness buffer, five MSM contexts
// (the prover keeps 2 (large) or 5 (small circuits) MSMs in flight).  The library owns one (the plain entry points,
// serialised by g.mu); every zkhip_prover owns another, so several host threads can keep several proofs in flight.
constexpr int ZK_MSM_SLOTS = 8;
constexpr int ZK_CTX_Z = ZK_MSM_SLOTS + 1, ZK_CTX_H = ZK_MSM_SLOTS + 2, ZK_CTX_TOTAL = ZK_MSM_SLOTS + 3;
struct ProveState {
  // MSM contexts: [0, ZK_MSM_SLOTS) the slots of zkhip_msm_submit / collect (the first five also serve a proof whose five MSMs run as
  // separate launch sequences), [ZK_MSM_SLOTS] the context of a proof's five MSMs in ONE launch sequence, [ZK_CTX_Z] / [ZK_CTX_H] the
  // two sequences of a proof ALONE (round 6): the four MSMs over the assignment, and the H MSM behind the QAP map
  MsmCtx ctx[ZK_CTX_TOTAL] = {};   // (all zeros: no plan yet - msm.h)
  MsmLane lane[ZK_CTX_TOTAL] = {}; // ctx[k]'s streams and events, from its first plan (or zkhip_prover_create_streams) to release(), whatever becomes of the plans
  hipStream_t st = nullptr;
  hipEvent_t ev_st = nullptr;      // blocking-sync event for waits on st (the waiting host thread sleeps)
  hipEvent_t ev_up = nullptr, ev_qap = nullptr;   // split proofs: the assignment is on the device / the QAP map has finished (stream-to-stream)
  bool split_last = false;         // the last proof ran as two launch sequences (A, B-G2, B-G1, L beside the QAP map; then H)
  bool edw_last = false;           // the G1 MSMs of the last proof accumulated on the Edwards curve (read from their launches: MsmCtx::win_edw)
  MsmCtx* last_acc_ctx2 = nullptr; // ... whose second accumulation launch ran on this plan
  uint64_t* dz = nullptr;
  size_t dz_cap = 0;
  double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool chained_last = false;       // the last proof put upload, QAP map and MSMs on ONE stream without host waits: ms[0..1] are enqueueing times
  float last_accumulate_ms = 0.f;
  MsmCtx* last_acc_ctx = nullptr;  // the plan last_accumulate_ms was read from (zkhip_last_accumulate_entries)
  float last_acc_interval[2] = {0.f, 0.f};   // begin / end of that launch on the device's time base
  int last_submit_slot = -1;       // zkhip_msm_submit: the slot of the previous submission (its accumulation gates the next one's)
  uint32_t quad_below = 0;         // 0: the engine's default; else the MSM contexts' quad_below (zkhip_prover_set_streaming)
  void release() {
    for (MsmCtx& c : ctx) if (c.pending) { uint64_t drop[36]; (void)msm_finish(&c, drop); }      // never free work space or a lane under a running launch
    for (MsmCtx& c : ctx) if (c.planned) msm_plan_free(&c);
    for (MsmLane& l : lane) msm_lane_free(&l);
    if (st) { (void)hipStreamDestroy(st); st = nullptr; }
    if (ev_st) { (void)hipEventDestroy(ev_st); ev_st = nullptr; }
    if (ev_up) { (void)hipEventDestroy(ev_up); ev_up = nullptr; }
    if (ev_qap) { (void)hipEventDestroy(ev_qap); ev_qap = nullptr; }
    last_acc_ctx = last_acc_ctx2 = nullptr;
    if (dz) { (void)hipFree(dz); dz = nullptr; dz_cap = 0; }
  }
};

// One of these per GPU the process has initialised (zkhip_init(device), once per device).  HIP's current device is a
// property of the calling HOST THREAD, so every entry point that touches the device binds its thread first: to the device of
// the handle it is given (bases, key, constraint system, prover), or - for the entry points without a handle - to the
// thread's current library device (zkhip_set_device; defaults to the first initialised device).
constexpr int ZK_MAX_DEVICES = 16;
struct DevState {
  bool inited = false;
  ProveState ps;            // work space of the plain (handle-less / library-serialised) entry points on this device
  std::mutex mu;            // serialises them
};
struct Lib {
  DevState dev[ZK_MAX_DEVICES];
  int default_device = -1;
  // process-wide DEFAULTS of the key options (deprecated setters zkhip_set_*; a key's own options travel in zkhip_key_opts and
  // are resolved once at upload): atomics, so that a setter racing an upload is at least a clean read of one value or the other
  std::atomic<int> forced_c{0};
  std::atomic<int> crs_tables{1};       // zkhip_crs_upload builds window tables (zkhip_set_crs_precompute)
  std::atomic<int> batch_msms{1};       // table-backed keys: the five MSMs of a proof in one launch sequence
  std::mutex mu;            // guards inited / default_device
};
extern Lib g;                         // api_core.hip

// (defined here, inline: a unit that saw only an extern declaration could not know that they need no dynamic initialisation and
//  would reach them through the TLS init wrapper - whose weak reference to an init function that does not exist does not
//  resolve to null for a hidden symbol of a shared library)
inline thread_local char t_err[512] = {0};   // zkhip_last_error(): the calling thread's last failure
inline thread_local int t_dev = -1;          // this thread's library device (-1: the default device); changed by zkhip_init / zkhip_set_device ONLY
inline thread_local int t_slot_dev[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // device of this thread's last zkhip_msm_submit per slot (zkhip_msm_collect has no handle)
inline thread_local int t_prove_dev = -1;    // device of this thread's last MSM or proof through a handle (zkhip_last_prove_timings / _accumulate_ms)

// api_core.hip
int fail(int code, const char* msg);
int ctx_fail(int code, const MsmCtx* cx);
int cur_dev();
int bind_dev(int d);
#define BIND_CUR()  do { int rc_ = bind_dev(cur_dev()); if (rc_ != ZKHIP_OK) return rc_; } while (0)
#define BIND(h)     do { int rc_ = bind_dev((h)->device); if (rc_ != ZKHIP_OK) return rc_; } while (0)
// frees device / host allocations of an entry point on every exit path
struct Scratch {
  std::vector<void*> dev;
  ~Scratch() { for (void* p : dev) if (p) (void)hipFree(p); }
  hipError_t alloc(void** out, size_t bytes) { hipError_t e = hipMalloc(out, bytes ? bytes : 1); if (e == hipSuccess) dev.push_back(*out); return e; }
};
#define API_HIP(x)                                                                           \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) {                                                                  \
      snprintf(t_err, sizeof t_err, "%s: %s", #x, hipGetErrorString(e_));                    \
      return ZKHIP_ERR_HIP;                                                                  \
    }                                                                                        \
  } while (0)

// api_msm.hip
int auto_table_window(size_t n);
bool ctx_reusable(const MsmCtx* cx, size_t n, int table_c, int K, int naf, size_t total, int plain_c = 0);
int ensure_ctx(MsmCtx* cx, MsmLane& lane, size_t n, int table_c, int K = 1, int naf = 0, size_t total = 0, int plain_c = 0, int one_stream = -1);
void note_last_acc(ProveState& ps, MsmCtx* cx);
int last_entries_of(ProveState& ps, uint64_t* out);
bool naf_tables_fit(size_t total_points);
bool naf_tables_wanted(size_t total_points);
int bases_precompute_mode(zkhip_bases* b, int c, int naf, bool edw = false);
}  // namespace api
}  // namespace zkhip

// ---- per-application constants (zkhip.h: zkhip_aggregator_app) ------------------------------------------------------------------
struct zkhip_aggregator_app {
  zkhip_aggregator* agg = nullptr;
  const zkhip_crs* crs = nullptr;          // the key the cached points belong to
  int device = 0;
  std::vector<uint64_t> vk;                // the nested key (identity of the application)
  std::vector<uint32_t> s_idx;             // the constant positions: auxiliary variables only, sorted
  std::vector<uint64_t> s_val;             // their values, 6 limbs each
  uint64_t vk_hash[6];                     // primary input 0
  uint64_t points[4 * 36];                 // sum over s_idx of z_i Base_i for the A, B-G2, B-G1 and L queries (Jacobian)
  void* host_state = nullptr;              // aggregator.cpp: the key with its lines
  uint64_t* d_z_app = nullptr;             // n_vars x 6 limbs on the device: the constants at their positions, zero elsewhere
  std::mutex mu;                           // the GPU witness program of this application, uploaded on first use
  WitnessTape tape;
  bool prog_ready = false;
  WitnessProgDev prog;
};

#pragma GCC visibility pop
