// Internal interface of the MSM engine (msm.hip).  The public C ABI is include/zkhip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkhip.h"

namespace zkhip {

struct AffPacked;
struct EdwPacked;

#define MSM_MAX_AFF_LEVELS 4
#define MSM_MAX_JOBS 5   // MSMs sharing one launch sequence (the five query vectors of a proof)
struct MsmJob {
  const AffPacked* bases;        // table-backed base set (level 0 at bases[0 .. n))
  const uint8_t* inf_flags;
  const uint64_t* scalars;       // device memory, n x 6 u64
  size_t n;
  int scalars_mode;              // 0 canonical, 1 Montgomery (ABI), 2 packed device form
  size_t table_stride;           // distance between table levels, in points
  size_t n_finite;               // upper bound on the bases of this job that are not the point at infinity (0: unknown, use n):
                                 // sizes the slices of the accumulation to the entries that can actually occur
  const EdwPacked* edw = nullptr;  // the same table in precomputed Edwards form (msm_table_edw), or null: a single MSM over a one-level-
                                   // per-window table then accumulates on G1's 2-isogenous Edwards curve (ec_edw.cuh), and so do up to
                                   // four MSMs of a merged plan when every job that has terms brings one (msm_launch_multi)
};
// the terms of a job that can produce an entry: a base at infinity never does (plans are sized by this, launches counted by it)
static inline size_t msm_job_terms(const MsmJob& j) { return (j.n_finite && j.n_finite < j.n) ? j.n_finite : j.n; }

// A context's place on the runtime's hardware queues: its streams and the events that order and time its launch sequences.  The context's
// OWNER holds the lane for as long as the slot exists (all mains of its contexts are made first, then all sides: api_msm.hip); plans own memory only.
struct MsmLane {     // all zeros: nothing made yet
  hipStream_t main, side;   // side may stay null: the whole launch sequence then runs on main (stage_reduce)
  hipEvent_t ev, ev2, ev_acc0, ev_acc1, ev_done;
};
hipError_t msm_lane_create_main(MsmLane* lane);      // (the three create what is missing and leave the rest alone)
hipError_t msm_lane_create_side(MsmLane* lane);
hipError_t msm_lane_create_events(MsmLane* lane);
void msm_lane_free(MsmLane* lane);      // destroys what was made: all zeros again (nothing of it may be in flight)

#define ZK_PRIO_BOARD_WORDS (8 * 8 * 2 * 16 * 4 * 16)
struct MsmCtx {      // all zeros: no plan
  bool planned;        // msm_plan_init succeeded and msm_plan_free has not run since: every field below is valid
  int c, W, L, logL;   // W: bucket windows (each owns 2^(c-1) buckets)
  int Wd;              // digits per scalar: W without a table; with a precomputed table all Wd digit positions share ONE bucket window
  int merged;          // 1: bases are a table  table[w * stride + i] = 2^(off_w) P_i  (msm_table_build), one digit per window;
                       // 2: a table with EVERY bit position, table[j * stride + i] = 2^j P_i: scalars are recoded in width-(c+1)
                       //    non-adjacent form (odd signed digits at arbitrary positions, 378 / (c + 2) of them on average)
  int K;               // merged plans: MSMs per launch sequence, one bucket window each (W == K); plain plans: 1
  uint16_t win_off[96];
  uint8_t win_bits[96];
  size_t B, max_n;
  size_t total_terms;   // bound on the terms of one launch sequence (all jobs): sizes the entry list, the slices and the slot array
  int one_stream;       // 1: the whole launch sequence on the lane's main stream (a prover that shares the chip); 0: row / column trees side by side
  uint32_t quad_below;  // reduction launches with fewer outputs than this spread an addition over four lanes (latency) instead of one (total work)
  uint32_t S, T, slot_stride;   // slice length, slice count, words per row of the slot array
  MsmLane* lane;        // not owned: this context's streams and events (without a side stream stage_reduce keeps to main whatever one_stream says later)
  hipEvent_t acc_gate;  // optional (not owned): the accumulation of this launch sequence starts after this event - the end of the
                        // accumulation of the MSM submitted before it on another context (zkhip_msm_submit): the sort of MSM i+1 and
                        // the reduction of MSM i-1 run under the accumulation of MSM i, two accumulations never share the chip
  // bucket sort (k_digit_pass / k_bucket_sort): hist[part][block] (+ 1: the total), (entry, low bucket bits) pairs grouped by part
  uint32_t sort_LB, sort_NP, sort_bins, sort_tile;
  uint32_t* hist;
  uint2* pairs;
  size_t hist_len;
  uint32_t *counts, *offsets, *block_tot, *entries;
  uint32_t* goff;       // slice weights in front of every bucket (nb + 1 values): see k_accumulate
  uint32_t *order, *ord_hist;   // single Edwards launches (k_bucket_order): the bucket indices by count, descending (nb values), and the
                                // counting sort's histogram [ZK_LOCK_KEYS][blocks]; null in plans of K > 1 (their Edwards launches are sliced only)
  uint32_t lock_min_live;       // non-empty buckets a launch needs for the lockstep route: two waves for every SIMD of the chip
  uint2* fix_list;      // (first, last) F slot of the buckets cut into more than four F pieces (k_accumulate -> k_fixup_fold)
  uint2* fix_short;     // (first F slot, number of F pieces) of the buckets with two to four (k_accumulate -> k_fixup_fold)
  uint32_t *buckets, *segS[2], *colS[2], *hilo, *planes[2];
  uint64_t *win_abi, *win_host;
  // batched-affine levels in front of the XYZZ accumulation (k_affine_level): per level the bucket counts / offsets of its output,
  // two point buffers used alternately, the prefix-product scratch of one launch
  int aff_levels;                    // 0: every entry goes straight to k_accumulate
  int aff_forced;                    // the msm_forced_aff_levels() this plan was made under
  uint32_t aff_m, aff_lanes;         // outputs per lane; lanes per launch (the scratch holds aff_m * 27 * aff_lanes words)
  uint32_t *lcnt[MSM_MAX_AFF_LEVELS], *loff[MSM_MAX_AFF_LEVELS];
  AffPacked* pbuf[2];
  uint32_t* aff_scratch;
  size_t m_acc_max;                  // upper bound on the entries that reach k_accumulate (sizes S, T and the slot array)
  float last_accumulate_ms;
  size_t last_hist_m;                // words of hist the last launch scanned: the last one holds the number of entries it sorted (msm_last_entries)
  uint32_t acc_gen;                           // generation of the device's time base when this launch's ev_acc0 was recorded (msm_time_base_reset bumps it)
  float last_acc_begin_ms, last_acc_end_ms;   // the same launch on the device's time base (msm_time_base): lets a caller that keeps
                                              // several MSMs in flight see how their accumulations overlap
  // measurement aid (ZKHIP_DEBUG_DUMP=<dir>, tools/acc_probe.py): per-wave begin / end clocks of k_accumulate and, at collection, a dump
  // of the bucket populations; null / unused otherwise
  uint64_t* dbg_times;
  uint32_t* prio_board;      // k_accumulate: iteration counts of the waves of a launch, one word per hardware wave slot (zeroed once)
  uint32_t prio_seq;
  uint32_t last_S, last_T;           // slice length / slices of the last launch (before the kernel's own shortening, see slice_len)
  int last_tight;
  bool pending;       // an MSM has been enqueued by msm_launch and not yet collected by msm_finish
  size_t pending_n;
  bool win_edw;       // the pending launch leaves Edwards points (X : Y : Z : T) in win_host: msm_finish applies psi (msm.hip edw_abi_to_jac)
  char errbuf[256];
};

// tuning / test knob: number of batched-affine levels of the plans made from now on (-1: automatic)
void msm_force_aff_levels(int levels);
int msm_forced_aff_levels();
// A/B and test knob of the lockstep route of the Edwards accumulation: mode 0 off, 1 on, -1 the environment (ZKHIP_LOCKSTEP);
// min_buckets: the non-empty buckets a launch needs to take it (-1: the chip's own figure)
void msm_force_lockstep(int mode, int min_buckets);
// the route the plan's last launch took, read back from the device: 1 lockstep, 0 sliced (always, for a merged Edwards launch of
// several jobs), -1 not an Edwards launch
int msm_last_acc_path(MsmCtx* ctx, int* out);
// total_terms: upper bound on the terms (finite bases) of all K jobs of one launch together; 0 = K * max_n
// lane: the caller's, with its main stream and its events made; the plan refers to it and never creates or destroys a part of it
// one_stream: 1 / 0 the plan's one_stream from the start, -1 the environment (ZKHIP_MSM_ONE_STREAM, default 0): msm_one_stream resolves it
int msm_one_stream(int one_stream);
int msm_plan_init(MsmCtx* ctx, MsmLane* lane, size_t max_n, int c, int merged, int K, size_t total_terms = 0, int one_stream = -1);
// a per-device event recorded once: the origin of last_acc_begin_ms / last_acc_end_ms
hipEvent_t msm_time_base();
// record the origin again (now): intervals read afterwards are relative to this moment
int msm_time_base_reset();
void msm_plan_free(MsmCtx* ctx);      // the plan's memory; the lane stays with its owner
int msm_bases_convert(const uint64_t* d_bases_abi, size_t n, AffPacked* d_out, uint8_t* d_inf_flags, char* errbuf, size_t errlen);
// table_stride: distance (in points) between the levels of a precomputed table (merged plans only)
// edw: the table in precomputed Edwards form (or null)
int msm_launch(MsmCtx* ctx, const AffPacked* d_bases, const uint8_t* d_inf_flags, const uint64_t* d_scalars, size_t n,
               int scalars_montgomery, size_t table_stride, const EdwPacked* edw = nullptr);
int msm_finish(MsmCtx* ctx, uint64_t out_jac[36]);
// The entries (non-zero digits = mixed additions of k_accumulate, no affine levels in front) of the last launch of this plan, read
// back from the sort's histogram: a measurement aid, synchronises the device.  0: nothing launched yet.
int msm_last_entries(MsmCtx* ctx, uint64_t* out);
// merged plans: up to ctx->K independent MSMs (same window, each at most max_n terms) through ONE launch sequence:
// one sort, one accumulation launch, one reduction chain with a bucket window per job.  out_jac: K x 36.
int msm_launch_multi(MsmCtx* ctx, int K, const MsmJob* jobs);
int msm_finish_multi(MsmCtx* ctx, int K, uint64_t* out_jac);
// levels of a window table for window size c
static inline int msm_table_levels(int c, int naf = 0) { return naf ? 378 : (378 + c - 1) / c; }
// d_table: levels x n points, level 0 (= the n base points) already in place; d_tinf: levels x n flags, level 0 in place.
// Fills levels 1 .. levels-1:  table[w * n + i] = 2^(c w) P_i  in affine packed form.
int msm_table_build(AffPacked* d_table, uint8_t* d_tinf, size_t n, int c, int naf, char* errbuf, size_t errlen);
// The Edwards form of a one-level-per-window table over the n bases d_bases (level 0; flags d_inf): *d_out[w n + i] = chi([1/2 mod r]
// 2^(off_w) P_i) in precomputed form (ec_edw.cuh), so that MSMs over it use XYZZ's digits.  ZKHIP_ERR_ARG when a base is not a point
// of order r on G1's curve (a G2 set, a point outside the subgroup): the caller keeps the XYZZ path.
int msm_table_edw(const AffPacked* d_bases, const uint8_t* d_inf, size_t n, int c, EdwPacked** d_out, char* errbuf, size_t errlen);
// point i of an Edwards table (EdwPacked: 288 bytes; ec_edw.cuh), null stays null
static inline const EdwPacked* msm_edw_at(const EdwPacked* t, size_t i) {
  return t ? reinterpret_cast<const EdwPacked*>(reinterpret_cast<const char*>(t) + i * 288) : nullptr;
}

// Fq multiplications per second of the whole device, measured now: dependent fp_mul chains at two waves per SIMD (~25 ms)
int msm_field_selftest(int field, const uint32_t* in_host, size_t n, uint32_t* out_host, char* errbuf, size_t errlen);
// test hook: one function of the field layer (fp29.cuh, fp_inv.cuh) per launch on n cases of three raw-limb operands; out: n x (NL words
// and a flag word).  ZKHIP_ERR_ARG for an op the field does not have (msm.hip FieldOp)
int msm_field_ops_selftest(int field, int op, const uint32_t* in_host, size_t n, uint32_t* out_host, char* errbuf, size_t errlen);
// test hook (point_ops_selftest.hip): one point operation of ec.cuh / ec_mem.cuh / ec_edw.cuh per launch on n cases of raw-limb
// operands (224 words in, 217 words out per case; mem 0: limb-major references, 1: slot references).  ZKHIP_ERR_ARG for an unknown op,
// for mem 1 with an op that takes no memory reference, and for a lockstep run whose entries leave its table; nothing is launched then
int msm_point_ops_selftest(int op, int mem, const uint32_t* in_host, size_t n, const uint32_t* table_host, size_t n_table, uint32_t* out_host,
                           char* errbuf, size_t errlen);
int msm_measure_fqmul_rate(double* fq_mul_per_s, char* errbuf, size_t errlen);
// test hook: the tail of the bucket reduction (bit planes, R * hi + lo) on 2W groups of N affine ABI points given on the host;
// an Edwards run (edw != 0) returns twice the sums.  out_jac: W points (+ W plain totals of the lo groups if total), 36 limbs each
int msm_tail_selftest(int edw, const uint64_t* items_aff, int W, uint32_t N, int lo_bits, int total, uint64_t* out_jac, char* errbuf, size_t errlen);

int fixed_base_mul(const uint64_t base_aff[24], const uint64_t* d_scalars, size_t n, int montgomery, uint64_t* d_out,
                   char* errbuf, size_t errlen);

}  // namespace zkhip
