// C ABI (include/zkhip.h): per-application constants of the aggregator circuit, witness generation on the GPU.
#include <string.h>
#include <string>

#include "api_internal.hpp"
#include "wait.h"

using namespace zkhip::api;

#pragma GCC visibility push(hidden)      // this file's own helpers and handle structs

// ---- witness generation on the GPU (witness.hip) ---------------------------------------------------------------------------
struct zkhip_gpu_witness {
  int device;
  zkhip_aggregator* agg;
  WitnessProg prog;
  const WitnessTape* tape = nullptr;     // the circuit's recorded program (lives as long as agg): level boundaries for the wide kernels
  int waves = 0;                         // zkhip_gpu_witness_set_waves: 0 = auto
  size_t in_words;
  size_t max_batches = 1;
  uint64_t* d_in = nullptr;
  uint32_t* d_vals = nullptr;
  uint32_t* d_flag = nullptr;
  uint64_t* h_in = nullptr;       // pinned staging: inputs, then the flag and the primary inputs on the way back
  hipStream_t st = nullptr, st2 = nullptr;
  hipEvent_t ev = nullptr, ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;       // around the kernels of the last run (zkhip_gpu_witness_last_ms)
  bool timed = false;
};

// n batches in ONE launch sequence (one workgroup each).  vk / proofs / inputs: n pointers; d_z_out: n x n_vars x 6 limbs in device
// memory, contiguous; primary_inputs: n x n_primary x 6 limbs (host, may be null); degenerate[i] = 1 where an inversion met zero
// (that batch's assignment is unusable: use the host generator).
static int gpu_witness_run_impl(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_vk, const uint64_t* const* nested_proofs,
                                const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate,
                                uint32_t wpg, uint32_t seg /* witness_launch's knobs: the product passes witness_env_wpg() / _segment() */,
                                int waves /* -1: the handle's (zkhip_gpu_witness_set_waves) */) {
  if (!w || (!app && !nested_vk) || !nested_proofs || !nested_inputs || !d_z_out || !degenerate) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (n < 1 || n > w->max_batches) return fail(ZKHIP_ERR_ARG, "more batches than the work space holds");
  BIND(w);
  const zkhip_aggregator* a = w->agg;
  const size_t vk_w = 60 + 12 * (a->inputs_per_proof + 1), pr_w = 48 * a->num_proofs, in_w = 6 * a->inputs_per_proof * a->num_proofs;
  if (vk_w + pr_w + in_w != w->in_words) return fail(ZKHIP_ERR_STATE, "witness program does not match the circuit");
  WitnessProg prog = w->prog;
  const WitnessTape* tape = w->tape;
  if (waves < 0) waves = w->waves;
  if (app) {
    // the application's own program (its key folded in: no key-hash chain, a tenth fewer multiplications, zeros at the constant
    // positions of the assignment), uploaded on first use
    if (app->agg != a || app->device != w->device) return fail(ZKHIP_ERR_ARG, "application handle of another circuit or device");
    std::lock_guard<std::mutex> lk(app->mu);
    if (!app->prog_ready) {
      int rc = witness_prog_upload(app->tape, &app->prog, t_err, sizeof t_err);
      if (rc != ZKHIP_OK) return rc;
      app->prog_ready = true;
    }
    if (app->prog.prog.n_pos > w->prog.n_pos || app->prog.prog.n_inputs != w->prog.n_inputs)
      return fail(ZKHIP_ERR_STATE, "the application's program does not fit the generator's work space");
    prog = app->prog.prog;
    tape = &app->tape;                      // (auto decides on the program that runs)
  }
  for (size_t i = 0; i < n; i++) {
    uint64_t* h = w->h_in + i * w->in_words;
    memcpy(h, app ? app->vk.data() : nested_vk[i], vk_w * 8); memcpy(h + vk_w, nested_proofs[i], pr_w * 8); memcpy(h + vk_w + pr_w, nested_inputs[i], in_w * 8);
  }
  uint64_t* h_flags = w->h_in + w->max_batches * w->in_words;            // [n flags as u32 | primary inputs]
  uint64_t* h_prim = h_flags + w->max_batches;
  API_HIP(hipMemcpyAsync(w->d_in, w->h_in, n * w->in_words * 8, hipMemcpyHostToDevice, w->st));
  API_HIP(hipMemsetAsync(w->d_flag, 0, n * 4, w->st));
  API_HIP(hipEventRecord(w->ev_t0, w->st));
  witness_launch(prog, tape->level_start.data(), w->d_in, w->d_vals, (uint64_t*)d_z_out, w->d_flag, (uint32_t)n, wpg, seg, (uint32_t)waves, w->st, w->st2, w->ev_fork,
                 w->ev_join);
  API_HIP(hipEventRecord(w->ev_t1, w->st));
  w->timed = true;
  API_HIP(hipGetLastError());
  API_HIP(hipMemcpyAsync(h_flags, w->d_flag, n * 4, hipMemcpyDeviceToHost, w->st));
  for (size_t i = 0; i < n; i++)
    API_HIP(hipMemcpyAsync(h_prim + i * a->n_primary * 6, (const uint64_t*)d_z_out + (i * a->n_vars + 1) * 6, a->n_primary * 48, hipMemcpyDeviceToHost, w->st));
  API_HIP(hipEventRecord(w->ev, w->st));
  API_HIP(zk_event_wait(w->ev));
  for (size_t i = 0; i < n; i++) degenerate[i] = ((const uint32_t*)h_flags)[i] != 0;
  if (primary_inputs) memcpy(primary_inputs, h_prim, n * a->n_primary * 48);
  return ZKHIP_OK;
}

// ---- test hooks of the witness interpreter ----------------------------------------------------------------------------------
// The structural rules of tools/sanitize/tape_check.cpp: a program that passes cannot address outside its buffers on the device -
// every operand is a constant in range or an earlier position of the same part, every input and bit index is in range, the
// levelled part is whole chunks (k_witness fetches 64 positions at a time), every code is one w_exec knows.
static const char* witness_program_check(const zkhip_witness_program* p) {
  if (!p) return "null program";
  const size_t n = p->n_pos, cs = p->chain_start;
  if (n > (1u << 26) || p->n_consts > (1u << 26) || p->n_inputs > (1u << 26) || p->n_vars > (1u << 26) || p->n_levels > (1u << 26)) return "program too large";
  if ((n && (!p->code || !p->a || !p->b)) || !p->level_start || (p->n_vars && !p->out_ref) || (p->n_consts && !p->consts)) return "null array";
  if (n < 1 || p->n_vars < 1) return "empty program";
  if (cs > n || cs % 64) return "chain_start is not a chunk boundary inside the program";
  if (p->level_start[0] != 0 || p->level_start[p->n_levels] != cs) return "the levels do not cover [0, chain_start)";
  std::vector<uint32_t> level_begin(cs, 0);
  for (size_t l = 0; l < p->n_levels; l++) {
    const uint32_t b = p->level_start[l], e = p->level_start[l + 1];
    if (b % 64 || e % 64 || b > e || e > cs) return "a level is not a whole number of 64-position chunks";
    for (uint32_t q = b; q < e; q++) level_begin[q] = b;
  }
  std::vector<uint8_t> defined(n, 0);
  for (size_t q = 0; q < n; q++) {
    const uint8_t c = p->code[q];
    if (c == WT_NOP) continue;
    const bool chain = q >= cs;
    auto ref_ok = [&](int32_t r) -> bool {
      if (r < 0) return (size_t)(-1 - (int64_t)r) < p->n_consts;
      if ((size_t)r >= q || !defined[r]) return false;
      return chain ? (size_t)r >= cs : (size_t)r < level_begin[q];
    };
    if (c == WT_INPUT) {
      if (p->a[q] < 0 || (size_t)p->a[q] >= p->n_inputs) return "input index out of range";
    } else if (c == WT_ADD || c == WT_MUL || c >= WT_SUBK) {
      if (c >= WT_SUBK && (c - WT_SUBK < 1 || c - WT_SUBK > 11)) return "a - b + 2^k r with k outside 1 .. 11";
      if (!ref_ok(p->a[q]) || !ref_ok(p->b[q])) return "operand not defined before its reader (an earlier level / earlier in the chain)";
    } else if (c == WT_RED || c == WT_INV || c == WT_INV0 || c == WT_BIT) {
      if (!ref_ok(p->a[q])) return "operand not defined before its reader (an earlier level / earlier in the chain)";
      if (c == WT_BIT && (p->b[q] < 0 || p->b[q] >= 384)) return "bit index outside 0 .. 383";
    } else {
      return c == WT_SUB ? "plain WT_SUB in a laid-out program" : "unknown instruction code";
    }
    defined[q] = 1;
  }
  for (size_t i = 0; i < p->n_vars; i++) {
    const int32_t r = p->out_ref[i];
    if (r < 0 ? (size_t)(-1 - (int64_t)r) >= p->n_consts : ((size_t)r >= n || !defined[r])) return "assignment entry reads an undefined position or constant";
  }
  return nullptr;
}

#pragma GCC visibility pop

extern "C" {

// ---- per-application constants: the public entry points ---------------------------------------------------------------------
// (RegisterApplication fixes a nested verification key, aggregator_server.cpp:170-235; everything the wrapping circuit derives from
// the key alone - its variables, its MiMC hash chain, the lines of -beta and -delta, the doubling chains of ABC_i - is the same in
// every batch of that application: a quarter of the assignment.)
int zkhip_aggregator_app_new(zkhip_aggregator* a, const zkhip_crs* crs, const uint64_t* nested_vk, zkhip_aggregator_app** out) {
  if (!a || !crs || !nested_vk || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND(crs);
  const size_t m = a->n_vars, l = a->n_primary;
  if (crs->n_vars != m || crs->n_primary != l || crs->A->len != m || crs->L->len != m - l - 1)
    return fail(ZKHIP_ERR_ARG, "zkhip_aggregator_app_new: the proving key is not the whole key of this circuit");
  std::unique_ptr<zkhip_aggregator_app> app(new zkhip_aggregator_app());
  app->agg = a; app->crs = crs; app->device = crs->device;
  const size_t vk_w = 60 + 12 * (a->inputs_per_proof + 1);
  app->vk.assign(nested_vk, nested_vk + vk_w);
  {
    // the key's own points must lie on their curves (the proofs of a batch are checked per batch): checked with the key's points
    // standing in for a proof
    std::vector<uint64_t> stand_in(48 * a->num_proofs);
    for (size_t q = 0; q < a->num_proofs; q++) {
      memcpy(&stand_in[q * 48], nested_vk, 96); memcpy(&stand_in[q * 48 + 12], nested_vk + 12, 192); memcpy(&stand_in[q * 48 + 36], nested_vk, 96);
    }
    int ok = 0;
    if (zkhip_aggregator_check_inputs(a, nested_vk, stand_in.data(), &ok) != ZKHIP_OK || !ok)
      return fail(ZKHIP_ERR_ARG, "zkhip_aggregator_app_new: the nested verification key has a point that is not on its curve");
  }
  // the program of this application: the circuit recorded with the key as CONSTANTS (witness_tape.cpp) - what folds is constant
  std::string terr;
  if (witness_tape_build(a->num_proofs, a->inputs_per_proof, &app->tape, &terr, nested_vk) != 0) {
    snprintf(t_err, sizeof t_err, "application program: %s", terr.c_str());
    return ZKHIP_ERR_ARG;                            // (a key with a point off its curve / a degenerate key meets an inversion of zero here)
  }
  WitnessTape& T = app->tape;
  if (T.n_vars != m) return fail(ZKHIP_ERR_STATE, "application program does not match the circuit");
  if (T.out_ref[1] >= 0) return fail(ZKHIP_ERR_STATE, "application program: the key hash did not fold into a constant");
  memcpy(app->vk_hash, &T.consts[(size_t)(-1 - T.out_ref[1]) * 6], 48);
  // the zero constant every masked position is pointed at
  int32_t zero_ref = 0;
  {
    size_t zi = T.consts.size() / 6;
    for (size_t i = 0; i < T.consts.size() / 6; i++) {
      const uint64_t* c = &T.consts[i * 6];
      if (!(c[0] | c[1] | c[2] | c[3] | c[4] | c[5])) { zi = i; break; }
    }
    if (zi == T.consts.size() / 6) T.consts.insert(T.consts.end(), 6, 0);
    zero_ref = -1 - (int32_t)zi;
  }
  std::vector<uint64_t> z_app(m * 6, 0);
  for (size_t i = l + 1; i < m; i++) {
    if (T.out_ref[i] >= 0) continue;
    const uint64_t* c = &T.consts[(size_t)(-1 - T.out_ref[i]) * 6];
    app->s_idx.push_back((uint32_t)i);
    app->s_val.insert(app->s_val.end(), c, c + 6);
    memcpy(&z_app[i * 6], c, 48);
    T.out_ref[i] = zero_ref;                         // the application's generator writes the MASKED assignment
  }
  // The masked HOST generator (witness_proofs_only) leaves the whole hash and key sections [sec_hash, sec_proofs) at zero and relies on
  // every one of those positions being a constant of the handle: checked here rather than assumed - a recorder that stopped
  // folding one of them would otherwise give an assignment with a hole, a wrong H and an unverifiable proof with rc OK.
  {
    size_t covered = 0;
    for (uint32_t i : app->s_idx) covered += (i >= a->sec_hash && i < a->sec_proofs) ? 1 : 0;
    if (covered != a->sec_proofs - a->sec_hash)
      return fail(ZKHIP_ERR_STATE, "zkhip_aggregator_app_new: the key's hash and line sections did not fold into constants completely");
  }
  // Self-check: the constants came out of the RECORDING build of the circuit (the route the device takes); the host generator is the
  // reference for parity.  One full host assignment under this key (the key's own points stand in for the proofs: the constant
  // positions do not depend on them) must hold exactly these values there - a degenerate key, where the two routes part, gets no handle.
  {
    std::vector<uint64_t> stand_in(48 * a->num_proofs), zero_inputs(6 * a->inputs_per_proof * a->num_proofs, 0), z_full(m * 6);
    for (size_t q = 0; q < a->num_proofs; q++) {
      memcpy(&stand_in[q * 48], nested_vk, 96); memcpy(&stand_in[q * 48 + 12], nested_vk + 12, 192); memcpy(&stand_in[q * 48 + 36], nested_vk, 96);
    }
    if (zkhip_aggregator_witness(a, nested_vk, stand_in.data(), zero_inputs.data(), z_full.data()) != ZKHIP_OK)
      return fail(ZKHIP_ERR_ARG, "zkhip_aggregator_app_new: the host generator refuses this nested key");
    for (size_t j = 0; j < app->s_idx.size(); j++)
      if (memcmp(&z_full[(size_t)app->s_idx[j] * 6], &app->s_val[j * 6], 48) != 0)
        return fail(ZKHIP_ERR_ARG, "zkhip_aggregator_app_new: degenerate nested key (the recorded constants differ from the host generator's)");
    if (memcmp(&z_full[6], app->vk_hash, 48) != 0) return fail(ZKHIP_ERR_STATE, "zkhip_aggregator_app_new: key hash mismatch");
  }
  int rc = zk_app_host_new(a, nested_vk, &app->host_state);
  if (rc != ZKHIP_OK) return fail(rc, "zkhip_aggregator_app_new: the nested key's lines could not be computed (a degenerate key)");
  hipError_t e = hipMalloc(&app->d_z_app, m * 48);
  if (e == hipSuccess) e = hipMemcpy(app->d_z_app, z_app.data(), m * 48, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipStreamSynchronize(0);
  if (e != hipSuccess) {
    snprintf(t_err, sizeof t_err, "zkhip_aggregator_app_new: %s", hipGetErrorString(e));
    zkhip_aggregator_app_free(app.release());
    return ZKHIP_ERR_HIP;
  }
  // ONE masked MSM per query: sum over the constant positions of z_i Base_i (the positions hold zero in z_app elsewhere)
  struct { const zkhip_bases* b; size_t off, len; } q[4] = {{crs->A, 0, m}, {crs->B2, 0, m}, {crs->B1, 0, m}, {crs->L, l + 1, m - l - 1}};
  for (int k = 0; k < 4 && rc == ZKHIP_OK; k++)
    rc = zkhip_msm_dev(q[k].b, 0, app->d_z_app + q[k].off * 6, q[k].len, 1, app->points + 36 * k);
  if (rc != ZKHIP_OK) { zkhip_aggregator_app_free(app.release()); return rc; }
  *out = app.release();
  return ZKHIP_OK;
}

void zkhip_aggregator_app_free(zkhip_aggregator_app* app) {
  if (!app) return;
  (void)bind_dev(app->device);
  if (app->prog_ready) witness_prog_free(&app->prog);
  if (app->d_z_app) (void)hipFree(app->d_z_app);
  zk_app_host_free(app->host_state);
  delete app;
}

size_t zkhip_aggregator_app_num_constants(const zkhip_aggregator_app* app) { return app ? app->s_idx.size() : 0; }

int zkhip_aggregator_app_constants(const zkhip_aggregator_app* app, uint32_t* positions, uint64_t* values, uint64_t vk_hash[6], uint64_t points_jac[144]) {
  if (!app) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (positions) memcpy(positions, app->s_idx.data(), app->s_idx.size() * 4);
  if (values) memcpy(values, app->s_val.data(), app->s_val.size() * 8);
  if (vk_hash) memcpy(vk_hash, app->vk_hash, 48);
  if (points_jac) memcpy(points_jac, app->points, sizeof app->points);
  return ZKHIP_OK;
}

int zkhip_aggregator_app_mask(const zkhip_aggregator_app* app, uint64_t* z) {
  if (!app || !z) return fail(ZKHIP_ERR_ARG, "null pointer");
  for (size_t j = 0; j < app->s_idx.size(); j++) {
    uint64_t* w = z + (size_t)app->s_idx[j] * 6;
    if (memcmp(w, &app->s_val[j * 6], 48) != 0) return fail(ZKHIP_ERR_ARG, "this assignment was not generated under the application's nested key");
    memset(w, 0, 48);
  }
  return ZKHIP_OK;
}

int zkhip_aggregator_witness_app(const zkhip_aggregator_app* app, const uint64_t* nested_proofs, const uint64_t* nested_inputs, uint64_t* z_out) {
  if (!app || !nested_proofs || !nested_inputs || !z_out) return fail(ZKHIP_ERR_ARG, "null pointer");
  return zk_app_host_witness(app->agg, app->host_state, app->vk.data(), nested_proofs, nested_inputs, app->s_idx.data(), app->s_idx.size(), app->vk_hash, z_out);
}

int zkhip_gpu_witness_new(zkhip_aggregator* a, zkhip_gpu_witness** out) { return zkhip_gpu_witness_new_batched(a, 1, out); }

int zkhip_gpu_witness_new_batched(zkhip_aggregator* a, size_t max_batches, zkhip_gpu_witness** out) {
  BIND_CUR();
  if (!a || !out || max_batches < 1 || max_batches > 256) return fail(ZKHIP_ERR_ARG, "bad argument");
  zkhip_gpu_witness* w = new zkhip_gpu_witness();
  w->device = cur_dev(); w->agg = a; w->max_batches = max_batches;
  const WitnessTape* tape = nullptr;
  int rc = witness_prog(a, &w->prog, &tape, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) { delete w; return rc; }
  w->tape = tape;
  w->in_words = (size_t)w->prog.n_inputs * 6;
  {
    // n_pos x 64 bytes of values per witness (352 MB at 32 proofs with one input each): say so when they do not fit
    const size_t need = max_batches * (size_t)w->prog.n_pos * witness_value_bytes;
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess && need > mem_free) {
      snprintf(t_err, sizeof t_err, "zkhip_gpu_witness_new: the work space of %zu witnesses takes %zu bytes, %zu are free on the device", max_batches, need, mem_free);
      delete w;
      return ZKHIP_ERR_HIP;
    }
  }
  hipError_t e = hipMalloc(&w->d_in, max_batches * w->in_words * 8);
  if (e == hipSuccess) e = hipMalloc(&w->d_vals, max_batches * (size_t)w->prog.n_pos * witness_value_bytes);
  if (e == hipSuccess) e = hipMalloc(&w->d_flag, max_batches * 4 + 64);
  if (e == hipSuccess) e = hipHostMalloc(&w->h_in, max_batches * (w->in_words + 1 + a->n_primary * 6) * 8);
  // (High-priority streams for the witness launches - hardware queues of their own instead of a place behind some prover's 2 ms
  //  accumulation launch - were measured in round 6 and LOSE 10 %: 256-265 -> 221-234 proofs/s with nine inputs, 444-449 -> 395-407 with
  //  one, profiles/r06_witness_wpg_and_priority.txt.  A witness wave that is dispatched at once takes its CU slot at once, on whatever
  //  CU frees one first; what the provers need is that those slots are FEW, which is what k_witness's four waves a workgroup do.)
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&w->st, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&w->st2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&w->ev, hipEventBlockingSync | hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&w->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&w->ev_join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreate(&w->ev_t0);
  if (e == hipSuccess) e = hipEventCreate(&w->ev_t1);
  if (e != hipSuccess) {
    snprintf(t_err, sizeof t_err, "zkhip_gpu_witness_new: %s (work space of %zu witnesses: %zu bytes of values)", hipGetErrorString(e), max_batches,
             max_batches * (size_t)w->prog.n_pos * witness_value_bytes);
    zkhip_gpu_witness_free(w);
    return ZKHIP_ERR_HIP;
  }
  *out = w;
  return ZKHIP_OK;
}

int zkhip_gpu_witness_set_waves(zkhip_gpu_witness* w, int waves) {
  if (!w || !witness_waves_ok(waves)) return fail(ZKHIP_ERR_ARG, "waves per witness: 0 (auto), 1, 2, 4, 8 or 16");
  w->waves = waves;
  return ZKHIP_OK;
}

int zkhip_gpu_witness_last_ms(zkhip_gpu_witness* w, double* ms) {
  if (!w || !ms) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (!w->timed) return fail(ZKHIP_ERR_STATE, "no run yet");
  BIND(w);
  float t = 0.f;
  API_HIP(hipEventElapsedTime(&t, w->ev_t0, w->ev_t1));
  *ms = (double)t;
  return ZKHIP_OK;
}

// Host only: no device is touched
int zkhip_gpu_witness_plan(zkhip_aggregator* a, int waves, size_t out[4]) {
  if (!a || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  if (!witness_waves_ok(waves)) return fail(ZKHIP_ERR_ARG, "waves per witness: 0 (auto), 1, 2, 4, 8 or 16");
  const WitnessTape* T = nullptr;
  int rc = witness_tape_of(a, &T, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  const WitnessPlan pl = witness_plan(T->level_start.data(), T->level_start.size() - 1, T->code.size(), (uint32_t)waves);
  out[0] = pl.chunks; out[1] = pl.levels; out[2] = pl.steps; out[3] = pl.value_bytes;
  if (waves == 0) out[2] = pl.waves;      // (see zkhip.h: for auto the width, not its steps)
  return ZKHIP_OK;
}

void zkhip_gpu_witness_free(zkhip_gpu_witness* w) {
  if (!w) return;
  (void)bind_dev(w->device);
  if (w->d_in) (void)hipFree(w->d_in);
  if (w->d_vals) (void)hipFree(w->d_vals);
  if (w->d_flag) (void)hipFree(w->d_flag);
  if (w->h_in) (void)hipHostFree(w->h_in);
  if (w->st) (void)hipStreamDestroy(w->st);
  if (w->st2) (void)hipStreamDestroy(w->st2);
  if (w->ev) (void)hipEventDestroy(w->ev);
  if (w->ev_fork) (void)hipEventDestroy(w->ev_fork);
  if (w->ev_join) (void)hipEventDestroy(w->ev_join);
  if (w->ev_t0) (void)hipEventDestroy(w->ev_t0);
  if (w->ev_t1) (void)hipEventDestroy(w->ev_t1);
  delete w;
}

int zkhip_gpu_witness_run_batched(zkhip_gpu_witness* w, size_t n, const uint64_t* const* nested_vk, const uint64_t* const* nested_proofs,
                                  const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate) {
  return gpu_witness_run_impl(w, nullptr, n, nested_vk, nested_proofs, nested_inputs, d_z_out, primary_inputs, degenerate, witness_env_wpg(), witness_env_segment(), -1);
}
// the same for batches of ONE registered application: MASKED assignments (zeros at the application's constant positions), ready for
// zkhip_prover_prove_app_dev
int zkhip_gpu_witness_run_batched_app(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_proofs,
                                      const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate) {
  if (!app) return fail(ZKHIP_ERR_ARG, "null pointer");
  return gpu_witness_run_impl(w, app, n, nullptr, nested_proofs, nested_inputs, d_z_out, primary_inputs, degenerate, witness_env_wpg(), witness_env_segment(), -1);
}
// Test hook: either of the two above with witness_launch's knobs given by the caller (0 = the process-wide default; waves: 0 = auto)
int zkhip_internal_gpu_witness_run_wide(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_vk, const uint64_t* const* nested_proofs,
                                        const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate, int witnesses_per_workgroup,
                                        unsigned segment_chunks, int waves) {
  if (!witness_waves_ok(waves)) return fail(ZKHIP_ERR_ARG, "waves per witness: 0 (auto), 1, 2, 4, 8 or 16");
  if (witnesses_per_workgroup != 0 && witnesses_per_workgroup != 1 && witnesses_per_workgroup != 2 && witnesses_per_workgroup != 4)
    return fail(ZKHIP_ERR_ARG, "witnesses per workgroup: 0 (default), 1, 2 or 4");
  if (segment_chunks > (1u << 20)) return fail(ZKHIP_ERR_ARG, "segment: at most 2^20 chunks");
  return gpu_witness_run_impl(w, app, n, nested_vk, nested_proofs, nested_inputs, d_z_out, primary_inputs, degenerate,
                              witnesses_per_workgroup ? (uint32_t)witnesses_per_workgroup : witness_env_wpg(), segment_chunks ? segment_chunks : witness_env_segment(), waves);
}
int zkhip_internal_gpu_witness_run(zkhip_gpu_witness* w, zkhip_aggregator_app* app, size_t n, const uint64_t* const* nested_vk, const uint64_t* const* nested_proofs,
                                   const uint64_t* const* nested_inputs, void* d_z_out, uint64_t* primary_inputs, int* degenerate, int witnesses_per_workgroup,
                                   unsigned segment_chunks) {
  return zkhip_internal_gpu_witness_run_wide(w, app, n, nested_vk, nested_proofs, nested_inputs, d_z_out, primary_inputs, degenerate, witnesses_per_workgroup, segment_chunks, 1);
}

int zkhip_gpu_witness_run(zkhip_gpu_witness* w, const uint64_t* nested_vk, const uint64_t* nested_proofs, const uint64_t* nested_inputs,
                          void* d_z_out, uint64_t* primary_inputs) {
  int deg = 0;
  int rc = zkhip_gpu_witness_run_batched(w, 1, &nested_vk, &nested_proofs, &nested_inputs, d_z_out, primary_inputs, &deg);
  if (rc == ZKHIP_OK && deg)
    return fail(ZKHIP_ERR_ARG, "GPU witness: an inversion met zero (degenerate input); use the host generator for this batch");
  return rc;
}

int zkhip_aggregator_witness_gpu(zkhip_aggregator* a, const uint64_t* nested_vk, const uint64_t* nested_proofs, const uint64_t* nested_inputs,
                                 uint64_t* z_out) {
  if (!a || !z_out) return fail(ZKHIP_ERR_ARG, "null pointer");
  zkhip_gpu_witness* w = nullptr;
  int rc = zkhip_gpu_witness_new(a, &w);
  if (rc != ZKHIP_OK) return rc;
  void* dz = nullptr;
  hipError_t e = hipMalloc(&dz, a->n_vars * 48);
  if (e != hipSuccess) { zkhip_gpu_witness_free(w); snprintf(t_err, sizeof t_err, "hipMalloc: %s", hipGetErrorString(e)); return ZKHIP_ERR_HIP; }
  rc = zkhip_gpu_witness_run(w, nested_vk, nested_proofs, nested_inputs, dz, nullptr);
  if (rc == ZKHIP_OK && hipMemcpy(z_out, dz, a->n_vars * 48, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ZKHIP_ERR_HIP, "copy of the assignment failed");
  (void)hipFree(dz);
  zkhip_gpu_witness_free(w);
  return rc;
}

int zkhip_gpu_witness_stats(zkhip_aggregator* a, size_t out[6]) {
  BIND_CUR();
  if (!a || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  WitnessProg P;
  const WitnessTape* T = nullptr;
  int rc = witness_prog(a, &P, &T, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  out[0] = T->n_recorded; out[1] = T->code.size(); out[2] = T->level_start.size() - 1; out[3] = T->n_mul; out[4] = T->n_inv; out[5] = T->consts.size() / 6;
  return ZKHIP_OK;
}

int zkhip_internal_witness_run_program(const zkhip_witness_program* p, const uint64_t* inputs, size_t batches, int witnesses_per_workgroup, unsigned segment_chunks,
                                       uint64_t* z_out, uint32_t* flags_out) {
  return zkhip_internal_witness_run_program_wide(p, inputs, batches, witnesses_per_workgroup, segment_chunks, 1, z_out, flags_out);
}

int zkhip_internal_witness_run_program_wide(const zkhip_witness_program* p, const uint64_t* inputs, size_t batches, int witnesses_per_workgroup, unsigned segment_chunks,
                                            int waves, uint64_t* z_out, uint32_t* flags_out) {
  if (const char* why = witness_program_check(p)) return fail(ZKHIP_ERR_ARG, why);
  if (!witness_waves_ok(waves)) return fail(ZKHIP_ERR_ARG, "waves per witness: 0 (auto), 1, 2, 4, 8 or 16");
  if (witnesses_per_workgroup != 1 && witnesses_per_workgroup != 2 && witnesses_per_workgroup != 4) return fail(ZKHIP_ERR_ARG, "witnesses per workgroup: 1, 2 or 4");
  if (segment_chunks < 1 || segment_chunks > (1u << 20)) return fail(ZKHIP_ERR_ARG, "segment: 1 .. 2^20 chunks");
  if (batches > 256) return fail(ZKHIP_ERR_ARG, "at most 256 batches");
  if (batches == 0) return ZKHIP_OK;                                      // validated, nothing to run: no device needed
  if ((p->n_inputs && !inputs) || (p->n_vars && !z_out) || !flags_out) return fail(ZKHIP_ERR_ARG, "null pointer");
  BIND_CUR();
  WitnessTape T;
  T.code.assign(p->code, p->code + p->n_pos); T.a.assign(p->a, p->a + p->n_pos); T.b.assign(p->b, p->b + p->n_pos);
  T.level_start.assign(p->level_start, p->level_start + p->n_levels + 1);
  T.chain_start = p->chain_start;
  T.out_ref.assign(p->out_ref, p->out_ref + p->n_vars);
  T.consts.assign(p->consts, p->consts + p->n_consts * 6);
  T.n_vars = p->n_vars; T.n_inputs = p->n_inputs;
  struct Dev {            // released on every exit path
    WitnessProgDev pd;
    void *in = nullptr, *vals = nullptr, *z = nullptr, *flags = nullptr;
    hipStream_t st = nullptr, st2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ~Dev() {
      witness_prog_free(&pd);
      for (void* q : {in, vals, z, flags}) if (q) (void)hipFree(q);
      if (st) (void)hipStreamDestroy(st);
      if (st2) (void)hipStreamDestroy(st2);
      if (ev_fork) (void)hipEventDestroy(ev_fork);
      if (ev_join) (void)hipEventDestroy(ev_join);
    }
  } d;
  int rc = witness_prog_upload(T, &d.pd, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  const size_t in_bytes = batches * p->n_inputs * 48, z_bytes = batches * p->n_vars * 48;
  API_HIP(hipMalloc(&d.in, in_bytes + 64));
  API_HIP(hipMalloc(&d.vals, batches * p->n_pos * witness_value_bytes + 64));
  API_HIP(hipMalloc(&d.z, z_bytes + 64));
  API_HIP(hipMalloc(&d.flags, batches * 4 + 64));
  API_HIP(hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking));
  API_HIP(hipStreamCreateWithFlags(&d.st2, hipStreamNonBlocking));
  API_HIP(hipEventCreateWithFlags(&d.ev_fork, hipEventDisableTiming));
  API_HIP(hipEventCreateWithFlags(&d.ev_join, hipEventDisableTiming));
  if (in_bytes) API_HIP(hipMemcpyAsync(d.in, inputs, in_bytes, hipMemcpyHostToDevice, d.st));
  API_HIP(hipMemsetAsync(d.flags, 0, batches * 4, d.st));
  witness_launch(d.pd.prog, T.level_start.data(), (const uint64_t*)d.in, (uint32_t*)d.vals, (uint64_t*)d.z, (uint32_t*)d.flags, (uint32_t)batches,
                 (uint32_t)witnesses_per_workgroup, segment_chunks, (uint32_t)waves, d.st, d.st2, d.ev_fork, d.ev_join);
  API_HIP(hipGetLastError());
  if (z_bytes) API_HIP(hipMemcpyAsync(z_out, d.z, z_bytes, hipMemcpyDeviceToHost, d.st));
  API_HIP(hipMemcpyAsync(flags_out, d.flags, batches * 4, hipMemcpyDeviceToHost, d.st));
  API_HIP(hipStreamSynchronize(d.st));
  API_HIP(hipStreamSynchronize(d.st2));
  return ZKHIP_OK;
}

// Host only: the recorded program of the circuit (pointers into the aggregator's own copy, valid until it is freed)
int zkhip_internal_witness_tape(zkhip_aggregator* a, zkhip_witness_program* out) {
  if (!a || !out) return fail(ZKHIP_ERR_ARG, "null pointer");
  const WitnessTape* T = nullptr;
  int rc = witness_tape_of(a, &T, t_err, sizeof t_err);
  if (rc != ZKHIP_OK) return rc;
  out->code = T->code.data(); out->a = T->a.data(); out->b = T->b.data(); out->n_pos = T->code.size();
  out->level_start = T->level_start.data(); out->n_levels = T->level_start.size() - 1;
  out->chain_start = T->chain_start;
  out->out_ref = T->out_ref.data(); out->n_vars = T->n_vars;
  out->consts = T->consts.data(); out->n_consts = T->consts.size() / 6;
  out->n_inputs = T->n_inputs;
  return ZKHIP_OK;
}

}  // extern "C"
