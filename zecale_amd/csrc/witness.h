// Internal interface of the GPU witness generator (witness.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "aggregator_internal.h"
#include "witness_tape.h"

namespace zkhip {
constexpr int WT_SUBK_LEVELS = 12;        // K = 2^0 .. 2^11
struct WitnessProg {
  const uint8_t* code;
  const int32_t *a, *b;
  const uint32_t* level_start;
  const int32_t* out_ref;
  const uint32_t* consts;          // a value slot each: 14 limbs of the device form in 16 words
  uint32_t n_levels, n_pos, n_vars, n_inputs;
  uint32_t chain_start;            // positions [chain_start, n_pos): the key-hash chain (k_witness_chain)
  const uint32_t* subk;            // WT_SUBK_LEVELS value slots: 2^k r in subtraction-safe limbs
  uint32_t mu;                     // floor(2^390 / r) or one less (w_reduce)
};
// a program's device copy (seven buffers) and the argument block the kernels take
struct WitnessProgDev {
  WitnessProg prog;
  void* bufs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};
// uploads a recorded program to the calling thread's current device / frees it (the device must be current)
int witness_prog_upload(const WitnessTape& T, WitnessProgDev* out, char* err, size_t errlen);
void witness_prog_free(WitnessProgDev* pd);
// the program of `a` on the calling thread's current device (recorded and uploaded on first use)
int witness_prog(zkhip_aggregator* a, WitnessProg* out, const WitnessTape** tape, char* err, size_t errlen);
// the recorded program alone (host code: no device needed); it lives as long as `a`
int witness_tape_of(zkhip_aggregator* a, const WitnessTape** tape, char* err, size_t errlen);
// the process-wide defaults of witness_launch's two knobs: ZKHIP_WITNESS_WPG (1 | 2 | 4, default 4) and ZKHIP_WITNESS_SEGMENT
// (64 .. 2^20 chunks, default 2,048), each read once
uint32_t witness_env_wpg();
uint32_t witness_env_segment();
// wpg: witnesses per workgroup, a wave each (1, 2 or 4; anything else = 4; the narrow kernel only); seg: chunks of the levelled
// program per launch (>= 1; the wide kernels run whole levels, about seg chunks of them); waves: 1 = k_witness, a wave per witness,
// 2 | 4 | 8 | 16 = k_witness_wide, a workgroup of that many waves per witness, 0 = what witness_plan picks for the program;
// h_level_start: the program's level_start on the HOST (n_levels + 1 entries; without it the launch is narrow);
// inputs: batches x n_inputs x 6 u64 (ABI form: nested key | proofs | inputs); values: batches x n_pos x 16 u32 (witness_value_bytes);
// z: batches x n_vars x 6 u64 (ABI form); flags: one word per batch, set when an inversion met zero (cleared by the caller)
constexpr size_t witness_value_bytes = 64;      // one value slot
void witness_launch(const WitnessProg& P, const uint32_t* h_level_start, const uint64_t* d_inputs, uint32_t* d_values, uint64_t* d_z, uint32_t* d_flags,
                    uint32_t batches, uint32_t wpg, uint32_t seg, uint32_t waves, hipStream_t st, hipStream_t st_chain, hipEvent_t ev_fork, hipEvent_t ev_join);
// Host only.  steps: the sum over levels of ceil(chunks of the level / waves), the chunk-times on the critical path; waves: the
// width asked for, or for 0 the one auto picks - 1 below 1.5 chunks per level on average.
struct WitnessPlan { size_t chunks, levels, steps, value_bytes; uint32_t waves; };
WitnessPlan witness_plan(const uint32_t* level_start, size_t n_levels, size_t n_pos, uint32_t waves);
uint32_t witness_auto_waves(size_t chunks, size_t levels);      // what auto picks: two numbers of the program, no walk over its levels
bool witness_waves_ok(int waves);               // 0, 1, 2, 4, 8, 16
}  // namespace zkhip
