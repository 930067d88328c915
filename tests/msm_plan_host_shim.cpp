// zecale_amd/csrc/msm_plan.hpp (the MSM plan's arithmetic) behind a C interface for tests/test_msm_plan_host.py: plain g++, no HIP.
#include "../zecale_amd/csrc/msm_plan.hpp"

using namespace zkhip::plan;
typedef unsigned long long u64;

extern "C" {
u64 p_machine_fill() { return MACHINE_FILL; }
u64 p_total_terms(int K, u64 max_n, u64 given) { return total_terms(K, max_n, given); }
int p_digits(int c, int merged) { return digits(c, merged); }
void p_window_layout(int c, uint16_t* off, uint8_t* bits) { window_layout(c, off, bits); }
// out: LB, NP, bins, tile, hist_len; returns 0 when the plan is refused
int p_sort_plan(int c, int merged, int Wd, u64 nb, u64 max_n, u64 want_parts, uint32_t tile_knob, u64* out) {
  uint32_t LB, NP, bins, tile;
  size_t hist_len;
  if (!sort_plan(c, merged, Wd, nb, max_n, want_parts, tile_knob, LB, NP, bins, tile, hist_len)) return 0;
  out[0] = LB; out[1] = NP; out[2] = bins; out[3] = tile; out[4] = hist_len;
  return 1;
}
u64 p_ceil_div(u64 a, u64 b) { return ceil_div(a, b); }
u64 p_hist_m(u64 nb, uint32_t LB, u64 nbx) { return hist_m(nb, LB, nbx); }
u64 p_slice_rule(u64 m, u64 target) { return slice_rule(m, target); }
// out: S, T, slot_stride; returns 0 when the plan is refused
int p_slice_plan(u64 m_max, u64 nb, u64 target, u64 slot_words, u64* out) {
  uint32_t S, T, slot_stride;
  if (!slice_plan(m_max, nb, target, slot_words, S, T, slot_stride)) return 0;
  out[0] = S; out[1] = T; out[2] = slot_stride;
  return 1;
}
u64 p_slice_run(u64 m, u64 target, u64 mult, u64 live_buckets, uint32_t T_plan) { return slice_run(m, target, mult, live_buckets, T_plan); }
u64 p_level_bound(u64 m, u64 nb) { return level_bound(m, nb); }
u64 p_aff_m_cap(uint32_t aff_m) { return aff_m_cap(aff_m); }
uint32_t p_aff_lanes(uint32_t aff_m, int levels, u64 bound1) { return aff_lanes(aff_m, levels, bound1); }
uint32_t p_aff_outputs_per_lane(u64 m_out, uint32_t aff_m) { return aff_outputs_per_lane(m_out, aff_m); }
u64 p_aff_scratch_bytes() { return AFF_SCRATCH_BYTES; }
uint32_t p_lock_min_live(int cus) { return lock_min_live(cus); }
int p_lo_bits(int c) { return lo_bits(c); }
int p_hi_bits(int c) { return hi_bits(c); }
int p_tree_fan_in(int L, u64 n_in, uint32_t left, u64 quad_below) { return tree_fan_in(L, n_in, left, quad_below); }
int p_group_fan_in(int L, u64 n, u64 G) { return tree_fan_in(L, n, (uint32_t)(n / G), 0); }      // as stage_reduce asks
u64 p_cap_entries(int Wd, u64 total_terms) { return cap_entries(Wd, total_terms); }
u64 p_cap_block_tot(u64 nb, u64 hist_len, u64 lock_keys) { return cap_block_tot(nb, hist_len, lock_keys); }
u64 p_cap_fix_list(uint32_t T) { return cap_fix_list(T); }
u64 p_cap_fix_short(uint32_t T) { return cap_fix_short(T); }
u64 p_cap_segS(u64 nb) { return cap_segS(nb); }
u64 p_cap_segR(u64 nb, int W) { return cap_segR(nb, W); }
u64 p_cap_sumR(u64 nb, int W, int L) { return cap_sumR(nb, W, L); }
u64 p_cap_Rlevels(int W) { return cap_Rlevels(W); }
u64 p_cap_hilo(int W, int c) { return cap_hilo(W, c); }
}
