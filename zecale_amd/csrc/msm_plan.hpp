// The arithmetic of an MSM plan (msm.hip: msm_plan_init, msm_launch_multi): how big every buffer is, how many items every launch
// handles.  Integers only, no HIP: tests/test_msm_plan_host.py asks the functions the driver asks.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
namespace zkhip::plan {
constexpr int SCALAR_BITS = 378;           // scalars < 2^377, +1 bit for the signed-digit carry
constexpr size_t MACHINE_FILL = 131072;    // lanes resident at two waves per SIMD: 256 CUs x 8 waves x 64 lanes
constexpr size_t POINT_WORDS = 108;        // a point of the reduction buffers: four coordinates of 27 words
constexpr size_t AFF_SCRATCH_BYTES = 108;  // prefix-product scratch of a batched-affine level, per output: one coordinate
inline size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
// terms of ALL jobs of one launch sequence: K * max_n unless the caller knows better (slices, boundary slots, the zero fill scale with it)
inline size_t total_terms(int K, size_t max_n, size_t given) {
  if (given == 0 || given > (size_t)K * max_n) given = (size_t)K * max_n;
  return (given < max_n && K == 1) ? max_n : given;
}
// W = ceil(378 / c) windows tile exactly 378 bits; the top W*c - 378 of them get c-1 bits
inline void window_layout(int c, uint16_t* off, uint8_t* bits) {
  const int W = (SCALAR_BITS + c - 1) / c, n_small = W * c - SCALAR_BITS;
  for (int w = 0, bit = 0; w < W; bit += bits[w++]) {
    off[w] = (uint16_t)bit;
    bits[w] = (uint8_t)(w >= W - n_small ? c - 1 : c);
  }
}
// digits per scalar; merged == 2, width-(c+1) NAF: digits at least c+1 bits apart, +1 for the final carry
inline int digits(int c, int merged) { return merged == 2 ? SCALAR_BITS / (c + 1) + 2 : (SCALAR_BITS + c - 1) / c; }
// bucket sort: parts of 2^LB buckets (LB <= 10: k_bucket_sort keeps a part's counters in LDS); small bucket windows get smaller parts
// so that k_bucket_sort has about want_parts workgroups; `tile` scalars per block of k_digit_pass, at most 1024 blocks.  false: refused
inline size_t hist_m(size_t nb, uint32_t LB, size_t nbx) { return (nb >> LB) * nbx + 1; }      // hist[part][block] + the total
inline bool sort_plan(int c, int merged, int Wd, size_t nb, size_t max_n, size_t want_parts, uint32_t tile_knob,
                      uint32_t& LB, uint32_t& NP, uint32_t& bins, uint32_t& tile, size_t& hist_len) {
  const size_t B = (size_t)1 << (c - 1);
  LB = (uint32_t)(c - 1 < 10 ? c - 1 : 10);
  while (LB > 6 && (nb >> LB) < want_parts && (B >> (LB - 1)) * (merged ? 1 : (size_t)Wd) <= 4096) LB--;
  NP = (uint32_t)(B >> LB);
  bins = merged ? NP : NP * (uint32_t)Wd;
  for (tile = tile_knob & ~255u; ceil_div(max_n, tile) > 1024;) tile *= 2;
  hist_len = hist_m(nb, LB, max_n ? ceil_div(max_n, tile) : 1);
  return (size_t)bins * 8 <= 60 * 1024;      // LDS of k_digit_pass<1>: counters + bases
}
// the slice rule: every lane gets the same number of point operations - whole machine fills at ~`target` entries per lane, at least 16
inline size_t slice_rule(size_t m, size_t target) {
  const size_t fills = ceil_div(m, MACHINE_FILL * target), S = ceil_div(m, MACHINE_FILL * (fills < 1 ? 1 : fills));
  return S < 16 ? 16 : S;
}
// The plan's slices for at most m_max entries.  The slot array (nb buckets + two boundary slots per slice) is addressed through ONE
// buffer descriptor, slot_words x 4 bytes x slots < 4 GiB: large inputs get longer slices instead of more of them.  false: refused.
inline bool slice_plan(size_t m_max, size_t nb, size_t target, size_t slot_words, uint32_t& S_out, uint32_t& T, uint32_t& slot_stride) {
  size_t S = slice_rule(m_max, target);
  const size_t max_slots = (((size_t)1 << 32) - 1) / (slot_words * 4);
  if (nb + 64 >= max_slots) return false;
  while (nb + 2 * ceil_div(m_max, S) >= max_slots) S += (S + 7) / 8;
  S_out = (uint32_t)S;
  T = (uint32_t)ceil_div(m_max, S);
  slot_stride = (uint32_t)(nb + 2 * (size_t)T);
  return (size_t)slot_stride * slot_words * 4 < ((size_t)1 << 32);
}
// One launch's slice length for ITS m entries: stream_mult times longer for provers that share the chip; a bucket (of live_buckets)
// should span at most ~3 slices, longer chains of pieces take a workgroup each in the stitching; never more slices than T_plan.
inline size_t slice_run(size_t m, size_t target, size_t stream_mult, size_t live_buckets, uint32_t T_plan) {
  size_t S = slice_rule(m, target) * stream_mult;
  const size_t avg = m / (live_buckets ? live_buckets : 1);
  if (S < (avg + 1) / 2) S = (avg + 1) / 2;
  while (ceil_div(m, S) > T_plan) S++;
  return S;
}
// batched-affine levels: a bound on level l+1 from a bound on level l, ceil(n/2) summed over at most min(nb, m) non-empty buckets
inline size_t level_bound(size_t m, size_t nb) { return (m + (m < nb ? m : nb)) / 2; }
inline size_t aff_m_cap(uint32_t aff_m) { return (size_t)aff_m * 3 / 2; }       // a launch may use up to 1.5 aff_m outputs per lane
// lanes per launch: the scratch inside one buffer descriptor; no more than the first level (at most bound1 outputs) needs
inline uint32_t aff_lanes(uint32_t aff_m, int levels, size_t bound1) {
  uint32_t lanes = 1u << 18;
  while ((size_t)lanes * aff_m_cap(aff_m) * AFF_SCRATCH_BYTES >= ((size_t)1 << 32)) lanes >>= 1;
  const size_t need = ceil_div(bound1, aff_m);
  return (levels > 0 && need < lanes) ? (uint32_t)((need + 255) & ~(size_t)255) : lanes;
}
// outputs per lane of one level: as close to aff_m as whole machine fills allow (a partial last fill runs at a fraction of the chip)
inline uint32_t aff_outputs_per_lane(size_t m_out, uint32_t aff_m) {
  const size_t rounds = (m_out + MACHINE_FILL * aff_m / 2) / (MACHINE_FILL * aff_m);
  const size_t mm = rounds < 1 ? aff_m : ceil_div(m_out, MACHINE_FILL * rounds);
  return (uint32_t)(mm > aff_m_cap(aff_m) ? aff_m_cap(aff_m) : mm);
}
// non-empty buckets a launch needs for the lockstep route: two waves for each of a CU's four SIMDs
inline uint32_t lock_min_live(int cus) { return 64u * 2u * 4u * (uint32_t)(cus > 0 ? cus : 256); }
// bucket reduction: the bucket index splits as j = hi * R + lo, R = 2^lo_bits, H = 2^hi_bits, then G = 2 W groups of N = max(R, H) = R
inline int lo_bits(int c) { return (c - 1 + 1) / 2; }
inline int hi_bits(int c) { return (c - 1) - lo_bits(c); }
// fan-in of a row / column tree level: L while it is throughput-bound (one lane per output); 2 once it is latency-bound (a quad per
// output, ONE addition deep: the chain of dependent additions shrinks from 3 log4 to log2 of its length); at most the `left` items of a row.
// (Fan-in 4 for the latency-bound levels - the second level on quads, seven launches less per MSM - was measured beside this and
// does not gain: profiles/msm_chain_ab.txt.)  quad_below = 0: never latency-bound.
inline int tree_fan_in(int L, size_t n_in, uint32_t left, size_t quad_below) {
  for (L = n_in / (size_t)L < quad_below ? 2 : L; (uint32_t)L > left;) L >>= 1;
  return L;
}
// The tail of the reduction: per group g of N items (N a power of two) the weighted sum F_g = sum_i (i+1) item_i by BIT PLANES,
//   F_g = sum_j 2^j P_{g,j},  P_{g,j} = the sum of the items whose weight i+1 has bit j set   (weights 1 .. N: log2 N + 1 planes),
// plus, for a NAF plan, one plane that takes every item (the plain total).  The planes are plain tree sums over a (plane, group,
// item) grid, one quad per output and one launch per level; the first level selects by weight bit.
constexpr int TAIL_FAN_IN = 4;             // three additions deep per launch: a launch's fixed cost is worth about three quad additions
inline int tail_weight_planes(size_t N) { int b = 0; while (((size_t)1 << b) <= N) b++; return b; }      // bits of N
inline int tail_planes(size_t N, bool total) { return tail_weight_planes(N) + (total ? 1 : 0); }
inline int tail_fan_in(size_t left) { return left < (size_t)TAIL_FAN_IN ? (int)left : TAIL_FAN_IN; }      // items of a group that are left
inline int tail_levels(size_t N) { int l = 0; for (size_t left = N; left > 1; left /= (size_t)tail_fan_in(left)) l++; return l; }
// outputs of level `level` (0: the selecting one): planes x G groups x what is left of a group
inline size_t tail_level_outputs(int planes, int G, size_t N, int level) {
  size_t left = N;
  for (int l = 0; l <= level && left > 1; l++) left /= (size_t)tail_fan_in(left);
  return (size_t)planes * (size_t)G * left;
}
// the two ping-pong buffers of the levels: level 0 writes [0], level 1 [1], ...; the last level's output is where the planes are combined
inline size_t cap_tail(int W, size_t N, int which) { return tail_level_outputs(tail_planes(N, true), 2 * W, N, which) + 1; }
// capacities of the plan's buffers, in points of POINT_WORDS words unless stated
// (cap_segR, cap_sumR, cap_Rlevels: the buffers of the recursion the plane form replaced; the plan no longer allocates them)
inline size_t cap_entries(int Wd, size_t total_terms) { return (size_t)Wd * total_terms + 1; }      // words; `pairs`: as many uint2
// words: the block totals of the longest scan (slice weights, sort histogram, bucket order), with room for words [0..2] after them
inline size_t cap_block_tot(size_t nb, size_t hist_len, size_t lock_keys) { return std::max({nb, hist_len, lock_keys * ceil_div(nb, 1024)}) / 1024 + 4; }
inline size_t cap_fix_list(uint32_t T) { return (size_t)T / 5 + 2; }       // uint2: buckets of more than four F pieces, at most T / 5
inline size_t cap_fix_short(uint32_t T) { return (size_t)T / 2 + 2; }      // uint2: buckets of two to four F pieces, at most T / 2
inline size_t cap_segS(size_t nb) { return nb / 2 + 1; }                   // S ping-pong of the row tree and the recursion; colS alike
inline size_t cap_segR(size_t nb, int W) { return nb / 2 + 64 * (size_t)W; }      // one R array per level, back to back (sum < nb/3 at L = 4)
inline size_t cap_sumR(size_t nb, int W, int L) { return nb / L / L + 4 * (size_t)W + 1; }
inline size_t cap_Rlevels(int W) { return (size_t)32 * 2 * W; }            // G points for each of at most 32 levels
inline size_t cap_hilo(int W, int c) { return ((size_t)2 * W << lo_bits(c)) + 8; }      // G x N
}  // namespace zkhip::plan
