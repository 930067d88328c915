// Multi-scalar multiplication in G1 / G2 of BW6-761 on gfx950 (Pippenger / bucket method with
// signed digits).  Replaces the five libff::multi_exp calls the reference reaches through
// wsnarkT::generate_proof (libzecale/circuits/aggregator_circuit.tcc:168).
//
// Pipeline (all kernels hand-written for wave64; one lane owns one field element, see fp29.cuh):
//   k_bases_to_dev      ABI affine points -> packed device-form points (once per base set)
//   k_table_build       optional, once per resident base set: 2^(off_w) P_i for every window position (window table)
//   k_digit_pass<0/1>   Montgomery scalars -> canonical -> signed c-bit digits; counted, then placed, per PART of the bucket range (LDS)
//   k_scan_*            exclusive prefix sum of the (part, block) histogram
//   k_bucket_sort       a workgroup per part orders its entries by bucket: bucket-ordered list of (point index, sign), offsets, counts
//   k_accumulate        one lane per fixed-size SLICE of the sorted list: XYZZ mixed additions   <-- dominant
//   k_fixup_fold / k_fixup  stitch the buckets that slice boundaries cut
//   k_sum_lds / k_sum   bucket reduction  sum_j (j+1) B_j : two-level split of the bucket index, row and column trees
//   k_plane_sum / k_plane_combine   the two small weighted sums per bucket window by bit planes, then R * hi + lo
// Plain base sets: one bucket window per digit position, and the last step, sum_w 2^(off_w) W_w (about 380 serial
// doublings of ONE point), runs on the host.  Table-backed base sets: ONE bucket window for all digit positions (nothing
// left to combine), and up to five MSMs share one launch sequence with a bucket window each (msm_launch_multi).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <vector>

#include "ec_affine.cuh"
#include "ec_edw.cuh"
#include "host_field.hpp"
#include "msm.h"
#include "msm_plan.hpp"
#include "wait.h"


namespace zkhip {

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------

// one thread per point: 24 u64 (x, y in ABI Montgomery form; all-zero = infinity) -> AffPacked
__global__ void __launch_bounds__(256) k_bases_to_dev(const uint64_t* __restrict__ in, AffPacked* __restrict__ out,
                                                       uint8_t* __restrict__ inf_flags /* may be null */, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t x[12], y[12];
  uint64_t nz = 0;
#pragma unroll
  for (int k = 0; k < 12; k++) { x[k] = in[i * 24 + k]; y[k] = in[i * 24 + 12 + k]; nz |= x[k] | y[k]; }
  AffPacked p;
  if (nz == 0) {
#pragma unroll
    for (int k = 0; k < 24; k++) { p.x[k] = 0; p.y[k] = 0; }
  } else {
    Fq fx = fp_cond_sub_p(fp_from_abi<FqParams>(x));
    Fq fy = fp_cond_sub_p(fp_from_abi<FqParams>(y));
    fp_pack32<FqParams>(fx, p.x);
    fp_pack32<FqParams>(fy, p.y);
  }
  out[i] = p;
  if (inf_flags) inf_flags[i] = (nz == 0) ? 1 : 0;
}

// Window layout: W windows tile exactly 378 bits (scalars < r < 2^377, plus one bit for the
// signed-digit carry); window sizes differ by at most one bit (c or c-1) so that no window is a
// sparsely populated remainder - a short top window would funnel all n points of that window
// into a few hundred buckets, i.e. into a few hundred lanes.
struct WindowPlan {
  uint16_t off[96];   // first bit of window w
  uint8_t bits[96];   // size of window w
};

// ---- bucket sort of the digits: two passes with LDS histograms, no global atomics --------------------------------------
// A digit of a scalar is an ENTRY (which point, which sign) for a BUCKET (global index in [0, nb): window * B + |d| - 1, or
// job * B + |d| - 1 when all digit positions of a job share one bucket window).  k_accumulate wants the entries ordered by
// bucket.  bucket = part << LB | low:
//   k_digit_pass<0>   a block takes a tile of scalars, extracts their digits and counts them per PART in LDS; the counts go out
//                     as hist[part][block]
//   k_scan_*          exclusive scan of hist in (part, block) order: where each block's entries of each part start
//   k_digit_pass<1>   the same blocks extract the same digits again (two Fr multiplications per scalar: cheaper than storing
//                     and re-reading 4 bytes per digit), take their ranks from an LDS counter and write (entry, low bucket
//                     bits) pairs - one 8-byte store each -, grouped by part
//   k_bucket_sort     a workgroup per part: LDS histogram over the low bits, scan, placement - and the per-bucket
//                     offsets / counts the accumulation needs fall out on the way
// (Rounds 1-2 counted in global memory: one atomic per digit in the histogram and one RETURNING atomic per digit in the
// scatter, 1.6 ms of a 2^20-term MSM - 20 M device-scope atomics resolve in the memory-side cache, not in an XCD's L2.)
// The order of the entries inside a bucket is not defined (the sum is).
struct DigitJobs {
  const uint64_t* scalars[MSM_MAX_JOBS];
  const uint8_t* inf_flags[MSM_MAX_JOBS];
  size_t n[MSM_MAX_JOBS], tab_stride[MSM_MAX_JOBS];
  int mode[MSM_MAX_JOBS];
};
struct SortGeom {
  uint32_t LB;          // low bucket bits: a part is 2^LB consecutive buckets
  uint32_t NP;          // parts per bucket window (B >> LB)
  uint32_t bins;        // parts a block can hit: NP (merged plans: its job's window) or W * NP (plain plans: every window)
  uint32_t nbx;         // blocks per job = row length of hist
  uint32_t tile;        // scalars per block
  uint32_t nparts;      // nb >> LB
};

// canonical 32-bit words (13, the last one zero) of scalar i of a job
__device__ __forceinline__ void scalar_words(const uint64_t* __restrict__ scalars, size_t i, int mode, uint32_t* w32) {
  uint64_t s[6];
#pragma unroll
  for (int k = 0; k < 6; k++) s[k] = scalars[i * 6 + k];
  if (mode == 1) {
    fp_abi_to_canonical_words<FrParams>(s, w32);
  } else {
#pragma unroll
    for (int k = 0; k < 6; k++) { w32[2 * k] = (uint32_t)s[k]; w32[2 * k + 1] = (uint32_t)(s[k] >> 32); }
    if (mode == 2) {   // packed device form (value * 2^406, < 2^384), as the NTT kernels leave it
      Fp<FrParams> v = fp_unpack32<FrParams>(w32), one_raw = fp_zero<FrParams>();
      one_raw.l[0] = 1;
      fp_pack32<FrParams>(fp_cond_sub_p(fp_mul(v, one_raw)), w32);
    }
  }
  w32[12] = 0;
}

// PASS 0: count.  PASS 1: place.  NAF: scalars recoded in width-(c+1) non-adjacent form (merged == 2 plans).
// Dynamic LDS: cnt[bins] (+ base[bins] in pass 1).
template <int PASS, bool NAF>
__global__ void __launch_bounds__(256) k_digit_pass(DigitJobs jobs, int c, int W, WindowPlan plan, int merged, SortGeom ge,
                                                     uint32_t* __restrict__ hist, uint2* __restrict__ pairs) {
  extern __shared__ uint32_t sh_dyn[];
  __shared__ uint32_t s_w[NAF ? 13 : 1][256];
  uint32_t* s_cnt = sh_dyn;
  uint32_t* s_base = sh_dyn + ge.bins;
  const uint32_t job = blockIdx.y, bx = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  const size_t n = jobs.n[job];
  const uint64_t* __restrict__ scalars = jobs.scalars[job];
  const uint8_t* __restrict__ inf_flags = jobs.inf_flags[job];
  const int mode = jobs.mode[job];
  const size_t tab_stride = jobs.tab_stride[job];
  const uint32_t g0 = merged ? job * ge.NP : 0u;                 // first part this block can hit
  const uint32_t lb_mask = (1u << ge.LB) - 1u;
  for (uint32_t j = tid; j < ge.bins; j += 256) {
    s_cnt[j] = 0;
    if (PASS == 1) s_base[j] = hist[(size_t)(g0 + j) * ge.nbx + bx];
  }
  if (PASS == 0 && bx == 0 && job == 0 && tid == 0) hist[(size_t)ge.nparts * ge.nbx] = 0;     // the scan leaves the total here
  __syncthreads();
  // one digit: bin = part inside this block's range, low = bucket bits below the part, e = entry word
  auto emit = [&](bool valid, bool hot, uint32_t bin, uint32_t low, uint32_t e) {
    // "scalar == 1" (boolean-heavy witnesses) puts a third of all points into ONE bucket: its lanes share one LDS operation
    const unsigned long long hot_mask = __ballot(valid && hot);
    if (hot_mask) {
      const int leader = __ffsll((long long)hot_mask) - 1;
      const uint32_t cntw = (uint32_t)__popcll(hot_mask);
      if (PASS == 0) {
        if ((int)lane == leader) atomicAdd(&s_cnt[bin], cntw);
      } else {
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(&s_cnt[bin], cntw);
        base = __shfl(base, leader);
        if (valid && hot) {
          const uint32_t pos = s_base[bin] + base + (uint32_t)__popcll(hot_mask & ((1ull << lane) - 1ull));
          pairs[pos] = make_uint2(e, low);
        }
      }
    }
    if (valid && !hot) {
      if (PASS == 0) {
        atomicAdd(&s_cnt[bin], 1u);
      } else {
        const uint32_t pos = s_base[bin] + atomicAdd(&s_cnt[bin], 1u);
        pairs[pos] = make_uint2(e, low);
      }
    }
  };
  for (uint32_t it = 0; it < ge.tile; it += 256) {
    size_t i = (size_t)bx * ge.tile + it + tid;
    const bool live = i < n;
    if ((size_t)bx * ge.tile + it >= n) break;              // (block-uniform)
    if (!live) i = n - 1;                                   // whole waves stay in the loops: the hot-bucket path is wave-wide
    const bool skip0 = !live || (inf_flags && inf_flags[i]);   // a base at infinity contributes nothing: drop it here
    uint32_t w32[13];
    scalar_words(scalars, i, mode, w32);
    if constexpr (NAF) {
      // Width-(c+1) non-adjacent form: ODD signed digits |d| < 2^c at arbitrary bit positions, at least c+1 bits apart - 378 / (c + 2)
      // digits on average instead of 378 / c, over the same 2^(c-1) buckets (bucket = (|d| - 1) / 2, weight 2 * bucket + 1: the
      // reduction returns sum (bucket + 1) S_b and sum S_b, the finish makes 2 F - S of them).  The entry of a digit at bit position
      // j points at level j of the table (2^j P_i).  The LAST digit of a scalar covers only the bits that are left, so small
      // magnitudes are over-represented - LDS counters take that in their stride.
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 13; k++) s_w[k][tid] = w32[k];
      __syncthreads();
      const int wbits = c + 1;
      int pos = 0, slot = 0;
      uint32_t carry = 0;
      while (pos < 379 && slot < W) {
        const int j = pos >> 5, sh = pos & 31;
        uint64_t v = (uint64_t)s_w[j < 13 ? j : 12][tid] >> sh;
        if (j < 12) v |= (uint64_t)s_w[j + 1][tid] << (32 - sh);
        if (j >= 12) v = 0;
        const uint32_t v32 = (uint32_t)v;
        // bits + carry: skip the run that produces zeros (zeros without a carry, ones with it)
        const uint32_t run = carry ? ~v32 : v32;
        if ((run & 1u) == 0) { pos += run ? (__ffs((int)run) - 1) : 32; continue; }
        uint32_t win = (v32 & ((1u << wbits) - 1)) + carry;            // odd
        int32_t d;
        if (win > (1u << (wbits - 1))) { d = (int32_t)win - (int32_t)(1u << wbits); carry = 1; }
        else { d = (int32_t)win; carry = 0; }
        const uint32_t mag = d < 0 ? (uint32_t)(-d) : (uint32_t)d;
        const bool skip = skip0 || (inf_flags && pos > 0 && inf_flags[(size_t)pos * tab_stride + i]);      // 2^pos P_i = O
        if (!skip) {
          const uint32_t bl = (mag - 1) >> 1;
          const uint32_t e = (uint32_t)((size_t)pos * tab_stride + i) | (d < 0 ? 0x80000000u : 0u);
          // (divergent loop: no wave-wide aggregation here)
          if (PASS == 0) {
            atomicAdd(&s_cnt[bl >> ge.LB], 1u);
          } else {
            const uint32_t p_ = s_base[bl >> ge.LB] + atomicAdd(&s_cnt[bl >> ge.LB], 1u);
            pairs[p_] = make_uint2(e, bl & lb_mask);
          }
        }
        slot++;
        pos += wbits;
      }
    } else {
      uint32_t carry = 0;
      for (int w = 0; w < W; w++) {
        const int bit = plan.off[w], cw = plan.bits[w];
        const int j = bit >> 5, sh = bit & 31;
        uint64_t v = (uint64_t)w32[j] >> sh;
        if (j + 1 < 13) v |= (uint64_t)w32[j + 1] << (32 - sh);
        uint32_t d = ((uint32_t)v & ((1u << cw) - 1)) + carry;
        int32_t sd;
        if (d > (1u << (cw - 1))) { sd = (int32_t)d - (int32_t)(1u << cw); carry = 1; }
        else { sd = (int32_t)d; carry = 0; }
        const bool skip = skip0 || (merged && w > 0 && inf_flags && inf_flags[(size_t)w * tab_stride + i]);   // 2^(c w) P_i = O
        const bool valid = !skip && sd != 0;
        const uint32_t mag = sd < 0 ? (uint32_t)(-sd) : (uint32_t)sd;
        const uint32_t bw = valid ? mag - 1 : 0u;                                   // bucket inside its window
        const uint32_t bin = (merged ? 0u : (uint32_t)w * ge.NP) + (bw >> ge.LB);
        const uint32_t e = (uint32_t)(merged ? (size_t)w * tab_stride + i : i) | (sd < 0 ? 0x80000000u : 0u);
        emit(valid, mag == 1, bin, bw & lb_mask, e);
      }
    }
  }
  if (PASS == 0) {
    __syncthreads();
    for (uint32_t j = tid; j < ge.bins; j += 256) hist[(size_t)(g0 + j) * ge.nbx + bx] = s_cnt[j];
  }
}

// One workgroup per part g: its entries pairs[start, end) (grouped by part by k_digit_pass<1>) are ordered by their low bucket
// bits.  Writes offsets / counts of the part's 2^LB buckets (an empty bucket repeats the next offset) and the sorted entries.
__global__ void __launch_bounds__(512) k_bucket_sort(const uint32_t* __restrict__ hoff, SortGeom ge, const uint2* __restrict__ pairs,
                                                      uint32_t* __restrict__ entries,
                                                      uint32_t* __restrict__ offsets, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[1024], s_cur[1024], s_scan[512];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t start = hoff[(size_t)g * ge.nbx], end = hoff[(size_t)(g + 1) * ge.nbx];     // (hoff has nparts * nbx + 1 elements)
  const uint32_t NB = 1u << ge.LB;
  for (uint32_t j = tid; j < NB; j += 512) s_cnt[j] = 0;
  __syncthreads();
  const uint32_t len = end - start, rounds = (len + 511) / 512;
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t k = r * 512 + tid;
    const bool valid = k < len;
    const uint32_t lb = valid ? pairs[start + k].y : 0xffffu;
    const unsigned long long hot_mask = __ballot(lb == 0);       // the bucket of "digit 1" may hold a third of all entries
    if (hot_mask) {
      if ((int)lane == __ffsll((long long)hot_mask) - 1) atomicAdd(&s_cnt[0], (uint32_t)__popcll(hot_mask));
    }
    if (valid && lb != 0) atomicAdd(&s_cnt[lb], 1u);
  }
  __syncthreads();
  // exclusive scan of s_cnt[0 .. NB): two counters per thread
  const uint32_t c0 = (2 * tid < NB) ? s_cnt[2 * tid] : 0u, c1 = (2 * tid + 1 < NB) ? s_cnt[2 * tid + 1] : 0u;
  s_scan[tid] = c0 + c1;
  __syncthreads();
  for (int off = 1; off < 512; off <<= 1) {
    const uint32_t t_ = (tid >= (unsigned)off) ? s_scan[tid - off] : 0u;
    __syncthreads();
    s_scan[tid] += t_;
    __syncthreads();
  }
  const uint32_t ex = s_scan[tid] - (c0 + c1);
  if (2 * tid < NB) {
    s_cur[2 * tid] = ex;
    offsets[((size_t)g << ge.LB) + 2 * tid] = start + ex; counts[((size_t)g << ge.LB) + 2 * tid] = c0;
  }
  if (2 * tid + 1 < NB) {
    s_cur[2 * tid + 1] = ex + c0;
    offsets[((size_t)g << ge.LB) + 2 * tid + 1] = start + ex + c0; counts[((size_t)g << ge.LB) + 2 * tid + 1] = c1;
  }
  __syncthreads();
  for (uint32_t r = 0; r < rounds; r++) {
    const uint32_t k = r * 512 + tid;
    const bool valid = k < len;
    const uint2 pr = valid ? pairs[start + k] : make_uint2(0u, 0xffffu);
    const uint32_t lb = pr.y, e = pr.x;
    const unsigned long long hot_mask = __ballot(lb == 0);
    if (hot_mask) {
      const int leader = __ffsll((long long)hot_mask) - 1;
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(&s_cur[0], (uint32_t)__popcll(hot_mask));
      base = __shfl(base, leader);
      if (lb == 0) entries[start + base + (uint32_t)__popcll(hot_mask & ((1ull << lane) - 1ull))] = e;
    }
    if (valid && lb != 0) entries[start + atomicAdd(&s_cur[lb], 1u)] = e;
  }
}

// ---- exclusive scan over `m` u32 counters, 1024 per block ----
// (in and out may be the same array - the histogram is scanned in place -: no __restrict__ on them)
__global__ void __launch_bounds__(256) k_scan_local(const uint32_t* in, uint32_t* out, uint32_t* __restrict__ block_tot, size_t m) {
  __shared__ uint32_t sh[256];
  size_t base = (size_t)blockIdx.x * 1024 + (size_t)threadIdx.x * 4;
  uint32_t v[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { v[k] = (base + k < m) ? in[base + k] : 0; sum += v[k]; }
  sh[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    uint32_t t = (threadIdx.x >= (unsigned)off) ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t excl = sh[threadIdx.x] - sum;
#pragma unroll
  for (int k = 0; k < 4; k++) { if (base + k < m) out[base + k] = excl; excl += v[k]; }
  if (threadIdx.x == 255) block_tot[blockIdx.x] = sh[255];
}

__global__ void __launch_bounds__(1024) k_scan_tot(uint32_t* __restrict__ block_tot, size_t nb) {
  // single block, sequential over chunks of 1024
  __shared__ uint32_t sh[1024];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (size_t base = 0; base < nb; base += 1024) {
    size_t i = base + threadIdx.x;
    uint32_t v = (i < nb) ? block_tot[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      uint32_t t = (threadIdx.x >= (unsigned)off) ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nb) block_tot[i] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += sh[1023];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_scan_add(uint32_t* __restrict__ out, const uint32_t* __restrict__ block_tot, size_t m) {
  size_t base = (size_t)blockIdx.x * 1024 + (size_t)threadIdx.x * 4;
  uint32_t add = block_tot[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 4; k++) if (base + k < m) out[base + k] += add;
}

// Bucket accumulation, load-balanced: lane t owns a SLICE of the bucket-sorted entry list, whatever buckets it crosses.  A run of
// entries that covers a whole bucket is accumulated straight into that bucket's slot; a run cut by a slice boundary goes to a
// per-slice boundary slot (F = the slice starts inside the bucket, L = the slice ends inside it) and k_fixup stitches the pieces.
// All slots live in ONE array (one buffer descriptor; an array of structures, ec_mem.cuh): [0, nb) buckets, [nb, nb+T) F slots, [nb+T, nb+2T) L slots.
// Slices have equal WEIGHT, not equal length (round 4): the first entry of a bucket only OPENS a run - loads, no field arithmetic -
// so it weighs ZK_W_FIRST = 1 where an entry that is ADDED to a running sum weighs ZK_W_NEXT = 8.  Every lane then performs the same
// number of additions (to within one) and the openings ride along inside the iteration of the addition that follows them; with
// slices of equal length (rounds 1-3) every opening took a whole iteration of its wave: 7 % of the lane-iterations of a wrapping
// proof's launch, 5 % at 2^20 terms, did nothing.  (Thread-per-bucket loses ~45 % to the spread of bucket populations.)
// goff[b] = the weight in front of bucket b (exclusive scan of 8 count - 7 over the non-empty buckets, nb + 1 values); the entry at
// position p of bucket b starts at weight G(p) = goff[b] for p = offsets[b], goff[b] + 1 + 8 (p - offsets[b] - 1) otherwise; slice t
// holds the entries with t A <= G(p) < (t + 1) A.  The slot array's ZZ rows are zero-filled beforehand (all-zero ZZ = infinity), so
// empty buckets need no work.
// The Edwards accumulation (ec_edw.cuh) opens every run at the identity and ADDS its first entry: there every entry weighs
// ZK_W_NEXT (wf = ZK_W_NEXT below), the XYZZ accumulation passes wf = ZK_W_FIRST.
#define ZK_W_NEXT 8u
#define ZK_W_FIRST 1u
__global__ void __launch_bounds__(256) k_slice_weights(const uint32_t* __restrict__ counts, uint32_t* __restrict__ w, size_t nb, uint32_t wf) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nb) return;
  const uint32_t c = i < nb ? counts[i] : 0u;
  w[i] = c ? ZK_W_NEXT * c - (ZK_W_NEXT - wf) : 0u;
}
// first position p with G(p) >= x (M if there is none); *b_out: a bucket at or before the one that holds p
__device__ __forceinline__ uint32_t slice_pos(const uint32_t* __restrict__ goff, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
                                              uint32_t nb, uint32_t M, uint64_t x, uint32_t* b_out, uint32_t wf) {
  if (x >= (uint64_t)goff[nb]) { *b_out = nb - 1; return M; }
  uint32_t lo = 0, hi = nb;   // last b with goff[b] <= x: a non-empty bucket (an empty one repeats the value of the next non-empty one)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint64_t)goff[mid] <= x) lo = mid; else hi = mid;
  }
  *b_out = lo;
  const uint32_t g = goff[lo], off = offsets[lo], cnt = counts[lo];
  if ((uint64_t)g >= x) return off;
  const uint32_t j = (uint32_t)((x - g - wf + (ZK_W_NEXT - 1)) / ZK_W_NEXT) + 1u;      // first j >= 1 with g + wf + 8 (j - 1) >= x
  return off + (j < cnt ? j : cnt);
}
// slice of the entry at position p of bucket b
__device__ __forceinline__ uint32_t slice_of(const uint32_t* __restrict__ goff, const uint32_t* __restrict__ offsets, uint32_t b, uint32_t p, uint32_t A,
                                             uint32_t wf) {
  const uint32_t off = offsets[b];
  const uint64_t G = (uint64_t)goff[b] + (p == off ? 0u : wf + (uint64_t)ZK_W_NEXT * (p - off - 1));
  return (uint32_t)(G / A);
}
__device__ __forceinline__ uint32_t bucket_of(const uint32_t* __restrict__ offsets, uint32_t nb, uint32_t pos) {
  // last b with offsets[b] <= pos  (offsets is non-decreasing; empty buckets repeat the next offset)
  uint32_t lo = 0, hi = nb;   // invariant: offsets[lo] <= pos, (hi == nb or offsets[hi] > pos)
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (offsets[mid] <= pos) lo = mid; else hi = mid;
  }
  return lo;
}

// ZZ = 0 marks an empty slot (the point at infinity): the 27 ZZ words of every slot of the array of structures are cleared before a
// launch - a quarter of the array's bytes, as the limb-major layout's memset of its 27 ZZ rows was.  One word per lane, 27
// consecutive lanes per slot.
__global__ void __launch_bounds__(256) k_slots_clear_zz(uint32_t* __restrict__ slots, uint32_t n_slots) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n_slots * 27) return;
  const size_t s_ = i / 27, w = i % 27;
  slots[s_ * ZK_SLOT_WORDS + (size_t)CZZ * (ZK_SLOT_WORDS / 4) + w] = 0u;
}

// Several MSMs may share one launch (merged plans: bucket window k belongs to job k): the base set of a run is chosen
// by its bucket, b >> bshift (plain plans: one base set, bshift = 31).
// NJ = 1: a plan for single MSMs (the selection folds away); NJ = MSM_MAX_JOBS: the five MSMs of a proof in one launch.  Two
// instantiations, two kernel names in a trace: k_accumulate<1> and k_accumulate<5>.
struct BasePtrs { const AffPacked* p[MSM_MAX_JOBS]; };
template <int NJ> __device__ __forceinline__ const AffPacked* base_of(const BasePtrs& bp, uint32_t k) {
  const AffPacked* r = bp.p[0];
#pragma unroll
  for (int j = 1; j < NJ; j++) r = (k == (uint32_t)j) ? bp.p[j] : r;
  return r;
}

// Slice weight A.  The host sizes the slices for the entries that CAN occur (digit positions x finite bases: S_host entries each); the
// list the sort produced may be shorter - zero digits produce no entry (a boolean-heavy witness: most of them), recoded scalars
// have fewer digits than positions.  A launch that has the chip to itself (tight != 0) then shrinks the slices so that all T lanes
// of the grid get work: A = ceil((G + 1) / T), at least 16 additions' worth, never above the host's (so the slot array still fits).
// A prover that shares the chip with others keeps the longer slices (fewer cut buckets to stitch; the chip is full anyway).
__device__ __forceinline__ uint32_t slice_weight(uint32_t G, uint32_t T, uint32_t S_host, int tight) {
  const uint32_t a_host = S_host * ZK_W_NEXT;
  if (!tight) return a_host;
  const uint32_t a = (uint32_t)(((uint64_t)G + T) / T), a_min = 16u * ZK_W_NEXT;
  if (a < a_min) return a_host < a_min ? a_host : a_min;
  return a < a_host ? a : a_host;
}

// Closing a run: the four coordinates go to the run's slot (ec_mem.cuh: the slot array is an array of structures)
#define ZK_CLOSE_RUN(acc, xs, zz, zzz, ty)                                                                          \
  do {                                                                                                               \
    mem_st(acc, CX, lds_ld_packed(xs)); mem_st(acc, CZZ, lds_ld(zz)); mem_st(acc, CZZZ, lds_ld(zzz));             \
    mem_st(acc, CY, ty);                                                                                             \
  } while (0)

// entries == nullptr: the sorted list IS the dense point array bp.p[0] (the output of the batched-affine levels, k_affine_level):
// entry k is point k, never negated; a point may be the level encoding of infinity (skipped).
// EDW: bp.p[0] is a table of precomputed Edwards points (ec_edw.cuh) and the slots receive Edwards points (X | Y | Z | T in the
// X | Y | ZZ | ZZZ words; the stitching and the reduction go on in that model): every run starts at the identity, so every entry is one addition.
// Never dense.  NJ = 1: a single MSM; NJ = 4: the four G1 MSMs of a proof in one launch - bp.p[k] is job k's Edwards table, and a run
// takes its table from its bucket's window where it is opened (lanes of one wave are in different jobs: the lane carries the table
// until its next run).  Three kernels share this body: k_accumulate<NJ> (XYZZ), k_accumulate_edw and k_accumulate_edw_multi.
#define ZK_ACC_PARAMS                                                                                                                   \
  BasePtrs bp, int bshift, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,   \
      const uint32_t* __restrict__ goff, uint32_t nb, uint32_t S_host, int tight, uint32_t T, uint32_t* __restrict__ slots, uint32_t stride,      \
      uint32_t* __restrict__ fix_cnt /* [2] */, uint2* __restrict__ fix_short, uint2* __restrict__ fix_long,                                  \
      uint64_t* __restrict__ dbg_times /* null, or [waves][4]: tools/acc_probe.py */, int prio_mode,                                        \
      uint32_t* prio_board /* null, or one word per hardware wave slot */, uint32_t prio_tag
template <int NJ, bool EDW>
__device__ __forceinline__ void accumulate_impl(ZK_ACC_PARAMS) {
  static_assert(!EDW || NJ == 1 || NJ == 4, "the Edwards accumulation serves single MSMs and the four G1 MSMs of a proof");
  constexpr uint32_t wf = EDW ? ZK_W_NEXT : ZK_W_FIRST;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t dbg_t0 = dbg_times ? wall_clock64() : 0;
  const uint32_t M = offsets[nb - 1] + counts[nb - 1];
  const uint32_t A = slice_weight(goff[nb], T, S_host, tight);
  if (t >= T) return;
  uint32_t b, b1_;
  const uint32_t pos0 = slice_pos(goff, offsets, counts, nb, M, (uint64_t)t * A, &b, wf);
  if (pos0 >= M) return;
  const uint32_t pos1 = slice_pos(goff, offsets, counts, nb, M, (uint64_t)(t + 1) * A, &b1_, wf);
  while (offsets[b] + counts[b] <= pos0) b++;          // (the slice may start right behind the last entry of the bucket the search found)
  {
    // A bucket cut by slice boundaries leaves an L piece (slice t0, where it starts) and F pieces in the slices t0+1 .. t1.  The
    // slice that holds the FIRST F piece of a bucket with several of them puts the bucket on a list: (first F slot, number of F
    // pieces) - a short list (2 .. 4 pieces: one lane or quad folds them) and a long one (a workgroup each): k_fixup_fold.  One atomic per
    // wave and list.
    uint32_t span = 0, tF0 = 0;
    if (offsets[b] < pos0) {
      const uint32_t t0 = slice_of(goff, offsets, b, offsets[b], A, wf);
      tF0 = t0 + 1;
      span = slice_of(goff, offsets, b, offsets[b] + counts[b] - 1, A, wf) - t0;       // number of F pieces
      if (t != tF0) span = 0;
    }
    const bool is_short = span >= 2 && span <= 4, is_long = span > 4;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long ms = __ballot(is_short), ml = __ballot(is_long);
    if (ms) {
      const int leader = __ffsll((long long)ms) - 1;
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(&fix_cnt[0], (uint32_t)__popcll(ms));
      base = __shfl(base, leader);
      if (is_short) fix_short[base + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull))] = make_uint2(tF0, span);
    }
    if (ml) {
      const int leader = __ffsll((long long)ml) - 1;
      uint32_t base = 0;
      if ((int)lane == leader) base = atomicAdd(&fix_cnt[1], (uint32_t)__popcll(ml));
      base = __shfl(base, leader);
      if (is_long) fix_long[base + (uint32_t)__popcll(ml & ((1ull << lane) - 1ull))] = make_uint2(tF0, tF0 + span - 1);
    }
  }
  uint32_t bend = pos0;            // forces the run set-up on the first iteration
  bool first = true;
  // 78 KiB per 256-lane block, two blocks per CU: ZZ, ZZZ as 27 limbs, X as 24 packed words
  __shared__ uint32_t lds_zz[27 * ZK_LDS_STRIDE], lds_zzz[27 * ZK_LDS_STRIDE], lds_x[24 * ZK_LDS_STRIDE];
  uint32_t* zz = lds_zz + threadIdx.x;
  uint32_t* zzz = lds_zzz + threadIdx.x;
  uint32_t* xs = lds_x + threadIdx.x;
  XyzzRef acc = make_slot_ref(slots, stride, 0);
  bool inf = true;
  Fq ty = fp_zero<FqParams>();     // Y of the running accumulator, carried in registers across the additions of a run
  const bool dense = entries == nullptr;
  uint32_t e_next = dense ? pos0 : entries[pos0];
  // The SIMD's arbiter serves its OLDEST wave first: of the two waves that share a SIMD one runs at full speed and the other on
  // what is left, so a launch of a single machine fill ends with a third of its time at one wave per SIMD (78 % of the
  // multiplier's rate; measured: waves 0 .. 1023 of 2,000 end at 1.6 ms, the others at 2.55 ms).  The wave that is behind asks
  // for the higher priority, by quarters of its slice: both advance together and end together.
  // ... by quarters of its slice when it cannot see its partner; when it can - both waves of a SIMD belong to this launch and post
  // their iteration count in prio_board, one word per hardware wave slot (XCC, SE, SH, CU, SIMD, wave from HW_ID / XCC_ID), tagged
  // with the launch - the wave that has done fewer iterations gets the SIMD: the two stay within one iteration of each other.
  const uint32_t len4 = (pos1 - pos0) >> 2, q1 = pos0 + len4, q2 = q1 + len4, q3 = q2 + len4;
  uint32_t *board_mine = nullptr, *board_other = nullptr;
  if (prio_mode && prio_board) {
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 7u;
    const uint32_t simd = ((((xc * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u + ((hw >> 8) & 15u)) * 4u + ((hw >> 4) & 3u)) * 16u;
    board_mine = prio_board + simd + (hw & 15u);
    board_other = prio_board + simd + ((hw & 15u) ^ 1u);
  }
  uint32_t k = pos0, iter = 0;
  // one iteration's pacing: post this wave's progress, take the priority its partner's progress (or its own quarter) gives it
  auto pace = [&]() {
    if (!prio_mode) return;
    uint32_t other = 0;
    if (board_mine) {
      if ((threadIdx.x & 63u) == 0) __hip_atomic_store(board_mine, (prio_tag << 16) | (iter < 0xfffeu ? iter : 0xfffeu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      other = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(board_other, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    if (board_mine && (other >> 16) == prio_tag) {
      const uint32_t oi = other & 0xffffu;
      if (iter < oi) __builtin_amdgcn_s_setprio(3);
      else if (iter == oi) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    } else {
      const uint32_t kk = (uint32_t)__builtin_amdgcn_readfirstlane((int)k), a1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q1),
                     a2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q2), a3 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q3);
      if (kk < a1) __builtin_amdgcn_s_setprio(3);
      else if (kk < a2) __builtin_amdgcn_s_setprio(2);
      else if (kk < a3) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
    iter++;
  };
  if constexpr (EDW) {
    const EdwPacked* __restrict__ etab = reinterpret_cast<const EdwPacked*>(bp.p[0]);
    // inf: no run is open yet (an open run's slot is `acc`; LDS holds X, Z (zz), T (zzz), registers Y; it never returns to infinity)
    while (k < pos1) {
      pace();
      // run boundary: close the finished run, open the next one at the identity (memory operations only)
      if (k == bend) {
        if (!inf) {
          ZK_CLOSE_RUN(acc, xs, zz, zzz, ty);
          b++;
          while (offsets[b] + counts[b] <= k) b++;     // next non-empty bucket
        }
        bend = offsets[b] + counts[b];
        const bool starts = (k == offsets[b]), ends = (bend <= pos1);
        acc.voff = ((starts && ends) ? b : (!starts ? nb + t : nb + T + t)) * ZK_SLOT_PITCH;
        if constexpr (NJ > 1) etab = reinterpret_cast<const EdwPacked*>(base_of<NJ>(bp, b >> bshift));
        edw_set_identity(xs, zz, zzz, ty);
        inf = false;
      }
      // ---- one addition (bases at infinity never reach the entry list: k_digit_pass drops them)
      const uint32_t e = e_next;
      if (k + 1 < pos1) e_next = entries[k + 1];        // fetched a whole addition ahead of its use
      k++;
      edw_madd_lds_regy(xs, zz, zzz, ty, etab + (e & 0x7fffffffu), (e >> 31) != 0);
    }
  } else while (k < pos1) {
    pace();
    // ---- run boundaries and run openings: memory operations only.  The lanes that are in the middle of a run wait here for the few
    // that close one and open the next; whoever leaves this loop with k < pos1 has an addition to do.
    for (;;) {
      if (k == bend) {
        if (!first) {
          if (!inf) {   // close the finished run
            ZK_CLOSE_RUN(acc, xs, zz, zzz, ty);
          }
          b++;
          while (offsets[b] + counts[b] <= k) b++;     // next non-empty bucket
        }
        first = false;
        bend = offsets[b] + counts[b];
        const bool starts = (k == offsets[b]), ends = (bend <= pos1);
        const uint32_t slot = (starts && ends) ? b : (!starts ? nb + t : nb + T + t);
        acc.voff = slot * ZK_SLOT_PITCH;
        inf = true;
      }
      if (!inf) break;
      // open a run with entry k (also after a run cancelled to infinity in the middle of its bucket)
      const uint32_t e = e_next;
      if (k + 1 < pos1) e_next = dense ? k + 1 : entries[k + 1];
      const AffPacked* p = (dense ? bp.p[0] : base_of<NJ>(bp, b >> bshift)) + (e & 0x7fffffffu);
      k++;
      if (!(dense && p->x[23] == ZK_AFF_INF_WORD)) {               // (dense lists: a pair of the levels below may have cancelled)
#pragma unroll
        for (int i = 0; i < 24; i++) xs[i * ZK_LDS_STRIDE] = p->x[i];       // packed words straight into LDS
        ty = aff_ld_y(p, (e >> 31) != 0);
        lds_st(zz, fp_one<FqParams>());
        lds_st(zzz, fp_one<FqParams>());
        inf = false;
      }
      if (k >= pos1 || (k != bend && !inf)) break;
    }
    if (k >= pos1) break;
    // ---- one addition
    const uint32_t e = e_next;
    if (k + 1 < pos1) e_next = dense ? k + 1 : entries[k + 1];        // fetched a whole addition ahead of its use
    const AffPacked* p = (dense ? bp.p[0] : base_of<NJ>(bp, b >> bshift)) + (e & 0x7fffffffu);
    const bool neg = (e >> 31) != 0;        // (bases at infinity never reach the entry list: k_digit_pass drops them)
    k++;
    if (dense && p->x[23] == ZK_AFF_INF_WORD) continue;
    if (madd_lds_regy(acc, xs, zz, zzz, ty, p, neg)) inf = fp_is_zero_2p(lds_ld(zz));   // same-x path may have cancelled to infinity
  }
  if (board_mine && (threadIdx.x & 63u) == 0) __hip_atomic_store(board_mine, (prio_tag << 16) | 0xffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!inf) {
    ZK_CLOSE_RUN(acc, xs, zz, zzz, ty);
  }
  // a run that cancelled to infinity leaves ZZ = 0 in its slot: madd_same_x wrote the zeros, or the slot
  // was never written (zero-filled array)
  if (dbg_times && (threadIdx.x & 63u) == 0) {          // (wave-uniform: lane 0 of a wave that had work)
    const uint32_t wave = t >> 6;
    dbg_times[4 * wave] = dbg_t0; dbg_times[4 * wave + 1] = wall_clock64();
    dbg_times[4 * wave + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_ID: wave, SIMD, CU, SH, SE
    dbg_times[4 * wave + 3] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // XCC_ID
  }
}
template <int NJ>
__global__ void __launch_bounds__(256, 2) k_accumulate(ZK_ACC_PARAMS) {
  accumulate_impl<NJ, false>(bp, bshift, entries, offsets, counts, goff, nb, S_host, tight, T, slots, stride, fix_cnt, fix_short, fix_long,
                             dbg_times, prio_mode, prio_board, prio_tag);
}
// (fix_cnt[2] is the launch's lock_ok word, k_bucket_order below: 1 = k_accumulate_edw_lock has this launch, nothing to do here)
__global__ void __launch_bounds__(256, 2) k_accumulate_edw(ZK_ACC_PARAMS) {
  if (fix_cnt[2] == 1u) return;
  accumulate_impl<1, true>(bp, bshift, entries, offsets, counts, goff, nb, S_host, tight, T, slots, stride, fix_cnt, fix_short, fix_long,
                           dbg_times, prio_mode, prio_board, prio_tag);
}
// Merged Edwards launches (msm_launch_multi: up to four G1 jobs, a bucket window each) take the sliced route only - a proof's scalars
// are boolean-heavy and never pass the lockstep cap -, so nothing writes lock_ok there but the launch's memset: it reads 0.
__global__ void __launch_bounds__(256, 2) k_accumulate_edw_multi(ZK_ACC_PARAMS) {
  accumulate_impl<4, true>(bp, bshift, entries, offsets, counts, goff, nb, S_host, tight, T, slots, stride, fix_cnt, fix_short, fix_long,
                           dbg_times, prio_mode, prio_board, prio_tag);
}

// ---- the lockstep route of the Edwards accumulation: one bucket per lane -----------------------------------------------------
// With uniform scalars every bucket of a 2^20 launch holds 38 +- 6 entries.  Lanes that own whole BUCKETS of (nearly) equal
// population open and close their runs in the same iteration: no bucket is cut (nothing to stitch), the boundary block of the
// sliced kernel - paid by the whole wave whenever one lane is at a boundary - runs once per wave, and the loop carries an entry
// index and a count, nothing else.  What thread-per-bucket lost to the spread of populations (k_accumulate's comment) is taken out
// by ORDERING the buckets by population first: k_bucket_order is a counting sort of the bucket indices by count, descending, so
// the 64 buckets of a wave differ by a count or two and the waves are dispatched longest first.
// Whether a launch takes this route is decided ON THE DEVICE, per launch (the host never reads the word): lock_ok = 1 when no
// bucket holds more than ZK_LOCK_CAP entries (a boolean-heavy witness puts a third of its entries in one bucket: never here) and
// at least min_live buckets are non-empty (two waves for every SIMD).  Both routes are always enqueued; the one that is not
// taken returns on its first instruction.
// ZK_LOCK_CAP: at the headline's mean of 38 entries a bucket the largest of 2^19 binomial populations is about 70; 4 x 38 = 152,
// rounded to a power of two: 128.  A launch whose mean population is past ~90 (narrow windows over many terms) stays sliced.
#define ZK_LOCK_CAP 128u
#define ZK_LOCK_KEYS (ZK_LOCK_CAP + 2u)
// sort key of a bucket: 0 = over the cap (the order is not used then), CAP + 1 - count for counts 1 .. CAP, CAP + 1 = empty
__device__ __forceinline__ uint32_t lock_key(uint32_t cnt) { return cnt > ZK_LOCK_CAP ? 0u : ZK_LOCK_CAP + 1u - cnt; }
// PASS 0: ohist[key][block] = buckets of this block (1024 of them) with that key.  The host scans ohist (k_scan_*).
// PASS 1: order[] = the bucket indices by key (inside a key: any order - the counts are equal); block 0 writes lock_ok.
template <int PASS>
__global__ void __launch_bounds__(256) k_bucket_order(const uint32_t* __restrict__ counts, uint32_t nb, uint32_t* __restrict__ ohist,
                                                       uint32_t* __restrict__ order, uint32_t* __restrict__ lock_ok, uint32_t min_live, int enable) {
  __shared__ uint32_t s_k[ZK_LOCK_KEYS];
  const uint32_t tid = threadIdx.x, nblocks = gridDim.x;
  for (uint32_t j = tid; j < ZK_LOCK_KEYS; j += 256) s_k[j] = PASS == 0 ? 0u : ohist[(size_t)j * nblocks + blockIdx.x];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t b = blockIdx.x * 1024u + (uint32_t)k * 256u + tid;
    if (b < nb) {
      const uint32_t pos = atomicAdd(&s_k[lock_key(counts[b])], 1u);
      if (PASS == 1 && pos < nb) order[pos] = b;
    }
  }
  if (PASS == 0) {
    __syncthreads();
    for (uint32_t j = tid; j < ZK_LOCK_KEYS; j += 256) ohist[(size_t)j * nblocks + blockIdx.x] = s_k[j];
  } else if (blockIdx.x == 0 && tid == 0) {
    // (scanned ohist: [1][0] = the buckets over the cap, [CAP + 1][0] = the non-empty buckets)
    const uint32_t over = ohist[nblocks], live = ohist[(size_t)(ZK_LOCK_CAP + 1u) * nblocks];
    *lock_ok = (enable && over == 0u && live >= min_live) ? 1u : 0u;
  }
}

// Lane t owns bucket order[t].  The order is descending, so the wave's trip count is its first lane's count; a lane whose own
// count is reached sits out the remaining iterations (a count or two, at most).  Waves of empty buckets - the tail of the order -
// leave without touching a slot: the cleared Z words keep meaning "empty".  No pacing board here: the waves of a launch have
// different lengths and are dispatched longest first, a SIMD's two waves are never a pair that should end together.
__global__ void __launch_bounds__(256, 2) k_accumulate_edw_lock(const EdwPacked* __restrict__ etab, const uint32_t* __restrict__ entries,
                                                                 const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts,
                                                                 const uint32_t* __restrict__ order, uint32_t nb, uint32_t* __restrict__ slots,
                                                                 uint32_t stride, const uint32_t* __restrict__ lock_ok) {
  if (*lock_ok == 0u) return;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ uint32_t lds_zz[27 * ZK_LDS_STRIDE], lds_zzz[27 * ZK_LDS_STRIDE], lds_x[24 * ZK_LDS_STRIDE];
  uint32_t* zz = lds_zz + threadIdx.x;
  uint32_t* zzz = lds_zzz + threadIdx.x;
  uint32_t* xs = lds_x + threadIdx.x;
  const uint32_t b = t < nb ? order[t] : 0u;
  const uint32_t cnt = t < nb ? counts[b] : 0u;
  const uint32_t trip = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
  if (trip == 0u) return;
  const uint32_t off = offsets[b];
  // Entry j's table point is in T0, T1, T2 before iteration j starts (ec_edw.cuh edw_pre_issue): iteration j issues the gather of
  // entry j + 1 and the load of entry j + 2's index under its last product, so the loop carries the entry it works on, the two
  // behind it and the three temporaries that hold the point.  Every index load is guarded by the lane's own count - the last
  // bucket ends where the entry array ends - and a lane that sits out loads nothing.
  Fq ty, T0, T1, T2;           // (not initialised: written before they are read)
  uint32_t e = cnt ? entries[off] : 0u;
  uint32_t e1 = cnt > 1u ? entries[off + 1u] : 0u, e2 = cnt > 2u ? entries[off + 2u] : 0u;
  // iteration 0 (wave-uniform): the bucket opens FROM its first table point, one product; a bucket of one entry closes from here
  if (cnt) {
    edw_pre_issue(T0, T1, T2, etab, e);                                             // (the one exposed gather of a wave)
    edw_open_lds_pre(xs, zz, zzz, ty, T0, T1, T2, (e >> 31) != 0, etab, e1, cnt > 1u);
  }
  for (uint32_t j = 1; j < trip; j++) {
    if (j < cnt) {
      e = e1; e1 = e2;
      edw_madd_lds_pre(xs, zz, zzz, ty, T0, T1, T2, (e >> 31) != 0, etab, e1, j + 1 < cnt, e2, entries, off + j + 2, j + 2 < cnt);
    }
  }
  if (cnt) {
    XyzzRef acc = make_slot_ref(slots, stride, b);
    ZK_CLOSE_RUN(acc, xs, zz, zzz, ty);
  }
}

// chi for every entry of a window table (levels x n points): the precomputed Edwards table.  Entries at infinity hold zeros; *bad
// counts the points that are not on G1's curve or have even order (the base set then stays on the XYZZ path).
__global__ void __launch_bounds__(256) k_table_edw(const AffPacked* __restrict__ tab, const uint8_t* __restrict__ tinf, EdwPacked* __restrict__ out,
                                                   size_t total, uint32_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (tinf[i]) {
    uint32_t* w = reinterpret_cast<uint32_t*>(out + i);
#pragma unroll
    for (int k = 0; k < 72; k++) w[k] = 0u;
    return;
  }
  const AffPacked* p = tab + i;
  if (!edw_from_affine(aff_ld_x(p), aff_ld_y(p, false), out + i)) atomicAdd(bad, 1u);
}

// ---- batched-affine levels ------------------------------------------------------------------------------------------------
// The bucket-sorted entry list is summed PAIRWISE inside every bucket, level by level: a bucket of n points becomes ceil(n/2)
// points (floor(n/2) sums and, for odd n, its last point passed through), written densely in bucket order.  All additions of a
// level are independent, so a lane that produces m consecutive outputs shares one field inversion among them (ec_affine.cuh):
//   forward   d_j = x2 - x1 of pair j;  scratch[j] = d_0 ... d_(j-1);  acc = d_0 ... d_(m-1)
//   inv = 1 / acc                                       (fp_inv: division steps, all 64 lanes at once)
//   backward  1/d_j = inv * scratch[j];  inv *= d_j;  lambda, x3, y3;  store
// 5 M + 1 S per addition (+ ~30 M / m for the inversion) instead of the 8 M + 2 S of a mixed addition into an XYZZ accumulator.
// After a few levels (the buckets are down to a handful of points) k_accumulate sums what is left, in its dense mode.
__global__ void __launch_bounds__(256) k_half_counts(const uint32_t* __restrict__ in_cnt, uint32_t* __restrict__ out_cnt, size_t nb) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) out_cnt[i] = (in_cnt[i] + 1) >> 1;
}

struct LevelArgs {
  BasePtrs bp;                 // first level: the base tables, by job
  int bshift;
  const uint32_t* entries;     // first level: bucket-sorted (index | sign << 31)
  const AffPacked* src;        // later levels: the previous level's dense points
  const uint32_t* in_off;      // [nb] start of every bucket in the input level
  const uint32_t* in_cnt;      // [nb]
  const uint32_t* out_off;     // [nb] start of every bucket in the output level (counts: ceil(in_cnt / 2))
  uint32_t nb, m, lane0, lanes;  // outputs per lane; first lane of this launch; lanes of this launch (row length of `scratch`)
  AffPacked* dst;
  uint32_t* scratch;           // prefix products, limb-major: word (j * 27 + k) of lane t at scratch[(j * 27 + k) * lanes + t]
};

struct LevelWalk {             // the bucket that holds output j, and where its inputs start
  uint32_t b, ooff, oend, ioff, icnt;
};
__device__ __forceinline__ void walk_fwd(LevelWalk& w, uint32_t j, const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ in_cnt) {
  while (j >= w.oend) {
    w.b++;
    const uint32_t c = in_cnt[w.b];
    if (!c) continue;
    w.ooff = w.oend; w.icnt = c; w.ioff = in_off[w.b]; w.oend = w.ooff + ((c + 1) >> 1);
  }
}
__device__ __forceinline__ void walk_bwd(LevelWalk& w, uint32_t j, const uint32_t* __restrict__ in_off, const uint32_t* __restrict__ in_cnt) {
  while (j < w.ooff) {
    w.b--;
    const uint32_t c = in_cnt[w.b];
    if (!c) continue;
    w.oend = w.ooff; w.icnt = c; w.ioff = in_off[w.b]; w.ooff = w.oend - ((c + 1) >> 1);
  }
}
template <int NJ, bool FIRST>
__device__ __forceinline__ PairRef level_pair(const LevelArgs& a, const LevelWalk& w, uint32_t j) {
  const uint32_t i = j - w.ooff, p0 = w.ioff + 2 * i;
  const bool has2 = 2 * i + 1 < w.icnt;
  PairRef pr;
  if constexpr (FIRST) {
    const AffPacked* base = base_of<NJ>(a.bp, w.b >> a.bshift);
    const uint32_t e0 = a.entries[p0], e1 = has2 ? a.entries[p0 + 1] : 0u;
    pr.p1 = base + (e0 & 0x7fffffffu); pr.neg1 = (e0 >> 31) != 0;
    pr.p2 = has2 ? base + (e1 & 0x7fffffffu) : nullptr; pr.neg2 = (e1 >> 31) != 0;
  } else {
    pr.p1 = a.src + p0; pr.neg1 = false;
    pr.p2 = has2 ? a.src + p0 + 1 : nullptr; pr.neg2 = false;
  }
  return pr;
}
__device__ __forceinline__ void pair_ld_x(const PairRef& pr, uint32_t* wx1, uint32_t* wx2) {
  aff_ld_words(pr.p1->x, wx1);
  if (pr.p2) aff_ld_words(pr.p2->x, wx2);
}

template <int NJ, bool FIRST>
__global__ void __launch_bounds__(256, 2) k_affine_level(LevelArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t M_out = a.out_off[a.nb - 1] + ((a.in_cnt[a.nb - 1] + 1) >> 1);
  const uint64_t j0_64 = (uint64_t)(a.lane0 + t) * a.m;
  if (t >= a.lanes || j0_64 >= M_out) return;
  const uint32_t j0 = (uint32_t)j0_64, cnt = min(a.m, M_out - j0);
  const zk_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.scratch, 0, (int)((size_t)a.m * 27u * a.lanes * 4u), 0x00020000);
  const uint32_t voff = t * 4u, row_b = a.lanes * 4u;
  LevelWalk w;
  w.b = bucket_of(a.out_off, a.nb, j0);
  w.icnt = a.in_cnt[w.b]; w.ioff = a.in_off[w.b]; w.ooff = a.out_off[w.b]; w.oend = w.ooff + ((w.icnt + 1) >> 1);
  // Memory: every operand is fetched ONE multiplication ahead of its use (a gather from a multi-gigabyte table costs about as
  // much as a sixth of a multiplication, and with two waves per SIMD a stalled wave is half the SIMD's throughput lost): the
  // words wait in 48 registers (`pw`) carried around the loops, and the pair of the next output is located while the current
  // one computes.
  // ---- forward: prefix products of the slope denominators
  Fq acc = fp_one<FqParams>();
  {
    uint32_t pw[48];
    walk_fwd(w, j0, a.in_off, a.in_cnt);
    PairRef pr = level_pair<NJ, FIRST>(a, w, j0);
    pair_ld_x(pr, pw, pw + 24);
#pragma unroll 1
    for (uint32_t jj = 0; jj < cnt; jj++) {
      const uint32_t kind = pair_kind(pr, pw, pw + 24);
      const Fq d = pair_denominator(pr, kind, pw, pw + 24);
      if (jj + 1 < cnt) {                                            // the next pair's x coordinates travel under this multiplication
        walk_fwd(w, j0 + jj + 1, a.in_off, a.in_cnt);
        pr = level_pair<NJ, FIRST>(a, w, j0 + jj + 1);
        pair_ld_x(pr, pw, pw + 24);
      }
#pragma unroll
      for (int k = 0; k < 27; k++) __builtin_amdgcn_raw_buffer_store_b32(acc.l[k], rs, voff, (jj * 27u + (uint32_t)k) * row_b, 0);
      acc = fp_mul(acc, d);
    }
  }
  Fq inv = fp_inv<FqParams>(acc);
  // ---- backward: one addition per output.  A rolled micro-program (one multiplier body and one squaring body in the loop, as
  // in ec_mem.cuh); three field elements are carried from step to step: inv, T0 (1/d, then x3), T1 (3 x1^2, then lambda).
  PairRef pr = level_pair<NJ, FIRST>(a, w, j0 + cnt - 1);           // (the forward pass left w on the last output)
#pragma unroll 1
  for (uint32_t jj = a.m; jj-- > 0;) {               // (a wave-uniform counter: it is the scalar row offset of the scratch loads)
    if (jj >= cnt) continue;
    const uint32_t j = j0 + jj;
    PairRef pr_next = pr;
    uint32_t kind = PK_FIRST;
    bool any_dbl = false;
    Fq T0 = fp_zero<FqParams>(), T1 = T0;
    uint32_t pw[48];
#pragma unroll
    for (int k = 0; k < 48; k++) pw[k] = 0;
#pragma unroll 1
    for (int step = 0; step < 6; step++) {
      if (step == 2 && !any_dbl) continue;
      Fq A, B;
      switch (step) {
        case 0:                                                     // 1/d = inv * (d_0 ... d_(j-1))
          A = inv;
#pragma unroll
          for (int k = 0; k < 27; k++) B.l[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, (jj * 27u + (uint32_t)k) * row_b, 0);
          pair_ld_x(pr, pw, pw + 24);                               // for step 1
          break;
        case 1: {                                                   // inv <- inv * d
          kind = pair_kind(pr, pw, pw + 24);
          A = inv; B = pair_denominator(pr, kind, pw, pw + 24);
          aff_ld_words(pr.p1->y, pw);                               // for step 3
          if (pr.p2) aff_ld_words(pr.p2->y, pw + 24);
          break;
        }
        case 2: { uint32_t wx1[24]; aff_ld_words(pr.p1->x, wx1); A = fp_unpack32<FqParams>(wx1); B = A; break; }   // x1^2 (doublings)
        case 3: {                                                   // lambda = numerator / d
          if (kind == PK_ADD) A = fp_sub<FqParams, 2>(aff_y_eff(pw + 24, pr.neg2), aff_y_eff(pw, pr.neg1));      // [4]
          else A = T1;                                              // 3 x1^2 [6] (or unused)
          B = T0;
          pair_ld_x(pr, pw, pw + 24);                               // for the end of step 4
          break;
        }
        case 4: A = T1; B = T1; break;                              // lambda^2
        default: {                                                  // lambda (x1 - x3)
          A = T1; B = fp_sub<FqParams, 2>(fp_unpack32<FqParams>(pw), T0);                   // [3]
          if (jj > 0) {                                             // locate the pair of the next output under this multiplication
            walk_bwd(w, j - 1, a.in_off, a.in_cnt);
            pr_next = level_pair<NJ, FIRST>(a, w, j - 1);
          }
          break;
        }
      }
      const Fq r = (step == 2 || step == 4) ? fp_sqr(A) : fp_mul(A, B);
      switch (step) {
        case 0: T0 = r; break;
        case 1: inv = r; any_dbl = __any(kind == PK_DBL); break;
        case 2: T1 = fp_add(fp_dbl(r), r); break;                   // [6]
        case 3: T1 = r; break;
        case 4: {                                                   // x3 = lambda^2 - x1 - x2  (stored at once; kept in T0 for y3)
          Fq x1 = fp_unpack32<FqParams>(pw), x2 = x1;
          if (kind == PK_ADD) x2 = fp_unpack32<FqParams>(pw + 24);
          T0 = fp_canon_4p(fp_sub<FqParams, 2>(r, fp_add(x1, x2)));
          uint32_t ox[24];
          fp_pack32<FqParams>(T0, ox);
          aff_st_words(a.dst[j].x, ox);
          aff_ld_words(pr.p1->y, pw + 24);                          // y1 for the end of step 5 (x1 stays in pw[0 .. 24))
          break;
        }
        default: {                                                  // y3 = lambda (x1 - x3) - y1
          uint32_t oy[24];
          fp_pack32<FqParams>(fp_canon_4p(fp_sub<FqParams, 2>(r, aff_y_eff(pw + 24, pr.neg1))), oy);
          aff_st_words(a.dst[j].y, oy);
          break;
        }
      }
    }
    if (kind > PK_DBL) {                                            // no sum: overwrite what the program above stored for this output
      uint32_t ox[24], oy[24];
      if (kind == PK_INF) {
#pragma unroll
        for (int k = 0; k < 24; k++) { ox[k] = ZK_AFF_INF_WORD; oy[k] = 0; }
      } else {                                                      // the pair's finite point passes through (sign applied)
        const AffPacked* q = (kind == PK_FIRST) ? pr.p1 : pr.p2;
        const bool neg = (kind == PK_FIRST) ? pr.neg1 : pr.neg2;
        aff_ld_words(q->x, ox); aff_ld_words(q->y, oy);
        if (neg) fp_pack32<FqParams>(fp_canon_4p(aff_y_eff(oy, true)), oy);
      }
      aff_st_words(a.dst[j].x, ox); aff_st_words(a.dst[j].y, oy);
    }
    pr = pr_next;
  }
}

// Point operations on memory accumulators executed by one lane (QUAD = false: throughput-bound
// launches with at least as many additions as lanes) or by a DPP quad (QUAD = true: latency-bound
// launches; see ec_mem.cuh).  In quad mode all four lanes of a quad receive the same references.
// per-lane LDS scratch of the one-lane additions (add_mem_s): two 27-word limb-major images per 256-lane block
struct AddScratch { uint32_t* zz; uint32_t* zzz; };
#define ADD_SCRATCH_DECL(QUADFLAG)                                                                   \
  __shared__ uint32_t s_add_zz_[(QUADFLAG) ? 1 : 27 * ZK_LDS_STRIDE], s_add_zzz_[(QUADFLAG) ? 1 : 27 * ZK_LDS_STRIDE]; \
  const AddScratch sc{s_add_zz_ + ((QUADFLAG) ? 0 : threadIdx.x), s_add_zzz_ + ((QUADFLAG) ? 0 : threadIdx.x)}
// EDW: the point model of the launch.  false: XYZZ points of G1; true: extended points of the 2-isogenous Edwards curve in the same
// four words (ec_edw.cuh) - what k_accumulate_edw leaves in the slots.  Copies, "nothing here" (all-zero ZZ / Z words) and the
// array layouts are the same in both models; only the additions and doublings differ.  Every kernel below exists once per model:
// k_name (XYZZ) and k_name_edw share one body.
template <bool QUAD, bool EDW = false> __device__ __forceinline__ void pt_add(const XyzzRef& a, const XyzzRef& b, uint32_t q, const AddScratch& sc) {
  if constexpr (EDW) { if constexpr (QUAD) edw_add_mem_quad(a, b, q); else edw_add_mem(a, b); }
  else if constexpr (QUAD) add_mem_quad(a, b, q); else add_mem_s(a, b, sc.zz, sc.zzz);
}
template <bool EDW> __device__ __forceinline__ void pt_dbl_quad(const XyzzRef& a, uint32_t q) {
  if constexpr (EDW) edw_dbl_mem_quad(a, q); else dbl_mem_quad(a, q);
}
// full addition into an accumulator on the CU (X packed, ZZ / Z, ZZZ / T in LDS, Y in registers); true: the sum is XYZZ's infinity
template <bool EDW> __device__ __forceinline__ bool pt_add_lds(const XyzzRef& spill, uint32_t* xs, uint32_t* zz, uint32_t* zzz, Fq& ty, const XyzzRef& B) {
  if constexpr (EDW) { edw_add_lds_regy(xs, zz, zzz, ty, B); return false; }
  else return add_lds_regy(spill, xs, zz, zzz, ty, B) && fp_is_zero_2p(lds_ld(zz));     // same-x path may have cancelled to infinity
}
template <bool QUAD> __device__ __forceinline__ void pt_copy(const XyzzRef& dst, const XyzzRef& src, uint32_t q) {
  if constexpr (QUAD) mem_st_lane(dst, q, mem_ld_lane(src, q)); else mem_copy(dst, src);
}
template <bool QUAD> __device__ __forceinline__ void pt_set_inf(const XyzzRef& dst, uint32_t q) {
  if constexpr (QUAD) mem_st_lane(dst, q, fp_zero<FqParams>()); else mem_set_inf(dst);
}

// Stitch buckets that were cut by slice boundaries.  A bucket that starts in slice t0 and ends in slice t1 > t0 has pieces L[t0],
// F[t0+1], ..., F[t1].  First the F pieces are folded into F[t0+1] (k_fixup_fold, ONE launch, two kinds of workgroup):
//   * buckets of 2 .. 4 F pieces (the short list k_accumulate made): one lane - or one quad, in a latency-bound launch - folds them,
//     densely over the list.  With uniform scalars a few percent of the buckets have two F pieces, none more: one launch over
//     every slice, as rounds 1-2 had it, kept every wave busy for the sake of one lane in twelve.
//   * buckets of more pieces (the long list: "scalar == 1" in a boolean-heavy witness holds a third of all entries): a workgroup
//     each, its 64 quads fold the pieces pairwise (F[t] += F[t+d] for t - first divisible by 2d) in log2(pieces) rounds d = 1, 2,
//     4, ..., a barrier between rounds (the pieces live in global memory, coherent inside a CU).
// Both kinds touch different buckets, so they run side by side: a proof on its own waits for the longer of the two, not their sum.
#define ZK_FOLD_PARAMS                                                                                                             \
  const uint32_t* __restrict__ cnt /* [2]: short, long */, const uint2* __restrict__ list_short, const uint2* __restrict__ list_long, \
      uint32_t short_blocks, uint32_t nb, uint32_t* __restrict__ slots, uint32_t stride
template <bool QUAD, bool EDW>
__device__ __forceinline__ void fixup_fold_impl(ZK_FOLD_PARAMS) {
  ADD_SCRATCH_DECL(QUAD || EDW);
  const uint32_t q = threadIdx.x & 3u;
  if (blockIdx.x < short_blocks) {
    const uint32_t n = cnt[0], per = QUAD ? 64u : 256u;
    for (uint32_t i = blockIdx.x * per + (QUAD ? threadIdx.x >> 2 : threadIdx.x); i < n; i += short_blocks * per) {
      const uint2 w = list_short[i];                    // first F slot, number of F pieces
      const XyzzRef dst = make_slot_ref(slots, stride, nb + w.x);
      for (uint32_t j = 1; j < w.y; j++) pt_add<QUAD, EDW>(dst, make_slot_ref(slots, stride, nb + w.x + j), q, sc);
    }
    return;
  }
  const uint32_t n = cnt[1], quad = threadIdx.x >> 2;
  for (uint32_t i = blockIdx.x - short_blocks; i < n; i += gridDim.x - short_blocks) {
    const uint2 w = list_long[i];                       // first and last F piece of the bucket
#pragma unroll 1
    for (uint32_t d = 1; d <= w.y - w.x; d <<= 1) {
      for (uint64_t t = (uint64_t)w.x + (uint64_t)quad * 2 * d; t + d <= w.y; t += (uint64_t)64 * 2 * d)
        pt_add<true, EDW>(make_slot_ref(slots, stride, nb + (uint32_t)t), make_slot_ref(slots, stride, nb + (uint32_t)t + d), q, sc);
      __threadfence_block();
      __syncthreads();
    }
  }
}
template <bool QUAD> __global__ void __launch_bounds__(256, 2) k_fixup_fold(ZK_FOLD_PARAMS) {
  fixup_fold_impl<QUAD, false>(cnt, list_short, list_long, short_blocks, nb, slots, stride);
}
template <bool QUAD> __global__ void __launch_bounds__(256, 2) k_fixup_fold_edw(ZK_FOLD_PARAMS) {
  if (cnt[2] == 1u) return;         // (lock_ok: the lockstep route cut no bucket)
  fixup_fold_impl<QUAD, true>(cnt, list_short, list_long, short_blocks, nb, slots, stride);
}

// final stitch: the slice in which a cut bucket STARTS owns it: bucket = L[t0] + F[t0+1] (folded).
#define ZK_FIXUP_PARAMS                                                                                                             \
  const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ goff, uint32_t nb, uint32_t S_host, \
      int tight, uint32_t T, uint32_t* __restrict__ slots, uint32_t stride, uint32_t wf
template <bool EDW>
__device__ __forceinline__ void fixup_impl(ZK_FIXUP_PARAMS) {
  // the L piece goes to the CU (X, ZZ, ZZZ in LDS, Y in registers, as in k_accumulate / k_sum_lds), the F piece is added to it
  // there and the sum is stored once: ten coordinate loads and four stores per cut bucket (a copy into the bucket's slot followed by
  // an addition in memory - rounds 1-3 - moved fourteen and eight)
  __shared__ uint32_t lds_zz[27 * ZK_LDS_STRIDE], lds_zzz[27 * ZK_LDS_STRIDE], lds_x[24 * ZK_LDS_STRIDE];
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;   // throughput-bound (one addition per slice): one lane each
  const uint32_t M = offsets[nb - 1] + counts[nb - 1];
  const uint32_t A = slice_weight(goff[nb], T, S_host, tight);
  if (t >= T) return;
  uint32_t b0_, b1_;
  const uint32_t pos0 = slice_pos(goff, offsets, counts, nb, M, (uint64_t)t * A, &b0_, wf);
  if (pos0 >= M) return;
  const uint32_t pos1 = slice_pos(goff, offsets, counts, nb, M, (uint64_t)(t + 1) * A, &b1_, wf);
  uint32_t b = bucket_of(offsets, nb, pos1 - 1);
  uint32_t bend = offsets[b] + counts[b];
  if (bend <= pos1 || offsets[b] < pos0) return;      // not cut at this slice's end, or started earlier
  const XyzzRef dst = make_slot_ref(slots, stride, b), pl = make_slot_ref(slots, stride, nb + T + t), pf = make_slot_ref(slots, stride, nb + t + 1);
  const bool l_inf = mem_is_inf(pl), f_inf = mem_is_inf(pf);
  if (l_inf || f_inf) {                                 // (a piece whose points cancelled: rare)
    if (l_inf && f_inf) mem_set_inf(dst);
    else mem_copy(dst, l_inf ? pf : pl);
    return;
  }
  uint32_t* zz = lds_zz + threadIdx.x;
  uint32_t* zzz = lds_zzz + threadIdx.x;
  uint32_t* xs = lds_x + threadIdx.x;
  lds_st_packed(xs, mem_ld(pl, CX));                    // X of a stored point is an X3 [10]: below 2^768, packs into 24 words
  Fq ty = mem_ld(pl, CY);
  lds_st(zz, mem_ld(pl, CZZ));
  lds_st(zzz, mem_ld(pl, CZZZ));
  if (pt_add_lds<EDW>(dst, xs, zz, zzz, ty, pf)) { mem_set_inf(dst); return; }   // same-x path: L = -F
  mem_st(dst, CX, lds_ld_packed(xs)); mem_st(dst, CY, ty); mem_st(dst, CZZ, lds_ld(zz)); mem_st(dst, CZZZ, lds_ld(zzz));
}
__global__ void __launch_bounds__(256, 2) k_fixup(ZK_FIXUP_PARAMS) { fixup_impl<false>(offsets, counts, goff, nb, S_host, tight, T, slots, stride, wf); }
__global__ void __launch_bounds__(256, 2) k_fixup_edw(ZK_FIXUP_PARAMS, const uint32_t* __restrict__ lock_ok) {
  if (*lock_ok == 1u) return;       // (the lockstep route cut no bucket)
  fixup_impl<true>(offsets, counts, goff, nb, S_host, tight, T, slots, stride, wf);
}

// out[t] = sum_u in[i(t) + u * row_len],  i(t) = (t / row_len) * (L * row_len) + (t % row_len).
// row_len = 1: sums of L consecutive items (row sums);  row_len = R: for items laid out [g][h][R] it sums L
// consecutive h for every (g, h / L, lo) (column sums).  in: n_in items with row stride in_stride words.
#define ZK_SUM_PARAMS                                                                                       \
  uint32_t* __restrict__ in, size_t n_in, uint32_t in_stride, int L, uint32_t row_len, uint32_t* __restrict__ out, \
      int in_slots /* `in` is the slot array (ec_mem.cuh) */
template <bool QUAD, bool EDW>
__device__ __forceinline__ void sum_impl(ZK_SUM_PARAMS) {
  ADD_SCRATCH_DECL(QUAD || EDW);
  size_t n_out = n_in / L;
  size_t gt = (size_t)blockIdx.x * blockDim.x + threadIdx.x, t = QUAD ? gt >> 2 : gt;    // one lane / quad per output
  const uint32_t q = (uint32_t)(gt & 3);
  if (t >= n_out) return;
  const size_t i0 = (t / row_len) * ((size_t)L * row_len) + (t % row_len);
  XyzzRef acc = make_ref(out, (uint32_t)n_out, (uint32_t)t);
  pt_copy<QUAD>(acc, make_in_ref(in, in_stride, (uint32_t)i0, in_slots), q);
  for (int u = 1; u < L; u++) pt_add<QUAD, EDW>(acc, make_in_ref(in, in_stride, (uint32_t)(i0 + (size_t)u * row_len), in_slots), q, sc);
}
template <bool QUAD> __global__ void __launch_bounds__(256, 2) k_sum(ZK_SUM_PARAMS) { sum_impl<QUAD, false>(in, n_in, in_stride, L, row_len, out, in_slots); }
template <bool QUAD> __global__ void __launch_bounds__(256, 2) k_sum_edw(ZK_SUM_PARAMS) { sum_impl<QUAD, true>(in, n_in, in_stride, L, row_len, out, in_slots); }

// k_sum with one lane per output and the running sum held on the CU (add_lds_regy): the throughput-bound plain sums of the bucket
// reduction.  Same indexing as k_sum.
template <bool EDW>
__device__ __forceinline__ void sum_lds_impl(ZK_SUM_PARAMS) {
  __shared__ uint32_t lds_zz[27 * ZK_LDS_STRIDE], lds_zzz[27 * ZK_LDS_STRIDE], lds_x[24 * ZK_LDS_STRIDE];
  const size_t n_out = n_in / L;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_out) return;
  uint32_t* zz = lds_zz + threadIdx.x;
  uint32_t* zzz = lds_zzz + threadIdx.x;
  uint32_t* xs = lds_x + threadIdx.x;
  const size_t i0 = (t / row_len) * ((size_t)L * row_len) + (t % row_len);
  const XyzzRef dst = make_ref(out, (uint32_t)n_out, (uint32_t)t);
  bool inf = true;
  Fq ty = fp_zero<FqParams>();
  for (int u = 0; u < L; u++) {
    const XyzzRef B = make_in_ref(in, in_stride, (uint32_t)(i0 + (size_t)u * row_len), in_slots);
    if (mem_is_inf(B)) continue;
    if (inf) {
      lds_st_packed(xs, mem_ld(B, CX));             // X of a stored point is an X3 [10]: below 2^768, packs into 24 words
      ty = mem_ld(B, CY);
      lds_st(zz, mem_ld(B, CZZ));
      lds_st(zzz, mem_ld(B, CZZZ));
      inf = false;
      continue;
    }
    inf = pt_add_lds<EDW>(dst, xs, zz, zzz, ty, B);
  }
  if (inf) { mem_set_inf(dst); return; }
  mem_st(dst, CX, lds_ld_packed(xs)); mem_st(dst, CY, ty); mem_st(dst, CZZ, lds_ld(zz)); mem_st(dst, CZZZ, lds_ld(zzz));
}
__global__ void __launch_bounds__(256, 2) k_sum_lds(ZK_SUM_PARAMS) { sum_lds_impl<false>(in, n_in, in_stride, L, row_len, out, in_slots); }
__global__ void __launch_bounds__(256, 2) k_sum_lds_edw(ZK_SUM_PARAMS) { sum_lds_impl<true>(in, n_in, in_stride, L, row_len, out, in_slots); }

// Two-level split of the bucket index j = hi * R + lo (R = 2^lo_bits, H = 2^hi_bits rows):
//   sum_j (j+1) B_j = R * sum_hi hi * Row[hi] + sum_lo (lo+1) * Col[lo].
// k_place_hilo lays both small weighted sums out as 2W groups of N = max(R, H) items with weights index+1:
//   group w      : item i = Row[w][i+1]  (i < H-1), infinity beyond      (weight i+1 = hi)
//   group W + w  : item i = Col[w][i]    (i < R),   infinity beyond      (weight i+1 = lo+1)
__global__ void __launch_bounds__(256, 2) k_place_hilo(uint32_t* __restrict__ rows /* W*H */, uint32_t* __restrict__ cols /* W*R */,
                                                        uint32_t W, uint32_t H, uint32_t R, uint32_t N, uint32_t* __restrict__ out /* 2W*N */) {
  uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, t = gt >> 2, q = gt & 3u;
  if (t >= 2 * W * N) return;
  uint32_t g = t / N, i = t % N;
  XyzzRef dst = make_ref(out, 2 * W * N, t);
  if (g < W) {
    if (i + 1 < H) mem_st_lane(dst, q, mem_ld_lane(make_ref(rows, W * H, g * H + i + 1), q));
    else mem_st_lane(dst, q, fp_zero<FqParams>());
  } else {
    if (i < R) mem_st_lane(dst, q, mem_ld_lane(make_ref(cols, W * R, (g - W) * R + i), q));
    else mem_st_lane(dst, q, fp_zero<FqParams>());
  }
}

// The two small weighted sums by bit planes (msm_plan.hpp): F_g = sum_i (i+1) item_{g,i} = sum_j 2^j P_{g,j}, where plane j of group
// g sums the items whose weight i+1 has bit j set.  k_plane_sum is one level of the planes' trees, a quad per output:
//   out[p][r] = sum_{u < L} in[p'][r L + u],  r < per_plane / L
// The FIRST level (select != 0) reads the one item array for every plane (p' = 0; item i of a group has weight i % left + 1) and takes
// the items whose weight has bit p set - every item for plane total_plane (a NAF plan's plain total; -1: none).  The later levels
// are ordinary sums inside each plane (p' = p).  Ordering between the levels comes from the stream alone.
#define ZK_PLANE_PARAMS                                                                                                  \
  uint32_t* __restrict__ in, uint32_t in_stride, uint32_t per_plane /* G groups x `left` items */, uint32_t left, int L, \
      int planes, int select, int total_plane, uint32_t* __restrict__ out
template <bool EDW>
__device__ __forceinline__ void plane_sum_impl(ZK_PLANE_PARAMS) {
  const uint32_t per_out = per_plane / (uint32_t)L, n_out = (uint32_t)planes * per_out;
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, t = gt >> 2, q = gt & 3u;
  if (t >= n_out) return;
  const uint32_t p = t / per_out, r = t % per_out;
  const XyzzRef acc = make_ref(out, n_out, t);
  bool first = true;
  for (int u = 0; u < L; u++) {
    const uint32_t i = r * (uint32_t)L + (uint32_t)u;
    if (select && (int)p != total_plane && !(((i % left) + 1u) >> p & 1u)) continue;
    const XyzzRef it = make_ref(in, in_stride, select ? i : p * per_plane + i);
    if (mem_is_inf(it)) continue;      // (an empty slot has only its ZZ / Z words cleared: it must not reach the output by a copy)
    if (first) pt_copy<true>(acc, it, q);
    else pt_add<true, EDW>(acc, it, q, AddScratch{nullptr, nullptr});
    first = false;
  }
  if (first) pt_set_inf<true>(acc, q);
}
__global__ void __launch_bounds__(256, 2) k_plane_sum(ZK_PLANE_PARAMS) { plane_sum_impl<false>(in, in_stride, per_plane, left, L, planes, select, total_plane, out); }
__global__ void __launch_bounds__(256, 2) k_plane_sum_edw(ZK_PLANE_PARAMS) { plane_sum_impl<true>(in, in_stride, per_plane, left, L, planes, select, total_plane, out); }

// The planes of one bucket window recombined, one workgroup per window w: `sums` holds one point per (plane, group), point
// p * 2W + g.  Quad s < 2 wp takes weight plane j = s % wp of the hi group (s < wp: group w) or of the lo group (group W + w)
// and doubles it j times, the hi group's lo_bits times more (the window's sum is R * hi + lo, R = 2^lo_bits): side by side, not
// one Horner chain.  Then the 2 wp points are summed pairwise in place, a barrier between the rounds (the points live in global
// memory, coherent inside a CU, as in k_fixup_fold), and quad 0 writes the ABI limbs.  has_total: plane wp of the lo group is
// sum_b S_b of the window and goes out behind the W weighted sums (the NAF finish needs it).
// (an Edwards launch leaves (X : Y : Z : T) per window in out_abi: the host applies psi, edw_abi_to_jac)
#define ZK_PCOMB_PARAMS \
  uint32_t* __restrict__ sums, int W, int wp /* weight planes, 2 wp <= 64 */, int has_total, int lo_bits, uint64_t* __restrict__ out_abi
template <bool EDW>
__device__ __forceinline__ void plane_combine_impl(ZK_PCOMB_PARAMS) {
  const uint32_t w = blockIdx.x, s = threadIdx.x >> 2, q = threadIdx.x & 3u, n = 2u * (uint32_t)wp;
  const uint32_t stride = (uint32_t)((wp + has_total) * 2 * W);
  auto ref = [&](uint32_t k) { return make_ref(sums, stride, (k % (uint32_t)wp) * 2u * (uint32_t)W + (k < (uint32_t)wp ? w : (uint32_t)W + w)); };
  if (s < n) {
    const XyzzRef a = ref(s);
    const int dbl = (int)(s % (uint32_t)wp) + (s < (uint32_t)wp ? lo_bits : 0);
    for (int d = 0; d < dbl; d++) pt_dbl_quad<EDW>(a, q);
  }
#pragma unroll 1
  for (uint32_t d = 1; d < n; d <<= 1) {
    __threadfence_block();
    __syncthreads();
    if (s % (2 * d) == 0 && s + d < n) pt_add<true, EDW>(ref(s), ref(s + d), q, AddScratch{nullptr, nullptr});
  }
  if (s != 0) return;
  fp_to_abi<FqParams>(mem_ld_lane(ref(0), q), out_abi + (size_t)w * 48 + 12 * q);            // lane q converts coordinate q
  if (has_total) fp_to_abi<FqParams>(mem_ld_lane(make_ref(sums, stride, (uint32_t)(wp * 2 * W + W) + w), q), out_abi + (size_t)(W + w) * 48 + 12 * q);
}
__global__ void __launch_bounds__(256, 2) k_plane_combine(ZK_PCOMB_PARAMS) { plane_combine_impl<false>(sums, W, wp, has_total, lo_bits, out_abi); }
__global__ void __launch_bounds__(256, 2) k_plane_combine_edw(ZK_PCOMB_PARAMS) { plane_combine_impl<true>(sums, W, wp, has_total, lo_bits, out_abi); }

// Test hook (msm_tail_selftest): n affine points in ABI form (all-zero = infinity) -> points of the reduction's arrays (limb-major,
// stride n), XYZZ (x, y, 1, 1) or, edw != 0, chi of the point in extended coordinates (4 x_e : 4 y_e : 4 : 4 x_e y_e).
__global__ void __launch_bounds__(256) k_tail_items(const uint64_t* __restrict__ in, uint32_t n, int edw, uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t x[12], y[12], nz = 0;
#pragma unroll
  for (int k = 0; k < 12; k++) { x[k] = in[(size_t)i * 24 + k]; y[k] = in[(size_t)i * 24 + 12 + k]; nz |= x[k] | y[k]; }
  const XyzzRef dst = make_ref(out, n, i);
  if (nz == 0) { mem_set_inf(dst); return; }
  const Fq fx = fp_cond_sub_p(fp_from_abi<FqParams>(x)), fy = fp_cond_sub_p(fp_from_abi<FqParams>(y));
  if (!edw) {
    mem_st(dst, CX, fx); mem_st(dst, CY, fy); mem_st(dst, CZZ, fp_one<FqParams>()); mem_st(dst, CZZZ, fp_one<FqParams>());
    return;
  }
  EdwPacked e;
  if (!edw_from_affine(fx, fy, &e)) atomicAdd(bad, 1u);
  const Fq ymx = edw_ld(e.ymx), ypx = edw_ld(e.ypx), two = fp_dbl(fp_one<FqParams>());
  const Fq dx = fp_sub<FqParams, 2>(ypx, ymx);                                                // 2 x_e [3]
  const Fq sy = fp_add(ypx, ymx);                                                             // 2 y_e [2]
  mem_st(dst, CX, fp_mul(dx, two)); mem_st(dst, CY, fp_mul(sy, two)); mem_st(dst, CZZ, fp_mul(two, two)); mem_st(dst, CZZZ, fp_mul(dx, sy));
}
// ---- batch fixed-base scalar multiplication: out[i] = k_i * G (the inner loop of Groth16 setup:
// reference libzecale/circuits/aggregator_circuit.tcc:100-109 -> wsnarkT::generate_setup) ----
// table[w*15 + (d-1)] = d * 2^(4w) * G, w < 95, d = 1..15 (packed device form).
__device__ const uint32_t FQ_P_LIMBS_DEV[27] = {
    FqParams::P[0], FqParams::P[1], FqParams::P[2], FqParams::P[3], FqParams::P[4], FqParams::P[5], FqParams::P[6],
    FqParams::P[7], FqParams::P[8], FqParams::P[9], FqParams::P[10], FqParams::P[11], FqParams::P[12], FqParams::P[13],
    FqParams::P[14], FqParams::P[15], FqParams::P[16], FqParams::P[17], FqParams::P[18], FqParams::P[19], FqParams::P[20],
    FqParams::P[21], FqParams::P[22], FqParams::P[23], FqParams::P[24], FqParams::P[25], FqParams::P[26]};

__device__ __forceinline__ Fq fq_inv_fermat(const Fq& a) {
  // a^(p-2); exponent bits taken from the modulus limbs
  Fq acc = fp_one<FqParams>();
  for (int i = FqParams::NBITS - 1; i >= 0; i--) {
    acc = fp_sqr(acc);
    // bit i of p - 2 (p odd, p0 = ...8b so p - 2 only changes limb 0: 0x8b - 2 = 0x89)
    uint32_t limb = FQ_P_LIMBS_DEV[i / 29];
    if (i / 29 == 0) limb -= 2;
    if ((limb >> (i % 29)) & 1) acc = fp_mul(acc, a);
  }
  return acc;
}

__global__ void __launch_bounds__(256, 2) k_fixed_base_mul(const AffPacked* __restrict__ table, const uint64_t* __restrict__ scalars,
                                                            size_t n, int montgomery, uint32_t* __restrict__ work /* 108 x n */,
                                                            uint64_t* __restrict__ out_abi /* n x 24 */) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t s[6];
#pragma unroll
  for (int k = 0; k < 6; k++) s[k] = scalars[i * 6 + k];
  uint32_t w32[12];
  if (montgomery) {
    fp_abi_to_canonical_words<FrParams>(s, w32);
  } else {
#pragma unroll
    for (int k = 0; k < 6; k++) { w32[2 * k] = (uint32_t)s[k]; w32[2 * k + 1] = (uint32_t)(s[k] >> 32); }
  }
  XyzzRef acc = make_ref(work, (uint32_t)n, (uint32_t)i);
  bool inf = true;
  for (int w = 0; w < 95; w++) {
    uint32_t d = (w32[w >> 3] >> ((w & 7) * 4)) & 15u;
    if (d == 0) continue;
    const AffPacked* p = &table[w * 15 + (d - 1)];
    if (aff_is_inf(p)) continue;
    if (inf) {
      mem_st(acc, CX, aff_ld_x(p)); mem_st(acc, CY, aff_ld_y(p, false));
      mem_st(acc, CZZ, fp_one<FqParams>()); mem_st(acc, CZZZ, fp_one<FqParams>());
      inf = false;
      continue;
    }
    if (madd_mem(acc, p, false)) inf = mem_is_inf(acc);
  }
  uint64_t* o = out_abi + i * 24;
  if (inf) {
#pragma unroll
    for (int k = 0; k < 24; k++) o[k] = 0;
    return;
  }
  // x = X / ZZ, y = Y / ZZZ with one inversion: zi = 1 / (ZZ ZZZ).  A rolled 6-step micro-program.
  Fq zi = fp_zero<FqParams>(), t = zi;
#pragma unroll 1
  for (int step = 0; step < 6; step++) {
    Fq a, b;
    switch (step) {
      case 0: a = mem_ld(acc, CZZ); b = mem_ld(acc, CZZZ); break;
      case 1: a = zi; b = mem_ld(acc, CZZZ); break;       // 1/ZZ
      case 2: a = t; b = mem_ld(acc, CX); break;          // x
      case 3: a = zi; b = mem_ld(acc, CZZ); break;        // 1/ZZZ
      case 4: a = t; b = mem_ld(acc, CY); break;          // y
      default: a = zi; b = zi; break;
    }
    Fq r = fp_mul(a, b);
    switch (step) {
      case 0: zi = fq_inv_fermat(r); break;
      case 1: t = r; break;
      case 2: mem_st(acc, CX, r); break;
      case 3: t = r; break;
      case 4: mem_st(acc, CY, r); break;
      default: break;
    }
  }
  fp_to_abi<FqParams>(mem_ld(acc, CX), o);
  fp_to_abi<FqParams>(mem_ld(acc, CY), o + 12);
}

// ---- window tables: table[w * n + i] = 2^(off_w) P_i, affine, for w = 1 .. levels-1 (level 0 is the base set itself; off_w is
// the first bit of window w in the balanced layout, c*w for most of them).
// With the table every digit position of a scalar addresses the same bucket window (the entry points at the
// pre-shifted base), so one MSM has 2^(c-1) buckets instead of W * 2^(c-1): the bucket reduction shrinks W-fold and c
// can grow until the accumulation (n * ceil(378/c) mixed additions) stops shrinking.  Built once per base set (a
// proving key lives in HBM for the life of the server; 288 GB hold a 2^22 key 19 times over).
// One lane per point: a chain of c doublings per level on a memory-resident XYZZ accumulator, every level kept;
// then ONE inversion per point normalises all levels (Montgomery's trick over the levels: prefix products in a fifth
// coordinate row of the work array).  Setup-time code: the multiplications outside dbl_mem are out-of-line calls.
__device__ __noinline__ Fq fq_mul_ool(const Fq& a, const Fq& b) { return fp_mul(a, b); }

// XyzzRef over 5 coordinate rows (X, Y, ZZ, ZZZ, scratch)
__device__ __forceinline__ XyzzRef make_ref5(uint32_t* base, uint32_t stride, uint32_t idx) {
  XyzzRef r;
  r.rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)(135u * stride * 4u), 0x00020000);
  r.stride_b = stride * 4u;
  r.coord_b = 27u * stride * 4u;
  r.voff = idx * 4u;
  return r;
}

__global__ void __launch_bounds__(256, 2) k_table_build(AffPacked* __restrict__ table, uint8_t* __restrict__ tinf, size_t n, size_t i0,
                                                         uint32_t cn, WindowPlan plan, int levels, int every_bit, uint32_t* __restrict__ work, uint32_t stride) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cn) return;
  const size_t i = i0 + t;
  const AffPacked* p = &table[i];
  if (tinf[i]) {
    for (int w = 1; w < levels; w++) {
      AffPacked z;
#pragma unroll
      for (int k = 0; k < 24; k++) { z.x[k] = 0; z.y[k] = 0; }
      table[(size_t)w * n + i] = z;
      tinf[(size_t)w * n + i] = 1;
    }
    return;
  }
  const int CQ = 4;   // fifth row: prefix products
  // doubling chain
  for (int w = 1; w < levels; w++) {
    XyzzRef r = make_ref5(work, stride, (uint32_t)(w - 1) * cn + t);
    if (w == 1) {
      mem_st(r, CX, aff_ld_x(p)); mem_st(r, CY, aff_ld_y(p, false));
      mem_st(r, CZZ, fp_one<FqParams>()); mem_st(r, CZZZ, fp_one<FqParams>());
    } else {
      mem_copy(r, make_ref5(work, stride, (uint32_t)(w - 2) * cn + t));
    }
    const int nd = every_bit ? 1 : plan.bits[w - 1];       // level w = 2^(off_w) P, off_w - off_(w-1) = bits of window w-1 (every_bit: level w = 2^w P)
#pragma unroll 1
    for (int d = 0; d < nd; d++) dbl_mem(r);
  }
  // prefix products of ZZ * ZZZ over the finite levels
  Fq q = fp_one<FqParams>();
  for (int w = 1; w < levels; w++) {
    XyzzRef r = make_ref5(work, stride, (uint32_t)(w - 1) * cn + t);
    Fq zz = mem_ld(r, CZZ);
    if (!fp_is_zero_2p(zz)) q = fq_mul_ool(q, fq_mul_ool(zz, mem_ld(r, CZZZ)));
    mem_st(r, CQ, q);
  }
  Fq inv = fq_inv_fermat(q);      // q != 0: a product of non-zero field elements
  for (int w = levels - 1; w >= 1; w--) {
    XyzzRef r = make_ref5(work, stride, (uint32_t)(w - 1) * cn + t);
    Fq zz = mem_ld(r, CZZ);
    AffPacked o;
    uint8_t is_inf = 0;
    if (fp_is_zero_2p(zz)) {       // 2^(c w) P_i = O (a base outside the odd-order subgroup)
#pragma unroll
      for (int k = 0; k < 24; k++) { o.x[k] = 0; o.y[k] = 0; }
      is_inf = 1;
    } else {
      Fq zzz = mem_ld(r, CZZZ);
      Fq qprev = fp_one<FqParams>();
      if (w > 1) qprev = mem_ld(make_ref5(work, stride, (uint32_t)(w - 2) * cn + t), CQ);
      Fq tinv = fq_mul_ool(inv, qprev);                 // 1 / (ZZ ZZZ) of this level
      inv = fq_mul_ool(inv, fq_mul_ool(zz, zzz));       // inverse of the prefix below
      Fq x = fq_mul_ool(mem_ld(r, CX), fq_mul_ool(tinv, zzz));   // X / ZZ
      Fq y = fq_mul_ool(mem_ld(r, CY), fq_mul_ool(tinv, zz));    // Y / ZZZ
      fp_pack32<FqParams>(fp_cond_sub_p(x), o.x);
      fp_pack32<FqParams>(fp_cond_sub_p(y), o.y);
    }
    table[(size_t)w * n + i] = o;
    tinf[(size_t)w * n + i] = is_inf;
  }
}

// The Edwards table holds chi of the HALVED table points (msm_table_edw): H_i = [1/2 mod r] P_i, one lane per base, double-and-add
// over the bits of (r + 1) / 2 on an XYZZ accumulator in memory (work: 108 words per lane, limb-major, stride cn).  The same lane
// checks what the Edwards path needs of its base: y^2 = x^3 - 1 (a G2 set fails here, before any other work), and 2 H = P, which holds
// iff r P = O - order r, not merely odd order.  *bad counts the bases that fail; a base at infinity gives H = O.
__global__ void __launch_bounds__(256, 2) k_half_bases(const AffPacked* __restrict__ bases, const uint8_t* __restrict__ inf, AffPacked* __restrict__ out,
                                                        size_t i0, uint32_t cn, uint32_t* __restrict__ work, uint32_t* __restrict__ bad) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= cn) return;
  const size_t i = i0 + t;
  AffPacked o;
#pragma unroll
  for (int k = 0; k < 24; k++) { o.x[k] = 0; o.y[k] = 0; }
  if (inf[i]) { out[i] = o; return; }
  const AffPacked* p = bases + i;
  const Fq x = aff_ld_x(p), y = aff_ld_y(p, false), one = fp_one<FqParams>();
  const Fq rhs = fp_sub<FqParams, 4>(fp_add(fp_mul(y, y), one), fp_mul(fp_mul(x, x), x));        // y^2 + 1 - x^3 [7]
  if (!fp_is_zero_2p(fp_cond_sub_kp<FqParams, 2>(fp_cond_sub_kp<FqParams, 4>(rhs)))) { atomicAdd(bad, 1u); out[i] = o; return; }
  const XyzzRef acc = make_ref(work, cn, t);
  mem_st(acc, CX, x); mem_st(acc, CY, y); mem_st(acc, CZZ, one); mem_st(acc, CZZZ, one);
  constexpr int TOP = 375;                               // (r + 1) / 2 < 2^376, bit 375 set
#pragma unroll 1
  for (int j = TOP - 1; j >= 0; j--) {
    dbl_mem(acc);
    if ((FrParams::HALF_RAW[j / 29] >> (j % 29)) & 1u) {
      if (mem_is_inf(acc)) { mem_st(acc, CX, x); mem_st(acc, CY, y); mem_st(acc, CZZ, one); mem_st(acc, CZZZ, one); }
      else madd_mem(acc, p, false);
    }
  }
  const Fq zz = mem_ld(acc, CZZ), zzz = mem_ld(acc, CZZZ);
  bool ok = !fp_is_zero_2p(zz);
  if (ok) {
    const Fq tinv = fp_inv<FqParams>(fp_mul(zz, zzz));                                       // 1 / (ZZ ZZZ)
    const Fq hx = fp_cond_sub_p(fp_mul(mem_ld(acc, CX), fp_mul(tinv, zzz)));                   // X / ZZ
    const Fq hy = fp_cond_sub_p(fp_mul(mem_ld(acc, CY), fp_mul(tinv, zz)));                    // Y / ZZZ
    fp_pack32<FqParams>(hx, o.x);
    fp_pack32<FqParams>(hy, o.y);
    dbl_mem(acc);                                                                             // 2 H == P ?
    const Fq dzz = mem_ld(acc, CZZ);
    const Fq ex = fp_sub<FqParams, 16>(fp_mul(x, dzz), mem_ld(acc, CX));                      // X [<= 10]
    const Fq ey = fp_sub<FqParams, 8>(fp_mul(y, mem_ld(acc, CZZZ)), mem_ld(acc, CY));         // Y [<= 4]
    ok = !fp_is_zero_2p(dzz) && fp_is_zero_2p(fp_canon(ex)) && fp_is_zero_2p(fp_canon(ey));
  }
  if (!ok) atomicAdd(bad, 1u);
  out[i] = o;
}

// ---- the multiplier's own peak on THIS device, now (bench.py's fq_mul_frac divides by it) ----------------------------------------
// Two dependent chains of fp_mul per lane at the accumulation's occupancy (78 KiB of LDS per 256-lane block = two waves per SIMD):
// the kernel of tools/ubench/fqmul_occ_bench.hip inside the library.  The rate differs between boxes of the same model and between
// power states (420 .. 495 G wave-mads/s seen in round 4), so a fraction against a constant measured once means little.
__global__ void __launch_bounds__(256) k_fqmul_chain(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int iters) {
  extern __shared__ uint32_t lds_occ[];
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  Fq x, y;
#pragma unroll
  for (int i = 0; i < 27; i++) { x.l[i] = (in[i] ^ (tid & 0xffu)) & M29; y.l[i] = (in[27 + i] ^ ((tid >> 8) & 0xffu)) & M29; }
  x.l[26] &= 0x3fu; y.l[26] &= 0x3fu;
  if (iters < 0) lds_occ[threadIdx.x] = x.l[0];       // (keeps the allocation)
#pragma unroll 1
  for (int it = 0; it < iters; it++) { x = fp_mul(x, y); y = fp_mul(y, x); }
  uint32_t s_ = 0;
#pragma unroll
  for (int i = 0; i < 27; i++) s_ ^= x.l[i] + y.l[i];
  out[tid] = s_;
}

int msm_measure_fqmul_rate(double* fq_mul_per_s, char* errbuf, size_t errlen) {
  const int blocks = 256 * 2 * 4, iters = 100;
  const size_t lds = 78 * 1024;
  uint32_t *in = nullptr, *out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint32_t h[54];
  for (int i = 0; i < 54; i++) h[i] = (0x9e3779b9u * (uint32_t)(i + 1)) & M29;
  hipError_t e = hipMalloc(&in, sizeof h);
  if (e == hipSuccess) e = hipMalloc(&out, (size_t)blocks * 256 * 4);
  if (e == hipSuccess) e = hipMemcpy(in, h, sizeof h, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)k_fqmul_chain, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  float ms = 0;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fqmul_chain, dim3(blocks), dim3(256), lds, 0, in, out, 2);          // (code and clocks warm)
    hipLaunchKernelGGL(k_fqmul_chain, dim3(blocks), dim3(256), lds, 0, in, out, iters);
    for (int rep = 0; rep < 4 && e == hipSuccess; rep++) {                                   // a PEAK: the fastest of four launches
      float t = 0;
      e = hipEventRecord(e0, 0);
      hipLaunchKernelGGL(k_fqmul_chain, dim3(blocks), dim3(256), lds, 0, in, out, iters);
      if (e == hipSuccess) e = hipEventRecord(e1, 0);
      if (e == hipSuccess) e = hipEventSynchronize(e1);
      if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
      if (e == hipSuccess && (ms == 0 || t < ms)) ms = t;
    }
  }
  if (in) (void)hipFree(in);
  if (out) (void)hipFree(out);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (e != hipSuccess || ms <= 0) {
    if (errbuf) snprintf(errbuf, errlen, "msm_measure_fqmul_rate: %s", hipGetErrorString(e));
    return ZKHIP_ERR_HIP;
  }
  *fq_mul_per_s = (double)blocks * 256 * iters * 2 / (ms * 1e-3);
  return ZKHIP_OK;
}

// The three multiplier bodies of the DEVICE build on operands given limb by limb (tests/test_field_gpu.py: the worst cases of the
// column sums - every limb at 2^29 - 1, the top limb at the lazy bound - go through the same code the kernels run, and are checked
// against big integers on the host): out[i] = { a b / R, a^2 / R, (a b + c d) / R } for case i = (a, b, c, d), NL limbs each.
template <class PR>
__global__ void __launch_bounds__(64) k_field_selftest(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int N = PR::NL;
  Fp<PR> a, b, c, d;
  for (int k = 0; k < N; k++) { a.l[k] = in[(i * 4 + 0) * N + k]; b.l[k] = in[(i * 4 + 1) * N + k]; c.l[k] = in[(i * 4 + 2) * N + k]; d.l[k] = in[(i * 4 + 3) * N + k]; }
  const Fp<PR> m = fp_mul(a, b), q = fp_sqr(a), m2 = fp_mul2(a, b, c, d);
  for (int k = 0; k < N; k++) { out[(i * 3 + 0) * N + k] = m.l[k]; out[(i * 3 + 1) * N + k] = q.l[k]; out[(i * 3 + 2) * N + k] = m2.l[k]; }
}

int msm_field_selftest(int field, const uint32_t* in_host, size_t n, uint32_t* out_host, char* errbuf, size_t errlen) {
  const int N = field == 0 ? FqParams::NL : FrParams::NL;
  uint32_t *in = nullptr, *out = nullptr;
  hipError_t e = hipMalloc(&in, n * 4 * N * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&out, n * 3 * N * 4 + 4);
  if (e == hipSuccess) e = hipMemcpy(in, in_host, n * 4 * N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    if (field == 0) hipLaunchKernelGGL(k_field_selftest<FqParams>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
    else hipLaunchKernelGGL(k_field_selftest<FrParams>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out_host, out, n * 3 * N * 4, hipMemcpyDeviceToHost);
  if (in) (void)hipFree(in);
  if (out) (void)hipFree(out);
  if (e != hipSuccess) {
    if (errbuf) snprintf(errbuf, errlen, "msm_field_selftest: %s", hipGetErrorString(e));
    return ZKHIP_ERR_HIP;
  }
  return ZKHIP_OK;
}

// The rest of the field layer of the DEVICE build on raw limbs (tests/test_field_ops_gpu.py; cases and exact expectations from
// tests/field_ops_cases.py): the lazy linear operations, the range folds and the zero test, the packing, and fp_inv with its wave
// vote.  One lane per case, 64 lanes a workgroup: case i runs in wave i / 64 as lane i % 64, which is what the inversion cases are laid
// out by.  One op per launch (the switch is uniform).  in: n x (a, b, c), NL words each; out: n x (NL words, one flag word).
// fp_sub_k<K> is instantiated for the K its call sites use: Fq 1 (ec_edw.cuh) and 32 (pairing.cuh); Fr 16, 64, 128 and, through
// fr2_sub<K> / nf_sub<K>, 2, 4, 8, 16 (pairing_bls.cuh).
enum FieldOp : int {
  FO_ADD = 0, FO_DBL, FO_SUB2, FO_SUB4, FO_SUB8, FO_SUB16, FO_SUB_SUB2_8, FO_COND_SUB_P, FO_COND_SUB_KP1, FO_COND_SUB_KP2, FO_COND_SUB_KP4,
  FO_COND_SUB_KP8, FO_CANON_4P, FO_CANON, FO_IS_ZERO_2P, FO_UNPACK_PACK, FO_PACK_UNPACK, FO_ABI_ROUNDTRIP, FO_ABI_TO_CANONICAL_WORDS, FO_INV,
  FO_SUB_K = 32   // + log2 K
};
template <class PR>
constexpr bool field_op_known(int op) {
  if (op >= FO_ADD && op <= FO_INV) return true;
  const int K = (op >= FO_SUB_K && op < FO_SUB_K + 8) ? 1 << (op - FO_SUB_K) : 0;
  return PR::NL == FqParams::NL ? (K == 1 || K == 32) : (K == 2 || K == 4 || K == 8 || K == 16 || K == 64 || K == 128);
}
template <class PR, int K>
__device__ __forceinline__ Fp<PR> field_op_sub_k(const Fp<PR>& a, const Fp<PR>& b) {
  if constexpr (field_op_known<PR>(FO_SUB_K + __builtin_ctz(K))) return fp_sub_k<PR, K>(a, b);
  else return fp_zero<PR>();
}
template <class PR>
__global__ void __launch_bounds__(64) k_field_ops_selftest(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int N = PR::NL, W = PR::N32;
  static_assert(W <= N && 2 * PR::N64 == W, "");
  Fp<PR> a, b, c;
  for (int k = 0; k < N; k++) { a.l[k] = in[(i * 3 + 0) * N + k]; b.l[k] = in[(i * 3 + 1) * N + k]; c.l[k] = in[(i * 3 + 2) * N + k]; }
  Fp<PR> r = fp_zero<PR>();
  uint32_t flag = 0;
  uint32_t w[W];
  uint64_t x[PR::N64];
  switch (op) {
    case FO_ADD: r = fp_add(a, b); break;
    case FO_DBL: r = fp_dbl(a); break;
    case FO_SUB2: r = fp_sub<PR, 2>(a, b); break;
    case FO_SUB4: r = fp_sub<PR, 4>(a, b); break;
    case FO_SUB8: r = fp_sub<PR, 8>(a, b); break;
    case FO_SUB16: r = fp_sub<PR, 16>(a, b); break;
    case FO_SUB_SUB2_8: r = fp_sub_sub2<PR, 8>(a, b, c); break;
    case FO_COND_SUB_P: r = fp_cond_sub_p(a); break;
    case FO_COND_SUB_KP1: r = fp_cond_sub_kp<PR, 1>(a); break;
    case FO_COND_SUB_KP2: r = fp_cond_sub_kp<PR, 2>(a); break;
    case FO_COND_SUB_KP4: r = fp_cond_sub_kp<PR, 4>(a); break;
    case FO_COND_SUB_KP8: r = fp_cond_sub_kp<PR, 8>(a); break;
    case FO_CANON_4P: r = fp_canon_4p(a); break;
    case FO_CANON: r = fp_canon(a); break;
    case FO_IS_ZERO_2P: r = a; flag = fp_is_zero_2p(a) ? 1u : 0u; break;
    case FO_UNPACK_PACK:                              // a holds N32 packed words
      for (int k = 0; k < W; k++) w[k] = a.l[k];
      a = fp_unpack32<PR>(w);
      fp_pack32<PR>(a, w);
      for (int k = 0; k < W; k++) r.l[k] = w[k];
      break;
    case FO_PACK_UNPACK: fp_pack32<PR>(a, w); r = fp_unpack32<PR>(w); break;
    case FO_ABI_ROUNDTRIP: fp_to_abi<PR>(a, x); r = fp_from_abi<PR>(x); break;
    case FO_ABI_TO_CANONICAL_WORDS:                   // a holds the N64 ABI limbs as N32 words
      for (int k = 0; k < PR::N64; k++) x[k] = (uint64_t)a.l[2 * k] | ((uint64_t)a.l[2 * k + 1] << 32);
      fp_abi_to_canonical_words<PR>(x, w);
      for (int k = 0; k < W; k++) r.l[k] = w[k];
      break;
    case FO_INV: r = fp_inv<PR>(a); break;
    case FO_SUB_K + 0: r = field_op_sub_k<PR, 1>(a, b); break;
    case FO_SUB_K + 1: r = field_op_sub_k<PR, 2>(a, b); break;
    case FO_SUB_K + 2: r = field_op_sub_k<PR, 4>(a, b); break;
    case FO_SUB_K + 3: r = field_op_sub_k<PR, 8>(a, b); break;
    case FO_SUB_K + 4: r = field_op_sub_k<PR, 16>(a, b); break;
    case FO_SUB_K + 5: r = field_op_sub_k<PR, 32>(a, b); break;
    case FO_SUB_K + 6: r = field_op_sub_k<PR, 64>(a, b); break;
    case FO_SUB_K + 7: r = field_op_sub_k<PR, 128>(a, b); break;
    default: break;
  }
  for (int k = 0; k < N; k++) out[i * (N + 1) + k] = r.l[k];
  out[i * (N + 1) + N] = flag;
}

int msm_field_ops_selftest(int field, int op, const uint32_t* in_host, size_t n, uint32_t* out_host, char* errbuf, size_t errlen) {
  if (!(field == 0 ? field_op_known<FqParams>(op) : field_op_known<FrParams>(op))) {
    if (errbuf) snprintf(errbuf, errlen, "msm_field_ops_selftest: op %d is not one of field %d's", op, field);
    return ZKHIP_ERR_ARG;
  }
  const size_t N = field == 0 ? FqParams::NL : FrParams::NL;
  uint32_t *in = nullptr, *out = nullptr;
  hipError_t e = hipMalloc(&in, n * 3 * N * 4 + 4);
  if (e == hipSuccess) e = hipMalloc(&out, n * (N + 1) * 4 + 4);
  if (e == hipSuccess) e = hipMemcpy(in, in_host, n * 3 * N * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && n) {
    if (field == 0) hipLaunchKernelGGL(k_field_ops_selftest<FqParams>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, in, out, n);
    else hipLaunchKernelGGL(k_field_ops_selftest<FrParams>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, in, out, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out_host, out, n * (N + 1) * 4, hipMemcpyDeviceToHost);
  if (in) (void)hipFree(in);
  if (out) (void)hipFree(out);
  if (e != hipSuccess) {
    if (errbuf) snprintf(errbuf, errlen, "msm_field_ops_selftest: %s", hipGetErrorString(e));
    return ZKHIP_ERR_HIP;
  }
  return ZKHIP_OK;
}

// ------------------------------------------------------------------------------------------
// host orchestration
// ------------------------------------------------------------------------------------------
#define HIP_TRY(x)                                                                  \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      snprintf(ctx->errbuf, sizeof ctx->errbuf, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return ZKHIP_ERR_HIP;                                                         \
    }                                                                               \
  } while (0)

static inline unsigned nblk(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }
static int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  if (!e) return dflt;
  int v = atoi(e);
  return (v < lo || v > hi) ? dflt : v;
}
// target number of entries per lane and machine fill (tuning knob, read once).  48 / 80 / 160 give 83.3-83.7 / 84.1 / 81.9-83.2 Mscalar/s
// in the 2^20 stream: half the boundary pieces to stitch at 80; one fill per launch at 160 loses the overlap of fills
static size_t slice_target() {
  static const size_t v = (size_t)env_int("ZKHIP_SLICE_TARGET", 80, 8, 4096);
  return v;
}
static int g_aff_forced = -2;      // -2: not set (environment, then automatic); -1: automatic; >= 0: that many levels
void msm_force_aff_levels(int levels) { g_aff_forced = levels < -1 ? -1 : (levels > MSM_MAX_AFF_LEVELS ? MSM_MAX_AFF_LEVELS : levels); }
int msm_forced_aff_levels() { return g_aff_forced == -2 ? env_int("ZKHIP_AFF_LEVELS", -1, 0, MSM_MAX_AFF_LEVELS) : g_aff_forced; }
// The lockstep route of the Edwards accumulation (k_accumulate_edw_lock): ZKHIP_LOCKSTEP=0|1, read once; 0 forces every launch's
// lock_ok word to 0 (the sliced route).  msm_force_lockstep overrides the environment (A/B runs and tests: -1 = the environment
// again) and, with min_buckets >= 0, the number of non-empty buckets a launch needs (-1 = two waves for every SIMD of the chip).
#define ZK_LOCKSTEP_DEFAULT 1
static int g_lock_forced = -1, g_lock_min_live = -1;
void msm_force_lockstep(int mode, int min_buckets) { g_lock_forced = mode < 0 ? -1 : (mode ? 1 : 0); g_lock_min_live = min_buckets < 0 ? -1 : min_buckets; }
static int lockstep_mode() {
  static const int env_mode = env_int("ZKHIP_LOCKSTEP", ZK_LOCKSTEP_DEFAULT, 0, 1);
  return g_lock_forced >= 0 ? g_lock_forced : env_mode;
}
// the lock_ok word of the plan's last launch (1: the lockstep route ran, 0: the sliced one; -1: not an Edwards launch), copied
// back here and nowhere else: a test hook, synchronises the device
int msm_last_acc_path(MsmCtx* ctx, int* out) {
  *out = -1;
  if (!ctx->planned || !ctx->win_edw) return ZKHIP_OK;      // (a merged Edwards launch has no lockstep route: its word reads 0)
  uint32_t v = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&v, ctx->block_tot + 2, 4, hipMemcpyDeviceToHost));
  *out = (int)v;
  return ZKHIP_OK;
}

// One event per device, recorded the first time a plan is made there - and again whenever the caller asks (msm_time_base_reset):
// the origin of the absolute launch times of k_accumulate.  hipEventElapsedTime returns FLOAT milliseconds: 1 us of resolution
// lasts ~8 s from the origin, 0.06 ms an hour - a caller that compares intervals re-bases at the start of its timed region.
static hipEvent_t g_time_base[64];
static bool g_time_base_made[64];
static uint32_t g_time_base_gen[64];        // bumped by every reset: an interval whose launch predates the current origin is dropped
static std::mutex g_time_base_mu;           // plans are made under per-device or per-prover locks: several threads may arrive here
static hipEvent_t time_base_locked(int dev, bool renew) {
  if (!g_time_base_made[dev] && hipEventCreate(&g_time_base[dev]) != hipSuccess) return nullptr;
  if (!g_time_base_made[dev] || renew) {
    if (hipEventRecord(g_time_base[dev], 0) != hipSuccess || hipEventSynchronize(g_time_base[dev]) != hipSuccess) {
      if (!g_time_base_made[dev]) (void)hipEventDestroy(g_time_base[dev]);
      return nullptr;
    }
    g_time_base_made[dev] = true;
  }
  return g_time_base[dev];
}
hipEvent_t msm_time_base() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lk(g_time_base_mu);
  return time_base_locked(dev, false);
}
int msm_time_base_reset() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lk(g_time_base_mu);
  g_time_base_gen[dev]++;
  return time_base_locked(dev, true) ? ZKHIP_OK : ZKHIP_ERR_HIP;
}
static uint32_t time_base_gen() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lk(g_time_base_mu);
  return g_time_base_gen[dev];
}

// ZKHIP_DEBUG_DUMP=<dir>: the last launch's bucket populations and per-wave clocks of k_accumulate, for tools/acc_probe.py
// (synchronous copies: a measurement aid, never on in a timed run)
static void debug_dump(MsmCtx* ctx) {
  const char* dir = getenv("ZKHIP_DEBUG_DUMP");
  if (!dir || !ctx->dbg_times) return;
  const size_t nb = ctx->B * (size_t)ctx->W, nw = (size_t)ctx->T / 64 + 8;
  std::vector<uint32_t> cnt(nb);
  std::vector<uint64_t> tm(4 * nw);
  if (hipMemcpy(cnt.data(), ctx->counts, nb * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
  if (hipMemcpy(tm.data(), ctx->dbg_times, nw * 32, hipMemcpyDeviceToHost) != hipSuccess) return;
  char path[512];
  snprintf(path, sizeof path, "%s/acc_K%d_c%d_m%d.bin", dir, ctx->K, ctx->c, ctx->merged);
  FILE* f = fopen(path, "wb");
  if (!f) return;
  const uint64_t hdr[8] = {nb, nw, ctx->last_S, ctx->last_T, (uint64_t)ctx->last_tight, (uint64_t)ctx->K, (uint64_t)ctx->c, (uint64_t)ctx->merged};
  fwrite(hdr, 8, 8, f);
  fwrite(cnt.data(), 4, nb, f);
  fwrite(tm.data(), 8, 4 * nw, f);
  fclose(f);
}

int msm_last_entries(MsmCtx* ctx, uint64_t* out) {
  *out = 0;
  if (!ctx->last_hist_m) return ZKHIP_OK;
  uint32_t v = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&v, ctx->hist + ctx->last_hist_m - 1, 4, hipMemcpyDeviceToHost));
  *out = v;
  return ZKHIP_OK;
}

static void read_accumulate_times(MsmCtx* ctx) {
  debug_dump(ctx);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, ctx->lane->ev_acc0, ctx->lane->ev_acc1);
  ctx->last_accumulate_ms = ms;
  hipEvent_t base = msm_time_base();
  float t0 = 0, t1 = 0;
  // (a launch recorded before the last msm_time_base_reset would be measured against an origin that lies AFTER it: no interval)
  if (ctx->acc_gen != time_base_gen()) { ctx->last_acc_begin_ms = ctx->last_acc_end_ms = -1.f; return; }
  if (base && hipEventElapsedTime(&t0, base, ctx->lane->ev_acc0) == hipSuccess && hipEventElapsedTime(&t1, base, ctx->lane->ev_acc1) == hipSuccess) {
    ctx->last_acc_begin_ms = t0; ctx->last_acc_end_ms = t1;
  }
}

// (non-blocking streams: no implicit ordering against the null stream - the host application's, e.g. torch's)
hipError_t msm_lane_create_main(MsmLane* lane) { return lane->main ? hipSuccess : hipStreamCreateWithFlags(&lane->main, hipStreamNonBlocking); }
hipError_t msm_lane_create_side(MsmLane* lane) { return lane->side ? hipSuccess : hipStreamCreateWithFlags(&lane->side, hipStreamNonBlocking); }
// (ev_done, the end of a launch sequence, is BLOCKING: the host thread that collects the result sleeps instead of spinning - provers wait side by side and share the cores with the witness generators)
hipError_t msm_lane_create_events(MsmLane* lane) {
  const std::pair<hipEvent_t*, unsigned> want[] = {{&lane->ev, hipEventDisableTiming}, {&lane->ev2, hipEventDisableTiming}, {&lane->ev_acc0, hipEventDefault},
                                                   {&lane->ev_acc1, hipEventDefault}, {&lane->ev_done, hipEventBlockingSync | hipEventDisableTiming}};
  for (const auto& [ev, flags] : want) if (!*ev) { const hipError_t e = hipEventCreateWithFlags(ev, flags); if (e != hipSuccess) return e; }
  return hipSuccess;
}
void msm_lane_free(MsmLane* lane) {
  for (hipStream_t st : {lane->main, lane->side}) if (st) (void)hipStreamDestroy(st);
  for (hipEvent_t ev : {lane->ev, lane->ev2, lane->ev_acc0, lane->ev_acc1, lane->ev_done}) if (ev) (void)hipEventDestroy(ev);
  *lane = MsmLane{};
}
int msm_one_stream(int one_stream) { return one_stream >= 0 ? (one_stream ? 1 : 0) : env_int("ZKHIP_MSM_ONE_STREAM", 0, 0, 1); }

int msm_plan_init(MsmCtx* ctx, MsmLane* lane, size_t max_n, int c, int merged, int K, size_t total_terms, int one_stream) {
  memset(ctx, 0, sizeof *ctx);
  ctx->total_terms = total_terms = plan::total_terms(K, max_n, total_terms);
  if (K < 1 || K > MSM_MAX_JOBS || (!merged && K != 1)) return ZKHIP_ERR_ARG;
  if (!(ctx->lane = lane) || !lane->main || !lane->ev || !lane->ev2 || !lane->ev_acc0 || !lane->ev_acc1 || !lane->ev_done) return ZKHIP_ERR_ARG;
  ctx->K = K;
  ctx->quad_below = (uint32_t)env_int("ZKHIP_QUAD_BELOW", 65536, 1, 1 << 30);
  ctx->one_stream = msm_one_stream(one_stream);
  // 108 * (W * 2^(c-1) + 2T) * 4 bytes must stay below 4 GiB (buffer descriptor); checked below
  if (c < 4 || c > (merged ? 22 : 18)) return ZKHIP_ERR_ARG;
  ctx->c = c;
  ctx->merged = merged;
  ctx->Wd = plan::digits(c, merged);
  ctx->W = merged ? K : ctx->Wd;
  // plain and merged plans share the balanced layout: a table's level w is 2^(off_w) P.  (A short top window would also
  // hurt a merged plan: its n digits of a few bits would all land in a handful of the shared buckets.)
  plan::window_layout(c, ctx->win_off, ctx->win_bits);
  ctx->B = (size_t)1 << (c - 1);
  ctx->max_n = max_n;
  ctx->logL = env_int("ZKHIP_SUM_LOGL", 2, 2, 5); ctx->L = 1 << ctx->logL;      // fan-in of the reduction trees (tuning knob; the R arrays are sized for L >= 4)
  size_t nb = ctx->B * ctx->W;
  if ((size_t)ctx->Wd * max_n >= ((size_t)1 << 31)) return ZKHIP_ERR_ARG;   // entry = 31-bit point index + sign
  if ((size_t)ctx->Wd * total_terms >= ((size_t)1 << 32)) return ZKHIP_ERR_ARG;  // positions in the entry list are 32-bit
  const int sort_parts = env_int("ZKHIP_SORT_PARTS", 1024, 64, 8192), sort_tile = env_int("ZKHIP_SORT_TILE", 1024, 256, 16384);      // (tuning knobs)
  if (!plan::sort_plan(c, merged, ctx->Wd, nb, max_n, sort_parts, sort_tile, ctx->sort_LB, ctx->sort_NP, ctx->sort_bins, ctx->sort_tile, ctx->hist_len)) return ZKHIP_ERR_ARG;
  HIP_TRY(hipMalloc(&ctx->hist, ctx->hist_len * 4));
  HIP_TRY(hipMalloc(&ctx->pairs, plan::cap_entries(ctx->Wd, total_terms) * sizeof(uint2)));
  HIP_TRY(hipMalloc(&ctx->counts, nb * 4));
  HIP_TRY(hipMalloc(&ctx->offsets, nb * 4));
  HIP_TRY(hipMalloc(&ctx->goff, (nb + 1) * 4));
  if ((size_t)ctx->Wd * total_terms * ZK_W_NEXT >= ((size_t)1 << 32)) return ZKHIP_ERR_ARG;      // slice weights are 32-bit
  HIP_TRY(hipMalloc(&ctx->block_tot, plan::cap_block_tot(nb, ctx->hist_len, ZK_LOCK_KEYS) * 4));      // (see enqueue_scan)
  if (merged == 1 && K == 1) {      // a plan that may serve Edwards launches: the lockstep route's bucket order
    HIP_TRY(hipMalloc(&ctx->order, nb * 4));
    HIP_TRY(hipMalloc(&ctx->ord_hist, (size_t)ZK_LOCK_KEYS * nblk(nb, 1024) * 4));
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    ctx->lock_min_live = plan::lock_min_live(cus);
  }
  HIP_TRY(hipMalloc(&ctx->entries, plan::cap_entries(ctx->Wd, total_terms) * 4));
  // Batched-affine levels before the XYZZ accumulation: NONE unless forced (zkhip_set_affine_levels, ZKHIP_AFF_LEVELS; tested: the same
  // group element; slower than the XYZZ kernel: DESIGN.md section 5).  Bounds on the level sizes, the buffers of their outputs:
  ctx->aff_forced = msm_forced_aff_levels();
  ctx->aff_levels = ctx->aff_forced >= 0 ? ctx->aff_forced : 0;
  ctx->aff_m = (uint32_t)env_int("ZKHIP_AFF_M", 64, 4, 512);
  size_t bound[MSM_MAX_AFF_LEVELS + 1];
  bound[0] = (size_t)ctx->Wd * total_terms;
  for (int l = 0; l < ctx->aff_levels; l++) {
    bound[l + 1] = plan::level_bound(bound[l], nb);
    HIP_TRY(hipMalloc(&ctx->lcnt[l], nb * 4));
    HIP_TRY(hipMalloc(&ctx->loff[l], nb * 4));
  }
  ctx->aff_lanes = plan::aff_lanes(ctx->aff_m, ctx->aff_levels, plan::level_bound(bound[0], nb));
  if (ctx->aff_levels > 0) {
    HIP_TRY(hipMalloc(&ctx->pbuf[0], (bound[1] + 1) * sizeof(AffPacked)));
    if (ctx->aff_levels > 1) HIP_TRY(hipMalloc(&ctx->pbuf[1], (bound[2] + 1) * sizeof(AffPacked)));
    HIP_TRY(hipMalloc(&ctx->aff_scratch, (size_t)ctx->aff_lanes * plan::aff_m_cap(ctx->aff_m) * plan::AFF_SCRATCH_BYTES));
  }
  ctx->m_acc_max = bound[ctx->aff_levels];
  if (!plan::slice_plan(ctx->m_acc_max, nb, slice_target(), ZK_SLOT_WORDS, ctx->S, ctx->T, ctx->slot_stride)) return ZKHIP_ERR_ARG;
  HIP_TRY(hipMalloc(&ctx->buckets, (size_t)ctx->slot_stride * ZK_SLOT_WORDS * 4));
  if (getenv("ZKHIP_DEBUG_DUMP")) HIP_TRY(hipMalloc(&ctx->dbg_times, ((size_t)ctx->T / 64 + 8) * 32));
  HIP_TRY(hipMalloc(&ctx->prio_board, (size_t)ZK_PRIO_BOARD_WORDS * 4));          // 8 XCC x 8 SE x 2 SH x 16 CU x 4 SIMD x 16 wave slots
  HIP_TRY(hipMemset(ctx->prio_board, 0, (size_t)ZK_PRIO_BOARD_WORDS * 4));
  const size_t pt = plan::POINT_WORDS * 4;      // bytes of a point of the reduction scratch
  HIP_TRY(hipMalloc(&ctx->fix_list, plan::cap_fix_list(ctx->T) * sizeof(uint2)));
  HIP_TRY(hipMalloc(&ctx->fix_short, plan::cap_fix_short(ctx->T) * sizeof(uint2)));
  HIP_TRY(hipMalloc(&ctx->segS[0], plan::cap_segS(nb) * pt));
  HIP_TRY(hipMalloc(&ctx->segS[1], plan::cap_segS(nb) * pt));
  HIP_TRY(hipMalloc(&ctx->colS[0], plan::cap_segS(nb) * pt));
  HIP_TRY(hipMalloc(&ctx->colS[1], plan::cap_segS(nb) * pt));
  HIP_TRY(hipMalloc(&ctx->hilo, plan::cap_hilo(ctx->W, c) * pt));
  for (int k = 0; k < 2; k++) HIP_TRY(hipMalloc(&ctx->planes[k], plan::cap_tail(ctx->W, (size_t)1 << plan::lo_bits(c), k) * pt));
  HIP_TRY(hipMalloc(&ctx->win_abi, (size_t)ctx->W * 48 * 8 * 2));       // (the second half: the plain totals of a NAF plan)
  HIP_TRY(hipHostMalloc(&ctx->win_host, (size_t)ctx->W * 48 * 8 * 2));
  ctx->planned = true;
  return ZKHIP_OK;
}

void msm_plan_free(MsmCtx* ctx) {
  void* ptrs[] = {ctx->hist, ctx->pairs, ctx->counts, ctx->offsets, ctx->block_tot, ctx->entries, ctx->buckets,
                  ctx->segS[0], ctx->segS[1], ctx->planes[0], ctx->planes[1], ctx->win_abi,
                  ctx->colS[0], ctx->colS[1], ctx->hilo, ctx->pbuf[0], ctx->pbuf[1], ctx->aff_scratch,
                  ctx->lcnt[0], ctx->lcnt[1], ctx->lcnt[2], ctx->lcnt[3], ctx->loff[0], ctx->loff[1], ctx->loff[2], ctx->loff[3],
                  ctx->fix_list, ctx->fix_short, ctx->dbg_times, ctx->goff, ctx->prio_board, ctx->order, ctx->ord_hist};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (ctx->win_host) (void)hipHostFree(ctx->win_host);
  memset(ctx, 0, sizeof *ctx);
}

int msm_bases_convert(const uint64_t* d_bases_abi, size_t n, AffPacked* d_out, uint8_t* d_inf_flags, char* errbuf, size_t errlen) {
  hipLaunchKernelGGL(k_bases_to_dev, dim3(nblk(n, 256)), dim3(256), 0, 0, d_bases_abi, d_out, d_inf_flags, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    if (errbuf) snprintf(errbuf, errlen, "msm_bases_convert: %s", hipGetErrorString(e));
    return ZKHIP_ERR_HIP;
  }
  return ZKHIP_OK;
}

// Enqueue one MSM on the context's streams and return without waiting (the prover keeps two contexts
// in flight so that the latency-bound reduction of one MSM overlaps the accumulation of the next).
int msm_launch(MsmCtx* ctx, const AffPacked* d_bases, const uint8_t* d_inf_flags, const uint64_t* d_scalars, size_t n,
               int scalars_montgomery, size_t table_stride, const EdwPacked* edw) {
  MsmJob job{d_bases, d_inf_flags, d_scalars, n, scalars_montgomery, table_stride, 0, edw};
  return msm_launch_multi(ctx, 1, &job);
}

// Exclusive prefix sum of m words, in -> out (may be the same array).  block_tot holds a scan's block totals while it runs; AFTER the
// launch's last scan its words [0], [1] are the lengths of the two stitching lists (zeroed by stage_accumulate, counted by
// k_accumulate) and [2] is lock_ok (written by k_bucket_order<1> behind its own scan): no scan may follow that memset.
static void enqueue_scan(hipStream_t st, const uint32_t* in, uint32_t* out, uint32_t* block_tot, size_t m) {
  const unsigned sb = nblk(m, 1024);
  hipLaunchKernelGGL(k_scan_local, dim3(sb), dim3(256), 0, st, in, out, block_tot, m);
  hipLaunchKernelGGL(k_scan_tot, dim3(1), dim3(1024), 0, st, block_tot, (size_t)sb);
  hipLaunchKernelGGL(k_scan_add, dim3(sb), dim3(256), 0, st, out, block_tot, m);
}
struct RedKernels {      // the stitching and reduction kernels that exist for XYZZ and for Edwards points (red_kernels)
  void (*fold_quad)(ZK_FOLD_PARAMS), (*fold)(ZK_FOLD_PARAMS);
  void (*sum_lds)(ZK_SUM_PARAMS), (*sum_quad)(ZK_SUM_PARAMS);
  void (*plane_sum)(ZK_PLANE_PARAMS), (*plane_combine)(ZK_PCOMB_PARAMS);
};
struct Launch {      // what the stages of one msm_launch_multi share
  int K;                                  // jobs of this launch (<= ctx->K)
  const MsmJob* jobs;
  size_t nb;                              // buckets of all windows
  bool edw;                               // the Edwards accumulation and reduction (see msm_launch_multi)
  uint32_t wf;                            // slice weight of a bucket's first entry
  int bshift;                             // bucket -> job
  BasePtrs bp;                            // the points the entries index: every job's bases, then the last affine level's sums
  const uint32_t *cur_off, *cur_cnt;      // the list k_accumulate sums: the sort's, then every affine level's
  size_t m_cur;                           // bound on its entries
  uint32_t S_run, T_run;                  // slice length and slices for THIS launch (the plan's slot array is sized for max_n)
  int tight;                              // slices cut by weight, not by entry count (slice_len); 0 for provers that share the chip
  RedKernels red;                         // the XYZZ or the Edwards kernels of the stitching and the reduction
};

// (1) bucket sort: count per (part, block) in LDS, scan, place by part, then order every part by its low bucket bits.  The bucket
// windows of the jobs this call does not use (K < ctx->K) stay empty: their rows of hist are written as zeros by grid row k.
static int stage_sort(MsmCtx* ctx, const Launch& lp) {
  const int KK = ctx->merged ? ctx->K : 1;                       // every bucket window's rows of hist are (re)written
  hipStream_t st = ctx->lane->main;
  WindowPlan wp = {};
  for (int w = 0; w < ctx->Wd; w++) { wp.off[w] = ctx->win_off[w]; wp.bits[w] = ctx->win_bits[w]; }
  DigitJobs dj = {};
  size_t n_max = 0;      // terms of the longest job
  for (int k = 0; k < lp.K; k++) {
    const MsmJob& j = lp.jobs[k];
    dj.scalars[k] = j.scalars; dj.inf_flags[k] = j.inf_flags; dj.n[k] = j.n; dj.tab_stride[k] = j.table_stride; dj.mode[k] = j.scalars_mode;
    if (j.n > n_max) n_max = j.n;
  }
  SortGeom ge;
  ge.LB = ctx->sort_LB; ge.NP = ctx->sort_NP; ge.bins = ctx->sort_bins; ge.tile = ctx->sort_tile;
  ge.nbx = nblk(n_max, ge.tile);
  ge.nparts = (uint32_t)(lp.nb >> ge.LB);
  const size_t hist_m = plan::hist_m(lp.nb, ge.LB, ge.nbx);
  if (hist_m > ctx->hist_len) return ZKHIP_ERR_ARG;
  ctx->last_hist_m = hist_m;
  for (int pass = 0; pass < 2; pass++) {      // (NAF digits or plain ones; LDS: the counters, in pass 1 the bases too)
    const bool naf = ctx->merged == 2;
    const auto digit_pass = !pass ? (naf ? k_digit_pass<0, true> : k_digit_pass<0, false>) : (naf ? k_digit_pass<1, true> : k_digit_pass<1, false>);
    hipLaunchKernelGGL(digit_pass, dim3(ge.nbx, KK), dim3(256), (size_t)ge.bins * 4 * (pass + 1), st, dj, ctx->c, ctx->Wd, wp, ctx->merged, ge, ctx->hist, ctx->pairs);
    if (pass == 0) enqueue_scan(st, ctx->hist, ctx->hist, ctx->block_tot, hist_m);
  }
  hipLaunchKernelGGL(k_bucket_sort, dim3(ge.nparts), dim3(512), 0, st, ctx->hist, ge, ctx->pairs, ctx->entries, ctx->offsets, ctx->counts);
  HIP_TRY(hipGetLastError());
  return ZKHIP_OK;
}

// (2) batched-affine levels: the sorted list is summed pairwise inside every bucket, ctx->aff_levels times
static int stage_affine_levels(MsmCtx* ctx, Launch& lp) {
  hipStream_t st = ctx->lane->main;
  ctx->acc_gen = time_base_gen();
  if (ctx->aff_levels > 0) HIP_TRY(hipEventRecord(ctx->lane->ev_acc0, st));     // the timed accumulation includes the affine levels
  for (int l = 0; l < ctx->aff_levels; l++) {
    const size_t m_out = plan::level_bound(lp.m_cur, lp.nb);
    hipLaunchKernelGGL(k_half_counts, dim3(nblk(lp.nb, 256)), dim3(256), 0, st, lp.cur_cnt, ctx->lcnt[l], lp.nb);
    enqueue_scan(st, ctx->lcnt[l], ctx->loff[l], ctx->block_tot, lp.nb);
    LevelArgs la;
    la.bp = lp.bp; la.bshift = lp.bshift; la.entries = ctx->entries; la.src = l ? ctx->pbuf[(l - 1) & 1] : nullptr;
    la.in_off = lp.cur_off; la.in_cnt = lp.cur_cnt; la.out_off = ctx->loff[l];
    la.nb = (uint32_t)lp.nb; la.m = plan::aff_outputs_per_lane(m_out, ctx->aff_m); la.dst = ctx->pbuf[l & 1]; la.scratch = ctx->aff_scratch;
    const size_t lanes_tot = (m_out + la.m - 1) / la.m;
    for (size_t lane0 = 0; lane0 < lanes_tot; lane0 += ctx->aff_lanes) {
      const size_t ln = lanes_tot - lane0 < ctx->aff_lanes ? lanes_tot - lane0 : ctx->aff_lanes;
      la.lane0 = (uint32_t)lane0; la.lanes = ctx->aff_lanes;       // row length of the scratch: fixed; lanes beyond ln do not exist
      const auto level = l == 0 ? (ctx->K == 1 ? k_affine_level<1, true> : k_affine_level<MSM_MAX_JOBS, true>) : k_affine_level<1, false>;
      hipLaunchKernelGGL(level, dim3(nblk(ln, 256)), dim3(256), 0, st, la);
    }
    lp.cur_off = ctx->loff[l]; lp.cur_cnt = ctx->lcnt[l]; lp.m_cur = m_out;
  }
  if (ctx->aff_levels > 0) lp.bp.p[0] = ctx->pbuf[(ctx->aff_levels - 1) & 1];
  HIP_TRY(hipGetLastError());
  return ZKHIP_OK;
}

// (3) slice weights, the lockstep route's bucket order, the slot array's zero fill, the accumulation between ev_acc0 and ev_acc1
static int stage_accumulate(MsmCtx* ctx, Launch& lp) {
  hipStream_t st = ctx->lane->main;
  const size_t nb = lp.nb;
  const bool dense = ctx->aff_levels > 0;
  // slice weights: goff = exclusive scan of (8 count - 7) over the non-empty buckets of the list k_accumulate sums (nb + 1 values)
  hipLaunchKernelGGL(k_slice_weights, dim3(nblk(nb + 1, 256)), dim3(256), 0, st, lp.cur_cnt, ctx->goff, nb, lp.wf);
  enqueue_scan(st, ctx->goff, ctx->goff, ctx->block_tot, nb + 1);
  const bool lock_route = lp.edw && ctx->K == 1;      // (merged Edwards launches, K > 1, are sliced only: no order, lock_ok = 0)
  if (lock_route) {      // the lockstep route's bucket order and its go / no-go word, block_tot[2]
    const unsigned ob = nblk(nb, 1024);
    const int lock_on = lockstep_mode();
    const uint32_t min_live = g_lock_min_live >= 0 ? (uint32_t)g_lock_min_live : ctx->lock_min_live;
    hipLaunchKernelGGL(k_bucket_order<0>, dim3(ob), dim3(256), 0, st, lp.cur_cnt, (uint32_t)nb, ctx->ord_hist, ctx->order, ctx->block_tot + 2, min_live, lock_on);
    enqueue_scan(st, ctx->ord_hist, ctx->ord_hist, ctx->block_tot, (size_t)ZK_LOCK_KEYS * ob);
    hipLaunchKernelGGL(k_bucket_order<1>, dim3(ob), dim3(256), 0, st, lp.cur_cnt, (uint32_t)nb, ctx->ord_hist, ctx->order, ctx->block_tot + 2, min_live, lock_on);
  }
  // the lengths of the two stitching lists: the launch's scans are done (enqueue_scan); an Edwards launch without the lockstep route clears lock_ok too
  HIP_TRY(hipMemsetAsync(ctx->block_tot, 0, (lp.edw && !lock_route) ? 12 : 8, st));
  size_t n_jobs = 0;
  for (int k = 0; k < lp.K; k++) n_jobs += lp.jobs[k].n ? 1 : 0;
  lp.S_run = (uint32_t)plan::slice_run(lp.m_cur, slice_target(), ctx->one_stream ? (size_t)env_int("ZKHIP_STREAM_SLICE_MULT", 2, 1, 16) : 1, ctx->merged ? ctx->B * (n_jobs ? n_jobs : 1) : nb, ctx->T);
  lp.T_run = nblk(lp.m_cur, lp.S_run);
  lp.tight = (ctx->one_stream || dense) ? 0 : env_int("ZKHIP_TIGHT_SLICES", 1, 0, 1);      // (a streaming prover shares the chip: see slice_len)
  // all-zero ZZ = infinity is what every reader of a slot tests first (mem_is_inf; X, Y, ZZZ of an infinite slot are copied along at
  // most, never used): only the 27 ZZ rows of the limb-major array need the zero fill - a quarter of the bytes
#if ZK_SLOTS_AOS
  static const int clear_mode = env_int("ZKHIP_SLOTS_CLEAR", 0, 0, 1);      // 0: the ZZ words only (a kernel); 1: the whole array (one memset, four times the bytes, whole lines)
  if (clear_mode == 1) HIP_TRY(hipMemsetAsync(ctx->buckets, 0, (size_t)ctx->slot_stride * ZK_SLOT_WORDS * 4, st));
  else hipLaunchKernelGGL(k_slots_clear_zz, dim3(nblk((size_t)ctx->slot_stride * 27, 256)), dim3(256), 0, st, ctx->buckets, ctx->slot_stride);
#else
  HIP_TRY(hipMemsetAsync(ctx->buckets + (size_t)CZZ * 27 * ctx->slot_stride, 0, (size_t)ctx->slot_stride * 27 * 4, st));
#endif
  if (ctx->dbg_times) HIP_TRY(hipMemsetAsync(ctx->dbg_times, 0, ((size_t)ctx->T / 64 + 8) * 32, st));
  if (ctx->acc_gate) HIP_TRY(hipStreamWaitEvent(st, ctx->acc_gate, 0));
  if (!dense) HIP_TRY(hipEventRecord(ctx->lane->ev_acc0, st));
  static const int acc_prio = env_int("ZKHIP_ACC_PRIO", 1, 0, 2);      // 2: by quarters of the slice only (no board)
  const uint32_t prio_tag = (++ctx->prio_seq & 0x7fffu) + 1u;     // (see k_accumulate: the wave that is behind asks for priority; 0 = the arbiter's own order)
  if (lock_route)
    hipLaunchKernelGGL(k_accumulate_edw_lock, dim3(nblk(nb, 256)), dim3(256), 0, st, lp.jobs[0].edw, ctx->entries, lp.cur_off, lp.cur_cnt, ctx->order, (uint32_t)nb, ctx->buckets, ctx->slot_stride, ctx->block_tot + 2);
  const auto accumulate = lp.edw ? (lock_route ? k_accumulate_edw : k_accumulate_edw_multi) : (ctx->K == 1 || dense) ? k_accumulate<1> : k_accumulate<MSM_MAX_JOBS>;
  hipLaunchKernelGGL(accumulate, dim3(nblk(lp.T_run, 256)), dim3(256), 0, st, lp.bp, lp.bshift, dense ? (const uint32_t*)nullptr : ctx->entries, lp.cur_off, lp.cur_cnt, ctx->goff, (uint32_t)nb,
                     lp.S_run, lp.tight, lp.T_run, ctx->buckets, ctx->slot_stride, ctx->block_tot + 0, ctx->fix_short, ctx->fix_list, ctx->dbg_times, acc_prio, (acc_prio == 1 && !ctx->one_stream) ? ctx->prio_board : (uint32_t*)nullptr, prio_tag);
  HIP_TRY(hipEventRecord(ctx->lane->ev_acc1, st));
  ctx->last_S = lp.S_run; ctx->last_T = lp.T_run; ctx->last_tight = lp.tight;
  HIP_TRY(hipGetLastError());
  return ZKHIP_OK;
}
// (stands HERE, its candidates in THIS order: the device code keeps its template kernels in the order of their first use on the host,
// see profiles/msm_driver_refactor_codeobj.txt.  k_fixup / k_fixup_edw differ in their arguments and stay a branch.)
static RedKernels red_kernels(bool edw) {
  return {edw ? k_fixup_fold_edw<true> : k_fixup_fold<true>, edw ? k_fixup_fold_edw<false> : k_fixup_fold<false>,
          edw ? k_sum_lds_edw : k_sum_lds,                   edw ? k_sum_edw<true> : k_sum<true>,
          edw ? k_plane_sum_edw : k_plane_sum,               edw ? k_plane_combine_edw : k_plane_combine};
}

// (4) stitching: fold the F pieces of the buckets that have several (lists made by k_accumulate), then L + F for every cut bucket
static int stage_stitch(MsmCtx* ctx, const Launch& lp) {
  hipStream_t st = ctx->lane->main;
  const uint32_t nb = (uint32_t)lp.nb, T_run = lp.T_run;
  if (T_run > 2) {
    const bool fold_quads = T_run < (1u << 18) && ctx->quad_below > 1024;     // a small launch that has the chip to itself is latency-bound
    const uint32_t sblocks = std::min(1024u, nblk((size_t)T_run / 2 + 1, fold_quads ? 64u : 256u));      // (the list is walked with a grid stride)
    // + 512 workgroups for the long list (a wrapping proof has ~290 buckets of 7-8 pieces; 128 workgroups took three sweeps of three rounds)
    hipLaunchKernelGGL(fold_quads ? lp.red.fold_quad : lp.red.fold, dim3(sblocks + 512), dim3(256), 0, st, ctx->block_tot, ctx->fix_short, ctx->fix_list, sblocks, nb, ctx->buckets, ctx->slot_stride);
  }
  if (lp.edw)
    hipLaunchKernelGGL(k_fixup_edw, dim3(nblk(T_run, 256)), dim3(256), 0, st, lp.cur_off, lp.cur_cnt, ctx->goff, nb, lp.S_run, lp.tight, T_run, ctx->buckets, ctx->slot_stride, lp.wf, ctx->block_tot + 2);
  else
    hipLaunchKernelGGL(k_fixup, dim3(nblk(T_run, 256)), dim3(256), 0, st, lp.cur_off, lp.cur_cnt, ctx->goff, nb, lp.S_run, lp.tight, T_run, ctx->buckets, ctx->slot_stride, lp.wf);
  HIP_TRY(hipGetLastError());
  return ZKHIP_OK;
}

// out[t] = the sum of L items of `in`, row_len apart (k_sum).  Fewer outputs than quad_below: the launch is latency-bound, a quad of
// lanes per addition finishes it sooner (at ~twice the lane-cycles: a prover that shares the chip with others lowers the threshold)
static void enqueue_sum(MsmCtx* ctx, const Launch& lp, hipStream_t s, uint32_t* in, size_t n_in, uint32_t in_stride, int L, uint32_t row_len, uint32_t* out) {
  const size_t n_out = n_in / L;
  const int in_slots = (in == ctx->buckets) ? 1 : 0;          // the first level reads the slot array (an array of structures: ec_mem.cuh)
  if (n_out >= ctx->quad_below) hipLaunchKernelGGL(lp.red.sum_lds, dim3(nblk(n_out, 256)), dim3(256), 0, s, in, n_in, in_stride, L, row_len, out, in_slots);
  else hipLaunchKernelGGL(lp.red.sum_quad, dim3(nblk(n_out * 4, 256)), dim3(256), 0, s, in, n_in, in_stride, L, row_len, out, in_slots);
}
// A tree over the slot array [W][H][R]: the `left` items of every row (contiguous: col_stride 0) or column (col_stride R apart) are
// summed to one; returns the result.  Halving-style grouping inside each row (item lo' + u * left/L): lanes of a wave read adjacent
// slots (L CONSECUTIVE items make every lane stride L slots).  left > 1: msm_plan_init refuses c < 4, so lo_bits >= 2, hi_bits >= 1.
static uint32_t* enqueue_tree(MsmCtx* ctx, const Launch& lp, hipStream_t s, uint32_t left, uint32_t col_stride, uint32_t* const buf[2]) {
  uint32_t* in = ctx->buckets; uint32_t in_stride = ctx->slot_stride; size_t n_in = lp.nb; int pp = 0;
  while (left > 1) {
    const int L = plan::tree_fan_in(ctx->L, n_in, left, ctx->quad_below);
    enqueue_sum(ctx, lp, s, in, n_in, in_stride, L, col_stride ? col_stride : left / L, buf[pp]);
    n_in /= L; left /= L; in = buf[pp]; in_stride = (uint32_t)n_in; pp ^= 1;
  }
  return in;
}

// The tail of the reduction: 2W groups of N items (limb-major, stride 2W N, weights index + 1; the hi groups first) -> the W window
// results R * hi + lo in ABI limbs, W plain totals of the lo groups behind them if `total`.  By bit planes (msm_plan.hpp): one
// k_plane_sum launch per tree level - at most six, N <= 2048 - and k_plane_combine, all on ONE stream, no events.
// planes[0], planes[1]: cap_tail points each.
static void enqueue_tail(const RedKernels& red, hipStream_t st, uint32_t* items, int W, uint32_t N, int lo_bits, bool total,
                         uint32_t* const planes[2], uint64_t* out_abi) {
  const int G = 2 * W, wp = plan::tail_weight_planes(N), P = plan::tail_planes(N, total);
  uint32_t* in = items;
  uint32_t in_stride = (uint32_t)G * N, left = N;
  for (int level = 0; left > 1; level++) {
    const int L = plan::tail_fan_in(left);
    const size_t n_out = plan::tail_level_outputs(P, G, N, level);
    hipLaunchKernelGGL(red.plane_sum, dim3(nblk(n_out * 4, 256)), dim3(256), 0, st, in, in_stride, (uint32_t)G * left, left, L, P, level == 0 ? 1 : 0,
                       total ? wp : -1, planes[level & 1]);
    in = planes[level & 1]; in_stride = (uint32_t)n_out; left /= (uint32_t)L;
  }
  hipLaunchKernelGGL(red.plane_combine, dim3(W), dim3(256), 0, st, in, W, wp, total ? 1 : 0, lo_bits, out_abi);
}

// (5) bucket reduction: (a) two-level split of the bucket index (row sums on stream 1, column sums on stream 2: plain trees), (b) the two
// small weighted sums per window by bit planes and (c) per window R * hi + lo (enqueue_tail), on stream 1.
static int stage_reduce(MsmCtx* ctx, const Launch& lp) {
  hipStream_t st = ctx->lane->main;
  // the row and the column tree run side by side on two streams - unless this context shares the chip with others anyway (one_stream)
  hipStream_t st2 = (ctx->one_stream || !ctx->lane->side) ? ctx->lane->main : ctx->lane->side;
  const int c = ctx->c, W = ctx->W, G = 2 * W;
  const uint32_t Rr = 1u << plan::lo_bits(c), Hh = 1u << plan::hi_bits(c), Nn = Rr > Hh ? Rr : Hh;
  HIP_TRY(hipEventRecord(ctx->lane->ev, st));
  HIP_TRY(hipStreamWaitEvent(st2, ctx->lane->ev, 0));
  uint32_t* rows = enqueue_tree(ctx, lp, st, Rr, 0, ctx->segS);       // [W][H][R] -> [W][H]  (sum over lo, contiguous)
  uint32_t* cols = enqueue_tree(ctx, lp, st2, Hh, Rr, ctx->colS);     // [W][H][R] -> [W][R]  (sum over hi, stride R)
  HIP_TRY(hipEventRecord(ctx->lane->ev2, st2));
  HIP_TRY(hipStreamWaitEvent(st, ctx->lane->ev2, 0));
  hipLaunchKernelGGL(k_place_hilo, dim3(nblk((size_t)G * Nn * 4, 256)), dim3(256), 0, st, rows, cols, (uint32_t)W, Hh, Rr, Nn, ctx->hilo);
  enqueue_tail(lp.red, st, ctx->hilo, W, Nn, plan::lo_bits(c), ctx->merged == 2, ctx->planes, ctx->win_abi);
  HIP_TRY(hipGetLastError());
  return ZKHIP_OK;
}

// (6) the window results to the host; ev_done ends the launch sequence
static int stage_copy_out(MsmCtx* ctx, const Launch& lp) {
  HIP_TRY(hipMemcpyAsync(ctx->win_host, ctx->win_abi, (size_t)ctx->W * 48 * 8 * (ctx->merged == 2 ? 2 : 1), hipMemcpyDeviceToHost, ctx->lane->main));
  HIP_TRY(hipEventRecord(ctx->lane->ev_done, ctx->lane->main));
  ctx->win_edw = lp.edw;      // what win_host will hold for THIS launch (the context may serve an XYZZ set next)
  ctx->pending = true;        // only a completely enqueued sequence is collectable; a failed launch leaves the context reusable
  return ZKHIP_OK;
}

int msm_launch_multi(MsmCtx* ctx, int K, const MsmJob* jobs) {
  const int c = ctx->c, Wd = ctx->Wd, merged = ctx->merged;
  if (K < 1 || K > ctx->K) return ZKHIP_ERR_ARG;
  size_t n_tot = 0, n_eff = 0;
  Launch lp;      // the launch sequence: the stage functions above, in stream order
  lp.K = K;
  lp.jobs = jobs;
  for (int k = 0; k < K; k++) {
    if (jobs[k].n > ctx->max_n) return ZKHIP_ERR_ARG;
    n_eff += msm_job_terms(jobs[k]);
    if (n_eff > ctx->total_terms) return ZKHIP_ERR_ARG;          // (the entry list and the slices are sized for total_terms)
    if (merged && jobs[k].n && (jobs[k].table_stride < jobs[k].n || (size_t)(merged == 2 ? 378 : Wd) * jobs[k].table_stride >= ((size_t)1 << 31))) return ZKHIP_ERR_ARG;
    n_tot += jobs[k].n;
  }
  ctx->pending_n = n_tot;
  ctx->win_edw = false;
  if (n_tot == 0) { ctx->pending = true; return ZKHIP_OK; }
  // the Edwards accumulation (ec_edw.cuh): MSMs over one-level-per-window tables that have their Edwards form, no batched-affine
  // levels in front - a single MSM, or up to four in a merged plan when EVERY job that has terms brings its Edwards table (a mixed
  // set of jobs runs as XYZZ).  The digits are XYZZ's (the table holds chi of the HALVED points); the slots, the stitching and the bucket
  // reduction hold Edwards points (the k_..._edw kernels), and the host maps the window results back (win_edw: edw_abi_to_jac).
  lp.edw = merged == 1 && ctx->K <= 4 && ctx->aff_levels == 0;
  for (int k = 0; k < K; k++) if (jobs[k].n && !jobs[k].edw) lp.edw = false;
  lp.wf = lp.edw ? ZK_W_NEXT : ZK_W_FIRST;
  lp.red = red_kernels(lp.edw);
  lp.nb = ctx->B * ctx->W;
  lp.bshift = merged ? c - 1 : 31;
  for (int k = 0; k < MSM_MAX_JOBS; k++) lp.bp.p[k] = jobs[k < K ? k : 0].bases;
  if (lp.edw) for (int k = 0; k < K; k++) lp.bp.p[k] = reinterpret_cast<const AffPacked*>(jobs[k].edw);     // (k_accumulate_edw[_multi] read them as EdwPacked)
  lp.cur_off = ctx->offsets;
  lp.cur_cnt = ctx->counts;
  lp.m_cur = (size_t)Wd * (n_eff ? n_eff : 1);       // entries that can occur: a base at infinity never produces one
  int r = stage_sort(ctx, lp);
  if (!r) r = stage_affine_levels(ctx, lp);
  if (!r) r = stage_accumulate(ctx, lp);
  if (!r) r = stage_stitch(ctx, lp);
  if (!r) r = stage_reduce(ctx, lp);
  return r ? r : stage_copy_out(ctx, lp);
}

// Wait for the MSM enqueued by msm_launch and finish it on the host.
static void xyzz_abi_to_jac(const uint64_t* p, host::HJac& q) {
  using namespace host;
  HFq X = HFq::from_limbs(p), Y = HFq::from_limbs(p + 12), ZZ = HFq::from_limbs(p + 24), ZZZ = HFq::from_limbs(p + 36);
  if (ZZ.is_zero()) { q = HJac::infinity(); return; }
  // XYZZ -> Jacobian with Z = ZZ*ZZZ:  X' = X ZZ ZZZ^2,  Y' = Y ZZ^3 ZZZ^2
  HFq z3s = ZZZ.sqr(), zz2 = ZZ.sqr();
  q.X = X * ZZ * z3s;
  q.Y = Y * zz2 * ZZ * z3s;
  q.Z = ZZ * ZZZ;
}

// The window result of an Edwards launch, (X : Y : Z : T) in ABI limbs: psi (ec_edw.cuh) takes it to the XYZZ point of G1 -
//   W = Z^2 - Y^2, lambda = X W, ZZ = lambda^2, ZZZ = lambda^3, X' = (X^2 + c1 Z^2) W^2, Y' = c2 Y Z^2 ZZ
// (x = 1 + c1 Z^2 / X^2, y = c2 Y Z^2 / (X W): tools/gen_params.py edwards_params).  psi is a homomorphism, so psi of the weighted
// bucket sum is the weighted sum of the buckets' images: twelve host products per MSM.  X = 0 - the identity, or an empty window
// (all zeros) - gives ZZ = 0: infinity.
static void edw_abi_to_jac(const uint64_t* p, host::HJac& q) {
  using namespace host;
  const HFq X = HFq::from_limbs(p), Y = HFq::from_limbs(p + 12), Z = HFq::from_limbs(p + 24);
  const HFq c1 = HFq::from_limbs(FqParams::EDW_C1_64), c2 = HFq::from_limbs(FqParams::EDW_C2_64);
  const HFq Z2 = Z.sqr(), Wv = Z2 - Y.sqr(), lam = X * Wv, ZZ = lam.sqr();
  uint64_t xyzz[48];
  ((X.sqr() + c1 * Z2) * Wv.sqr()).to_limbs(xyzz);
  (c2 * Y * Z2 * ZZ).to_limbs(xyzz + 12);
  ZZ.to_limbs(xyzz + 24);
  (ZZ * lam).to_limbs(xyzz + 36);
  xyzz_abi_to_jac(xyzz, q);
}

int msm_finish_multi(MsmCtx* ctx, int K, uint64_t* out_jac) {
  using namespace host;
  if (!ctx->pending || !ctx->merged || K < 1 || K > ctx->K) return ZKHIP_ERR_STATE;
  ctx->pending = false;
  if (ctx->pending_n) {
    HIP_TRY(zk_event_wait(ctx->lane->ev_done));
    read_accumulate_times(ctx);
  }
  for (int k = 0; k < K; k++) {
    HJac q = HJac::infinity();
    if (ctx->pending_n && ctx->win_edw) edw_abi_to_jac(ctx->win_host + (size_t)k * 48, q);      // (an Edwards launch: merged = 1, psi once per job)
    else if (ctx->pending_n) xyzz_abi_to_jac(ctx->win_host + (size_t)k * 48, q);    // one bucket window per job: nothing to combine
    if (ctx->pending_n && ctx->merged == 2) {                                  // odd digits: sum (2 b + 1) S_b = 2 F - sum S_b
      HJac tot;
      xyzz_abi_to_jac(ctx->win_host + (size_t)(ctx->K + k) * 48, tot);
      if (!tot.is_inf()) tot.Y = tot.Y.neg();
      q = q.dbl().add(tot);
    }
    q.X.to_limbs(out_jac + 36 * k); q.Y.to_limbs(out_jac + 36 * k + 12); q.Z.to_limbs(out_jac + 36 * k + 24);
  }
  return ZKHIP_OK;
}

int msm_finish(MsmCtx* ctx, uint64_t out_jac[36]) {
  using namespace host;
  if (!ctx->pending) return ZKHIP_ERR_STATE;
  if (ctx->merged) return msm_finish_multi(ctx, 1, out_jac);
  ctx->pending = false;
  const int W = ctx->W;
  if (ctx->pending_n == 0) {
    HJac inf = HJac::infinity();
    inf.X.to_limbs(out_jac); inf.Y.to_limbs(out_jac + 12); inf.Z.to_limbs(out_jac + 24);
    return ZKHIP_OK;
  }
  HIP_TRY(zk_event_wait(ctx->lane->ev_done));
  read_accumulate_times(ctx);

  // host: sum_w 2^(c w) W_w  (Horner from the top window)
  HJac acc = HJac::infinity();
  for (int w = W - 1; w >= 0; w--) {
    for (int d = 0; d < ctx->win_bits[w]; d++) acc = acc.dbl();
    HJac q;
    xyzz_abi_to_jac(ctx->win_host + (size_t)w * 48, q);
    acc = acc.add(q);
  }
  acc.X.to_limbs(out_jac); acc.Y.to_limbs(out_jac + 12); acc.Z.to_limbs(out_jac + 24);
  return ZKHIP_OK;
}

// Test hook: the tail of the reduction alone (enqueue_tail) on 2W groups of N points given as affine ABI points on the host, the hi
// groups first, weights index + 1.  An Edwards run maps every item through chi and the results back through psi: psi(chi(P)) = 2P,
// so it returns TWICE the weighted sums.  out_jac: W Jacobian points R * hi + lo, W plain totals of the lo groups behind them if total.
int msm_tail_selftest(int edw, const uint64_t* items_aff, int W, uint32_t N, int lo_bits, int total, uint64_t* out_jac, char* errbuf, size_t errlen) {
  using namespace host;
  if (W < 1 || W > MSM_MAX_JOBS || N < 2 || N > 2048 || (N & (N - 1)) || lo_bits < 0 || lo_bits > 11 || !items_aff || !out_jac) return ZKHIP_ERR_ARG;
  const size_t n = (size_t)2 * W * N, pt = plan::POINT_WORDS * 4, n_out = (size_t)W * (total ? 2 : 1);
  uint64_t *d_aff = nullptr, *d_abi = nullptr;
  uint32_t *d_items = nullptr, *planes[2] = {nullptr, nullptr}, *d_bad = nullptr, bad = 0;
  std::vector<uint64_t> abi(n_out * 48);
  hipError_t e = hipMalloc(&d_aff, n * 24 * 8);
  if (e == hipSuccess) e = hipMalloc(&d_items, n * pt);
  for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipMalloc(&planes[k], plan::cap_tail(W, N, k) * pt);
  if (e == hipSuccess) e = hipMalloc(&d_abi, n_out * 48 * 8);
  if (e == hipSuccess) e = hipMalloc(&d_bad, 4);
  if (e == hipSuccess) e = hipMemset(d_bad, 0, 4);
  if (e == hipSuccess) e = hipMemcpy(d_aff, items_aff, n * 24 * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_tail_items, dim3(nblk(n, 256)), dim3(256), 0, 0, d_aff, (uint32_t)n, edw, d_items, d_bad);
    enqueue_tail(red_kernels(edw != 0), 0, d_items, W, N, lo_bits, total != 0, planes, d_abi);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(abi.data(), d_abi, n_out * 48 * 8, hipMemcpyDeviceToHost);      // (synchronises)
  if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
  for (void* q : {(void*)d_aff, (void*)d_items, (void*)planes[0], (void*)planes[1], (void*)d_abi, (void*)d_bad}) if (q) (void)hipFree(q);
  if (e != hipSuccess || bad) {
    if (errbuf) snprintf(errbuf, errlen, e != hipSuccess ? "msm_tail_selftest: %s" : "msm_tail_selftest: items without an Edwards image%s", e != hipSuccess ? hipGetErrorString(e) : "");
    return e != hipSuccess ? ZKHIP_ERR_HIP : ZKHIP_ERR_ARG;
  }
  for (size_t k = 0; k < n_out; k++) {
    HJac q;
    if (edw) edw_abi_to_jac(abi.data() + k * 48, q); else xyzz_abi_to_jac(abi.data() + k * 48, q);
    q.X.to_limbs(out_jac + 36 * k); q.Y.to_limbs(out_jac + 36 * k + 12); q.Z.to_limbs(out_jac + 36 * k + 24);
  }
  return ZKHIP_OK;
}

int msm_table_build(AffPacked* d_table, uint8_t* d_tinf, size_t n, int c, int naf, char* errbuf, size_t errlen) {
  const int levels = msm_table_levels(c, naf);
  if (n == 0 || levels < 2) return ZKHIP_OK;
  WindowPlan wp;
  memset(&wp, 0, sizeof wp);
  plan::window_layout(c, wp.off, wp.bits);
  // points per launch: (levels - 1) * chunk slots of 135 words, at most 4M slots (2.2 GB of work space)
  size_t chunk = ((size_t)1 << 22) / (size_t)(levels - 1);
  chunk &= ~(size_t)255;
  if (chunk > n) chunk = n;
  const uint32_t stride = (uint32_t)(chunk * (size_t)(levels - 1));
  uint32_t* work = nullptr;
  hipError_t e = hipMalloc(&work, (size_t)stride * 135 * 4);
  for (size_t i0 = 0; e == hipSuccess && i0 < n; i0 += chunk) {
    uint32_t cn = (uint32_t)((n - i0 < chunk) ? n - i0 : chunk);
    hipLaunchKernelGGL(k_table_build, dim3(nblk(cn, 256)), dim3(256), 0, 0, d_table, d_tinf, n, i0, cn, wp, levels, naf ? 1 : 0, work, stride);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (work) (void)hipFree(work);
  if (e != hipSuccess) {
    if (errbuf) snprintf(errbuf, errlen, "msm_table_build: %s", hipGetErrorString(e));
    return ZKHIP_ERR_HIP;
  }
  return ZKHIP_OK;
}

int msm_table_edw(const AffPacked* d_bases, const uint8_t* d_inf, size_t n, int c, EdwPacked** d_out, char* errbuf, size_t errlen) {
  *d_out = nullptr;
  if (n == 0) return ZKHIP_OK;
  const size_t levels = (size_t)msm_table_levels(c, 0), chunk = n < ((size_t)1 << 21) ? n : ((size_t)1 << 21);
  AffPacked* half = nullptr;
  uint8_t* hinf = nullptr;
  uint32_t *work = nullptr, *d_bad = nullptr, bad = 0;
  EdwPacked* et = nullptr;
  int rc = ZKHIP_OK;
  hipError_t e = hipMalloc(&d_bad, 4);
  if (e == hipSuccess) e = hipMemset(d_bad, 0, 4);
  if (e == hipSuccess) e = hipMalloc(&half, levels * n * sizeof(AffPacked));
  if (e == hipSuccess) e = hipMalloc(&hinf, levels * n);
  if (e == hipSuccess) e = hipMemcpy(hinf, d_inf, n, hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMalloc(&work, chunk * 108 * 4);
  // level 0: H_i = [1/2] P_i, checked; the set is rejected (ZKHIP_ERR_ARG) before anything else is computed if a base fails
  for (size_t i0 = 0; e == hipSuccess && i0 < n; i0 += chunk) {
    const uint32_t cn = (uint32_t)(n - i0 < chunk ? n - i0 : chunk);
    hipLaunchKernelGGL(k_half_bases, dim3(nblk(cn, 256)), dim3(256), 0, 0, d_bases, d_inf, half, i0, cn, work, d_bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && bad) {
    if (errbuf) snprintf(errbuf, errlen, "msm_table_edw: %u bases are not points of order r on G1's curve", bad);
    rc = ZKHIP_ERR_ARG;
  }
  if (e == hipSuccess && rc == ZKHIP_OK) {
    if (work) { (void)hipFree(work); work = nullptr; }
    // levels w >= 1: 2^(off_w) H_i = [1/2] 2^(off_w) P_i, by the table build itself; then chi of every entry
    rc = msm_table_build(half, hinf, n, c, 0, errbuf, errlen);
    if (rc == ZKHIP_OK) {
      e = hipMemset(d_bad, 0, 4);
      if (e == hipSuccess) e = hipMalloc(&et, levels * n * sizeof(EdwPacked));
      if (e == hipSuccess) {
        hipLaunchKernelGGL(k_table_edw, dim3(nblk(levels * n, 256)), dim3(256), 0, 0, half, hinf, et, levels * n, d_bad);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);      // (synchronises)
      if (e == hipSuccess && bad) {                // (order-r points never hit chi's exceptional points: a failed check above)
        if (errbuf) snprintf(errbuf, errlen, "msm_table_edw: %u table points without an Edwards image", bad);
        rc = ZKHIP_ERR_ARG;
      }
    }
  }
  if (e != hipSuccess) {
    if (errbuf) snprintf(errbuf, errlen, "msm_table_edw: %s", hipGetErrorString(e));
    rc = ZKHIP_ERR_HIP;
  }
  for (void* q : {(void*)half, (void*)hinf, (void*)work, (void*)d_bad}) if (q) (void)hipFree(q);
  if (rc == ZKHIP_OK) *d_out = et;
  else if (et) (void)hipFree(et);
  return rc;
}

// out[i] = k_i * base for i < n.  base: ABI affine (host); d_scalars, d_out: device memory.
int fixed_base_mul(const uint64_t base_aff[24], const uint64_t* d_scalars, size_t n, int montgomery, uint64_t* d_out,
                   char* errbuf, size_t errlen) {
  using namespace host;
  struct { char errbuf[256]; } c_, *ctx = &c_;
  ctx->errbuf[0] = 0;
  // table on the host: 95 windows x 15 multiples, affine, ABI form -> device packed form
  std::vector<uint64_t> tab((size_t)95 * 15 * 24);
  HJac wbase = HJac::from_affine(HFq::from_limbs(base_aff), HFq::from_limbs(base_aff + 12));
  for (int w = 0; w < 95; w++) {
    HJac m = wbase;
    for (int d = 1; d <= 15; d++) {
      HFq x, y;
      m.to_affine(x, y);
      x.to_limbs(&tab[((size_t)w * 15 + d - 1) * 24]);
      y.to_limbs(&tab[((size_t)w * 15 + d - 1) * 24 + 12]);
      m = m.add(wbase);
    }
    for (int k = 0; k < 4; k++) wbase = wbase.dbl();
  }
  uint64_t* d_tab_abi = nullptr;
  AffPacked* d_tab = nullptr;
  uint32_t* d_work = nullptr;
  int rc = ZKHIP_OK;
  do {
    hipError_t e;
    if ((e = hipMalloc(&d_tab_abi, tab.size() * 8)) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
    if ((e = hipMalloc(&d_tab, (size_t)95 * 15 * sizeof(AffPacked))) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
    if ((e = hipMalloc(&d_work, n * 108 * 4)) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
    if ((e = hipMemcpy(d_tab_abi, tab.data(), tab.size() * 8, hipMemcpyHostToDevice)) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
    hipLaunchKernelGGL(k_bases_to_dev, dim3(nblk(95 * 15, 256)), dim3(256), 0, 0, d_tab_abi, d_tab, (uint8_t*)nullptr, (size_t)95 * 15);
    hipLaunchKernelGGL(k_fixed_base_mul, dim3(nblk(n, 256)), dim3(256), 0, 0, d_tab, d_scalars, n, montgomery, d_work, d_out);
    if ((e = hipGetLastError()) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
    if ((e = hipDeviceSynchronize()) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
  } while (0);
  if (rc != ZKHIP_OK && errbuf) snprintf(errbuf, errlen, "fixed_base_mul: HIP failure (%s)", hipGetErrorString(hipGetLastError()));
  if (d_tab_abi) (void)hipFree(d_tab_abi);
  if (d_tab) (void)hipFree(d_tab);
  if (d_work) (void)hipFree(d_work);
  return rc;
}

}  // namespace zkhip
