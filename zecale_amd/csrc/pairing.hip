// Groth16 verification over BW6-761 in batches on the device: the pairing of pairing_host.hpp (the reference's wsnarkT::verify,
// libzecale/tests/aggregator/aggregator_dummy_test.cpp:61-62) as two kernels over the lane bodies of pairing.cuh, and
// acc = ABC_0 + sum x_i ABC_i per proof.
//
// A verification owns a GROUP of eight lanes (pairing.cuh explains the cut); a workgroup of 128 threads holds 16 of them.  The group's
// state lives in LDS: the accumulator twice (an operation reads one copy and writes the other, so ONE barrier separates two operations),
// the lines of the four pairs and their running points.  Every loop has a fixed trip count (376 Miller iterations, the exponent's bit
// length, the scalar's 377 bits); the only synchronisation is the workgroup barrier, which every thread of a workgroup reaches the same
// number of times: groups past the end of the batch recompute the last verification and store nothing.  No waits, no spins, no atomics.
//
// Checked batches put k_point_check in front: one lane per proof point (and per key point, once), no LDS and no barrier, so a lane
// leaves at its first failure.  It writes one code per element; a proof with any code set is FLAGGED, and the kernels behind read its
// points and inputs as the point at infinity and zero (the `flags` arguments, null on the unchecked route).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <vector>

#include "ec.cuh"
#include "fp_inv.cuh"
#include "host_field.hpp"
#include "pairing.cuh"
#include "pairing.h"
#include "pairing_host.hpp"

namespace zkhip {

constexpr int PAIRING_BLOCK = 128;
constexpr int PAIRING_WG = PAIRING_BLOCK / PAIRING_GROUP;      // verifications per workgroup
// (PAIRING_STRIP, the strip of the combined batches' reduction trees, is pairing.cuh's: the lane bodies and the host shim read it too)
constexpr size_t PAIRING_CHUNK = 16384;                        // verifications per launch sequence (bounds the work space)

// ---- ABI points -> the constants of a Miller loop.  One lane per pair.
__global__ void __launch_bounds__(64) k_pair_prep(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2,
                                                  const uint64_t* __restrict__ quarter /* 1/4, -1/4 (ABI) */, size_t n,
                                                  MillerConst* __restrict__ pairs, uint32_t* __restrict__ inf,
                                                  const uint32_t* __restrict__ flags /* per product, or null */, int np) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flags && flags[i / np]) {                    // a flagged proof: its four pairs are pairs of points at infinity, its product is 1
    MillerConst z;
    z.px = z.py = z.xq4 = z.yq4n = fp_zero<FqParams>();
    pairs[i] = z;
    inf[i] = 1u;
    return;
  }
  uint64_t nz1 = 0, nz2 = 0;
  for (int k = 0; k < 24; k++) { nz1 |= g1[i * 24 + k]; nz2 |= g2[i * 24 + k]; }
  MillerConst c;
  c.px = fp_from_abi<FqParams>(g1 + i * 24);
  c.py = fp_from_abi<FqParams>(g1 + i * 24 + 12);
  c.xq4 = fp_mul(fp_from_abi<FqParams>(g2 + i * 24), fp_from_abi<FqParams>(quarter));
  c.yq4n = fp_mul(fp_from_abi<FqParams>(g2 + i * 24 + 12), fp_from_abi<FqParams>(quarter + 12));
  pairs[i] = c;
  inf[i] = (nz1 == 0 || nz2 == 0) ? 1u : 0u;     // a pair with a member at infinity contributes 1
}

// f <- f * line_p for the group's pairs, one after the other: every coefficient lane reads copy `cur`, writes the other, barrier.
__device__ __forceinline__ void fold_lines(Fq (*F)[6], const Fq (*L)[3], int np, int k, int& cur) {
#pragma unroll 1
  for (int p = 0; p < np; p++) {
    if (k < 6) F[cur ^ 1][k] = fq6_mul_line_coeff(k, F[cur], L[p]);
    __syncthreads();
    cur ^= 1;
  }
}

// ---- f = prod_p f_{r,P_p}(psi(Q_p)): the shared-accumulator Miller loop of pairing_host.hpp, `np` pairs per product.
__global__ void __launch_bounds__(PAIRING_BLOCK) k_miller(const MillerConst* __restrict__ pairs, const uint32_t* __restrict__ inf, int np,
                                                          size_t count, const uint64_t* __restrict__ r_order, Fq* __restrict__ f_out) {
  __shared__ Fq sF[PAIRING_WG][2][6];
  __shared__ Fq sL[PAIRING_WG][PAIRING_MAX_PAIRS][3];
  __shared__ MillerPoint sT[PAIRING_WG][PAIRING_MAX_PAIRS];
  const int g = threadIdx.x / PAIRING_GROUP, k = threadIdx.x % PAIRING_GROUP;
  size_t slot = (size_t)blockIdx.x * PAIRING_WG + g;
  const bool live = slot < count;
  if (!live) slot = count - 1;
  const bool pt = k < np;                                   // this lane runs the point steps of pair k
  const MillerConst* c = pairs + slot * np + (pt ? k : 0);
  bool done = true;
  if (pt) {
    done = inf[slot * np + k] != 0;
    sT[g][k].X = c->px;
    sT[g][k].Y = c->py;
    sT[g][k].Z = fp_one<FqParams>();
  }
  if (k < 6) sF[g][0][k] = k == 0 ? fp_one<FqParams>() : fp_zero<FqParams>();
  __syncthreads();
  int cur = 0;
#pragma unroll 1
  for (int i = PAIRING_MILLER_STEPS - 1; i >= 0; i--) {
    // the accumulator's squaring on the coefficient lanes and the pairs' doubling steps on lanes 0 .. np - 1 touch disjoint state
    if (k < 6) sF[g][cur ^ 1][k] = fq6_mul_coeff(k, sF[g][cur], sF[g][cur]);
    if (pt) miller_double_step(sT[g][k], *c, done, sL[g][k]);
    __syncthreads();
    cur ^= 1;
    fold_lines(sF[g], sL[g], np, k, cur);
    if ((r_order[i >> 6] >> (i & 63)) & 1) {                // the same bit for every thread of the launch
      if (pt) done = miller_add_step(sT[g][k], *c, done, sL[g][k]);
      __syncthreads();
      fold_lines(sF[g], sL[g], np, k, cur);
    }
  }
  if (live && k < 6) f_out[slot * 6 + k] = sF[g][cur][k];
}

// ---- f^((q^6-1)/r) by square-and-multiply over the exponent's `nbits` bits (pairing_host.hpp pow_limbs), then ABI limbs.
__global__ void __launch_bounds__(PAIRING_BLOCK) k_final_exp(const Fq* __restrict__ f_in, const uint64_t* __restrict__ e, int nbits, size_t count,
                                                             uint64_t* __restrict__ gt) {
  __shared__ Fq sF[PAIRING_WG][2][6];
  __shared__ Fq sB[PAIRING_WG][6];
  const int g = threadIdx.x / PAIRING_GROUP, k = threadIdx.x % PAIRING_GROUP;
  size_t slot = (size_t)blockIdx.x * PAIRING_WG + g;
  const bool live = slot < count;
  if (!live) slot = count - 1;
  if (k < 6) { sB[g][k] = f_in[slot * 6 + k]; sF[g][0][k] = sB[g][k]; }
  __syncthreads();
  int cur = 0;
#pragma unroll 1
  for (int i = nbits - 2; i >= 0; i--) {
    if (k < 6) sF[g][cur ^ 1][k] = fq6_mul_coeff(k, sF[g][cur], sF[g][cur]);
    __syncthreads();
    cur ^= 1;
    if ((e[i >> 6] >> (i & 63)) & 1) {                      // the same bit for every thread
      if (k < 6) sF[g][cur ^ 1][k] = fq6_mul_coeff(k, sF[g][cur], sB[g]);
      __syncthreads();
      cur ^= 1;
    }
  }
  if (live && k < 6) fp_to_abi<FqParams>(sF[g][cur][k], gt + slot * 72 + k * 12);       // [4] -> canonical
}

// ---- the lane bodies on operands given as ABI limbs (zkhip_internal_fq6_selftest)
__global__ void __launch_bounds__(PAIRING_BLOCK) k_fq6_selftest(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t n,
                                                                uint64_t* __restrict__ out) {
  __shared__ Fq sA[PAIRING_WG][6];
  __shared__ Fq sB[PAIRING_WG][6];
  __shared__ Fq sL[PAIRING_WG][3];
  const int g = threadIdx.x / PAIRING_GROUP, k = threadIdx.x % PAIRING_GROUP;
  size_t slot = (size_t)blockIdx.x * PAIRING_WG + g;
  const bool live = slot < n;
  if (!live) slot = n - 1;
  if (k < 6) {
    sA[g][k] = fp_from_abi<FqParams>(a + slot * 72 + k * 12);
    sB[g][k] = fp_from_abi<FqParams>(b + slot * 72 + k * 12);
    if (k == 0 || k == 3 || k == 4) sL[g][k == 0 ? 0 : k - 2] = sB[g][k];
  }
  __syncthreads();
  if (live && k < 6) {
    const Fq r = op == 0 ? fq6_mul_coeff(k, sA[g], sB[g]) : op == 1 ? fq6_mul_coeff(k, sA[g], sA[g]) : fq6_mul_line_coeff(k, sA[g], sL[g]);
    fp_to_abi<FqParams>(r, out + slot * 72 + k * 12);
  }
}

// ---- checked batches: encoding, curve and order of every point (pairing.cuh point_check), one lane per point.
// key == 0, the staged chunk of pairing_verify_batch: lane t checks element t % 3 of proof t / 3 - A (first G1 slot), B (first G2 slot),
// C (fourth G1 slot) - and A's lane also compares the proof's inputs with r.  codes: four bytes per proof (A, B, C, inputs); the
// kernels behind read them as one word, non-zero = flagged.
// key == 1, a verification key: g1 holds alpha | beta | delta | ABC_0 .., point 1 and 2 are G2's; codes: one byte per point.
__global__ void __launch_bounds__(64) k_point_check(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2, const uint64_t* __restrict__ inputs,
                                                    size_t n_inputs, size_t total, int key, const uint64_t* __restrict__ r_order,
                                                    uint8_t* __restrict__ codes) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  if (key) {
    codes[t] = (uint8_t)point_check(g1 + t * 24, t == 1 || t == 2, r_order);
    return;
  }
  const size_t j = t / 3;
  const int e = (int)(t % 3);
  if (e == 0) codes[j * 4 + 3] = (uint8_t)inputs_check(inputs + j * n_inputs * 6, n_inputs);
  const uint64_t* p = e == 1 ? g2 + j * 4 * 24 : g1 + (j * 4 + (e == 2 ? 3 : 0)) * 24;
  codes[j * 4 + e] = (uint8_t)point_check(p, e == 1, r_order);
}

// ---- acc = ABC_0 + sum x_i ABC_i.  The key's points in device form: x, y (27 limbs each) and an infinity flag.
struct AbcDev {
  Fq x, y;
  uint32_t inf;
};
__global__ void __launch_bounds__(64) k_abc_prep(const uint64_t* __restrict__ abc, size_t n, AbcDev* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t nz = 0;
  for (int k = 0; k < 24; k++) nz |= abc[i * 24 + k];
  out[i].x = fp_from_abi<FqParams>(abc + i * 24);
  out[i].y = fp_from_abi<FqParams>(abc + i * 24 + 12);
  out[i].inf = nz == 0;
}

// one lane per (proof, input): x_i ABC_i by double-and-add over the scalar's 377 bits, most significant first (the scalar is shifted
// through its twelve words, so no word is ever picked by a run-time index).  terms[t] = (X, Y, ZZ, ZZZ), 4 x 27 limbs.
__global__ void __launch_bounds__(64) k_acc_terms(const uint64_t* __restrict__ inputs, const AbcDev* __restrict__ abc, size_t n_inputs, size_t total,
                                                  XYZZ* __restrict__ terms, const uint32_t* __restrict__ flags /* per proof, or null */) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  if (flags && flags[t / n_inputs]) {              // a flagged proof: its inputs are zeros, its terms the point at infinity
    terms[t] = xyzz_infinity();
    return;
  }
  const AbcDev* base = abc + 1 + t % n_inputs;
  uint32_t w[12];
  fp_abi_to_canonical_words<FrParams>(inputs + t * 6, w);
  const Fq bx = base->x, by = base->y;
  const bool binf = base->inf != 0;
  constexpr int SKIP = 384 - FrParams::NBITS;               // bring bit NBITS - 1 to the top of the twelve words
#pragma unroll
  for (int j = 11; j >= 0; j--) w[j] = (w[j] << SKIP) | (j ? w[j - 1] >> (32 - SKIP) : 0u);
  XYZZ acc = xyzz_infinity();
#pragma unroll 1
  for (int b = 0; b < FrParams::NBITS; b++) {
    acc = xyzz_dbl(acc);
    const bool bit = (w[11] >> 31) != 0;
#pragma unroll
    for (int j = 11; j >= 0; j--) w[j] = (w[j] << 1) | (j ? w[j - 1] >> 31 : 0u);
    if (bit && !binf) xyzz_madd(acc, bx, by);
  }
  terms[t] = acc;
}

// one lane per proof: ABC_0 + the proof's terms, to affine with one inversion, ABI limbs into the product's second G1 slot
__global__ void __launch_bounds__(64) k_acc_sum(const XYZZ* __restrict__ terms, const AbcDev* __restrict__ abc, size_t n_inputs, size_t count,
                                                uint64_t* __restrict__ g1 /* count x 4 x 24 */, const uint32_t* __restrict__ flags /* per proof, or null */) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  if (flags && flags[j]) {                         // a flagged proof: acc is the point at infinity
    for (int k = 0; k < 24; k++) g1[(j * 4 + 1) * 24 + k] = 0;
    return;
  }
  XYZZ acc = abc[0].inf ? xyzz_infinity() : xyzz_from_affine(abc[0].x, abc[0].y);
#pragma unroll 1
  for (size_t i = 0; i < n_inputs; i++) {
    const XYZZ tm = terms[j * n_inputs + i];
    xyzz_add(acc, tm);
  }
  uint64_t* o = g1 + (j * 4 + 1) * 24;
  if (xyzz_is_inf(acc)) {
    for (int k = 0; k < 24; k++) o[k] = 0;
    return;
  }
  const Fq zi = fp_inv<FqParams>(fp_mul(acc.ZZ, acc.ZZZ));  // 1 / (ZZ ZZZ)
  const Fq x = fp_mul(acc.X, fp_mul(zi, acc.ZZZ));          // X / ZZ
  const Fq y = fp_mul(acc.Y, fp_mul(zi, acc.ZZ));           // Y / ZZZ
  fp_to_abi<FqParams>(x, o);
  fp_to_abi<FqParams>(y, o + 12);
}

// ---- combined batches (pairing_host.hpp states the equation): rho_i A_i and rho_i C_i, then two reduction trees.
// One lane per (proof, element): lanes 0 .. count - 1 scale A, the next count scale C, so a wave does one kind of work.  A's lane
// writes rho A as affine ABI limbs into pair i's G1 slot (all zero for a result at infinity: k_pair_prep then marks the pair as
// contributing 1); C's lane keeps XYZZ for k_g1_sum.  g1: the staged chunk of pairing_verify_batch, A in the first and C in the fourth
// of a proof's four slots.  A flagged proof (checked route) is the point at infinity in both places.
__global__ void __launch_bounds__(64) k_rho_scale(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ rho, size_t count,
                                                  uint64_t* __restrict__ ra /* count x 24 */, XYZZ* __restrict__ rc,
                                                  const uint32_t* __restrict__ flags /* per proof, or null */) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * count) return;
  const size_t j = t < count ? t : t - count;
  const bool is_c = t >= count;
  if (flags && flags[j]) {
    if (is_c) rc[j] = xyzz_infinity();
    else for (int k = 0; k < 24; k++) ra[j * 24 + k] = 0;
    return;
  }
  const XYZZ v = rho_scale(g1 + (j * 4 + (is_c ? 3 : 0)) * 24, rho + j * 2);
  if (is_c) rc[j] = v;
  else xyzz_to_affine_abi(v, ra + j * 24);
}

// `count` unreduced Miller values -> ceil(count / PAIRING_STRIP) products.  A group of eight lanes owns a strip: six coefficient lanes,
// the running product and the next operand twice in LDS (a product reads one copy of each and writes the other), ONE barrier per
// product - the cut of k_miller.  Groups past the last strip recompute it and store nothing, so every thread reaches every barrier; a
// strip that runs past the end of the values multiplies by one.  abi (the launch that is left with one strip): the product as ABI
// limbs.  in and out are different buffers.
__global__ void __launch_bounds__(PAIRING_BLOCK) k_gt_product(const Fq* __restrict__ in, size_t count, Fq* __restrict__ out,
                                                              uint64_t* __restrict__ abi) {
  __shared__ Fq sF[PAIRING_WG][2][6];
  __shared__ Fq sB[PAIRING_WG][2][6];
  const int g = threadIdx.x / PAIRING_GROUP, k = threadIdx.x % PAIRING_GROUP;
  const size_t strips = (count + PAIRING_STRIP - 1) / PAIRING_STRIP;
  size_t strip = (size_t)blockIdx.x * PAIRING_WG + g;
  const bool live = strip < strips;
  if (!live) strip = strips - 1;
  const size_t first = strip * PAIRING_STRIP;
  if (k < 6) {
    sF[g][0][k] = gt_strip_operand(k, in, first, 0, count);
    sB[g][0][k] = gt_strip_operand(k, in, first, 1, count);
  }
  __syncthreads();
  int cur = 0;
#pragma unroll 1
  for (int i = 1; i < PAIRING_STRIP; i++) {
    if (k < 6) {
      sF[g][cur ^ 1][k] = fq6_mul_coeff(k, sF[g][cur], sB[g][cur]);       // [4] x [4] -> [4]
      if (i + 1 < PAIRING_STRIP) sB[g][cur ^ 1][k] = gt_strip_operand(k, in, first, i + 1, count);
    }
    __syncthreads();
    cur ^= 1;
  }
  if (live && k < 6) {
    if (abi) fp_to_abi<FqParams>(sF[g][cur][k], abi + k * 12);            // [4] -> canonical
    else out[strip * 6 + k] = sF[g][cur][k];
  }
}

// `count` XYZZ values -> ceil(count / PAIRING_STRIP) sums, one lane per strip (pairing.cuh g1_strip_sum).  abi (the launch that is left
// with one strip): the sum as affine ABI limbs, all zero for infinity.  in and out are different buffers.
__global__ void __launch_bounds__(64) k_g1_sum(const XYZZ* __restrict__ in, size_t count, XYZZ* __restrict__ out, uint64_t* __restrict__ abi) {
  const size_t strips = (count + PAIRING_STRIP - 1) / PAIRING_STRIP;
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= strips) return;
  const XYZZ acc = g1_strip_sum(in, s * PAIRING_STRIP, count);
  if (abi) xyzz_to_affine_abi(acc, abi);
  else out[s] = acc;
}

#define PAIR_HIP(x)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) {                                                                           \
      if (errbuf) snprintf(errbuf, errlen, "pairing: %s: %s", #x, hipGetErrorString(e_));             \
      return ZKHIP_ERR_HIP;                                                                           \
    }                                                                                                 \
  } while (0)

namespace {
unsigned blocks_for(size_t n, size_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

int bit_length(const uint64_t* e, int limbs) {
  int top = limbs * 64 - 1;
  while (top > 0 && !((e[top / 64] >> (top % 64)) & 1)) top--;
  return top + 1;
}

// -Q for a point in ABI limbs (infinity stays infinity)
void neg_point(const uint64_t* p, uint64_t* o) {
  using host::HFq;
  memcpy(o, p, 96);
  const HFq y = HFq::from_limbs(p + 12);
  const bool inf = HFq::from_limbs(p).is_zero() && y.is_zero();
  (inf ? y : y.neg()).to_limbs(o + 12);
}
}  // namespace

struct PairingCtx {
  hipStream_t st = nullptr;
  uint64_t* d_const = nullptr;      // r (6), the final exponent (66), 1/4 and -1/4 (24)
  int fe_bits = 0;
  size_t cap = 0;                   // products the work space holds
  uint64_t *d_g1 = nullptr, *d_g2 = nullptr, *d_gt = nullptr;
  MillerConst* d_pairs = nullptr;
  uint32_t* d_inf = nullptr;
  Fq* d_f = nullptr;
  uint8_t* d_codes = nullptr;       // checked batches: four codes per proof (k_point_check), one word per proof as the flag array
  // verifier handles
  bool has_key = false;
  bool checked = false;             // the key passed k_point_check (pairing_ctx_new with checked set)
  size_t n_inputs = 0;
  AbcDev* d_abc = nullptr;
  uint64_t* d_inputs = nullptr;
  XYZZ* d_terms = nullptr;
  size_t in_cap = 0;
  uint64_t alpha[24], neg_g2[24], neg_beta[24], neg_delta[24];
  std::vector<uint64_t> abc;        // the key's ABC points, ABI limbs (the host finish of a combined batch)
  std::vector<uint64_t> h_g1, h_g2, h_gt;
  std::vector<uint8_t> h_codes;
  // combined batches (pairing_verify_all)
  size_t comb_cap = 0;
  uint64_t *d_rho = nullptr, *d_ra = nullptr, *d_b = nullptr, *d_res = nullptr;   // scalars, rho A and B per pair, the chunk's product | sum
  XYZZ *d_rc = nullptr, *d_rc2 = nullptr;                                         // rho C, and the other buffer of the sum tree
  Fq* d_f2 = nullptr;                                                             // the other buffer of the product tree
  std::vector<uint64_t> h_b;
  double finish_ms = 0;
};

static void ctx_release_work(PairingCtx* c) {
  for (void* p : {(void*)c->d_g1, (void*)c->d_g2, (void*)c->d_gt, (void*)c->d_pairs, (void*)c->d_inf, (void*)c->d_f, (void*)c->d_codes}) if (p) (void)hipFree(p);
  c->d_g1 = c->d_g2 = c->d_gt = nullptr; c->d_pairs = nullptr; c->d_inf = nullptr; c->d_f = nullptr; c->d_codes = nullptr; c->cap = 0;
}

static int ctx_reserve(PairingCtx* c, size_t count, char* errbuf, size_t errlen) {
  if (count <= c->cap) return ZKHIP_OK;
  ctx_release_work(c);
  PAIR_HIP(hipMalloc(&c->d_g1, count * 4 * 24 * 8));
  PAIR_HIP(hipMalloc(&c->d_g2, count * 4 * 24 * 8));
  PAIR_HIP(hipMalloc(&c->d_gt, count * 72 * 8));
  PAIR_HIP(hipMalloc(&c->d_pairs, count * 4 * sizeof(MillerConst)));
  PAIR_HIP(hipMalloc(&c->d_inf, count * 4 * sizeof(uint32_t)));
  PAIR_HIP(hipMalloc(&c->d_f, count * 6 * sizeof(Fq)));
  PAIR_HIP(hipMalloc(&c->d_codes, count * 4));
  c->cap = count;
  return ZKHIP_OK;
}

static void ctx_release_comb(PairingCtx* c) {
  for (void* p : {(void*)c->d_rho, (void*)c->d_ra, (void*)c->d_b, (void*)c->d_res, (void*)c->d_rc, (void*)c->d_rc2, (void*)c->d_f2}) if (p) (void)hipFree(p);
  c->d_rho = c->d_ra = c->d_b = c->d_res = nullptr; c->d_rc = c->d_rc2 = nullptr; c->d_f2 = nullptr; c->comb_cap = 0;
}

static int ctx_reserve_comb(PairingCtx* c, size_t count, char* errbuf, size_t errlen) {
  if (count <= c->comb_cap) return ZKHIP_OK;
  ctx_release_comb(c);
  const size_t strips = (count + PAIRING_STRIP - 1) / PAIRING_STRIP;
  PAIR_HIP(hipMalloc(&c->d_rho, count * 16));
  PAIR_HIP(hipMalloc(&c->d_ra, count * 192));
  PAIR_HIP(hipMalloc(&c->d_b, count * 192));
  PAIR_HIP(hipMalloc(&c->d_res, (72 + 24) * 8));
  PAIR_HIP(hipMalloc(&c->d_rc, count * sizeof(XYZZ)));
  PAIR_HIP(hipMalloc(&c->d_rc2, strips * sizeof(XYZZ)));
  PAIR_HIP(hipMalloc(&c->d_f2, strips * 6 * sizeof(Fq)));
  c->comb_cap = count;
  return ZKHIP_OK;
}

void pairing_ctx_free(PairingCtx* c) {
  if (!c) return;
  ctx_release_work(c);
  ctx_release_comb(c);
  for (void* p : {(void*)c->d_const, (void*)c->d_abc, (void*)c->d_inputs, (void*)c->d_terms}) if (p) (void)hipFree(p);
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

size_t pairing_ctx_num_inputs(const PairingCtx* c) { return c ? c->n_inputs : 0; }
double pairing_ctx_last_finish_ms(const PairingCtx* c) { return c ? c->finish_ms : 0; }
void pairing_ctx_key(const PairingCtx* c, const uint64_t** alpha, const uint64_t** neg_g2, const uint64_t** neg_beta, const uint64_t** neg_delta,
                     const uint64_t** abc) {
  *alpha = c->alpha; *neg_g2 = c->neg_g2; *neg_beta = c->neg_beta; *neg_delta = c->neg_delta; *abc = c->abc.data();
}
bool pairing_ctx_checked(const PairingCtx* c) { return c && c->checked; }

void pairing_key_refusal(size_t element, int code, char* buf, size_t len) {
  static const char* const names[3] = {"alpha", "beta", "delta"};
  const char* what = code == ZKHIP_VERIFY_ENCODING ? "ZKHIP_VERIFY_ENCODING" : code == ZKHIP_VERIFY_OFF_CURVE ? "ZKHIP_VERIFY_OFF_CURVE" : "ZKHIP_VERIFY_NOT_ORDER_R";
  if (element < 3) snprintf(buf, len, "verification key refused: %s: %s (%d)", names[element], what, code);
  else snprintf(buf, len, "verification key refused: ABC[%zu]: %s (%d)", element - 3, what, code);
}

// the key's n_inputs + 4 points through k_point_check, once: ZKHIP_ERR_ARG naming the first element that fails
static int ctx_check_key(PairingCtx* c, const uint64_t* vk_alpha_g1, const uint64_t* vk_beta_g2, const uint64_t* vk_delta_g2, const uint64_t* vk_abc,
                         size_t n_inputs, char* errbuf, size_t errlen) {
  const size_t n = n_inputs + 4;
  std::vector<uint64_t> pts(n * 24);
  memcpy(&pts[0], vk_alpha_g1, 192); memcpy(&pts[24], vk_beta_g2, 192); memcpy(&pts[48], vk_delta_g2, 192);
  memcpy(&pts[72], vk_abc, (n_inputs + 1) * 192);
  std::vector<uint8_t> codes(n);
  uint64_t* d_pts = nullptr;
  uint8_t* d_kc = nullptr;
  hipError_t e = hipMalloc(&d_pts, n * 192);
  if (e == hipSuccess) e = hipMalloc(&d_kc, n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_pts, pts.data(), n * 192, hipMemcpyHostToDevice, c->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_point_check, dim3(blocks_for(n, 64)), dim3(64), 0, c->st, d_pts, nullptr, nullptr, 0, n, 1, c->d_const, d_kc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(codes.data(), d_kc, n, hipMemcpyDeviceToHost, c->st);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st);
  for (void* p : {(void*)d_pts, (void*)d_kc}) if (p) (void)hipFree(p);
  PAIR_HIP(e);
  for (size_t i = 0; i < n; i++) {
    if (!codes[i]) continue;
    if (errbuf) pairing_key_refusal(i, codes[i], errbuf, errlen);
    return ZKHIP_ERR_ARG;
  }
  c->checked = true;
  return ZKHIP_OK;
}

static int ctx_init(PairingCtx* c, const uint64_t* vk_alpha_g1, const uint64_t* vk_beta_g2, const uint64_t* vk_delta_g2, const uint64_t* vk_abc,
                    size_t n_inputs, bool checked, char* errbuf, size_t errlen) {
  using host::HFq;
  PAIR_HIP(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
  uint64_t k[6 + 66 + 24];
  static_assert(FqParams::FINAL_EXP_LIMBS == 66, "");
  memcpy(k, FqParams::R_ORDER64, 48);
  memcpy(k + 6, FqParams::FINAL_EXP, 66 * 8);
  const HFq quarter = HFq::from_u64(4).inv();
  quarter.to_limbs(k + 72);
  quarter.neg().to_limbs(k + 84);
  if (bit_length(FqParams::R_ORDER64, 6) != PAIRING_MILLER_STEPS + 1) {
    if (errbuf) snprintf(errbuf, errlen, "pairing: the group order does not have %d bits", PAIRING_MILLER_STEPS + 1);
    return ZKHIP_ERR_STATE;
  }
  c->fe_bits = bit_length(FqParams::FINAL_EXP, 66);
  PAIR_HIP(hipMalloc(&c->d_const, sizeof k));
  PAIR_HIP(hipMemcpyAsync(c->d_const, k, sizeof k, hipMemcpyHostToDevice, c->st));
  PAIR_HIP(hipStreamSynchronize(c->st));
  if (!vk_alpha_g1) return ZKHIP_OK;
  if (checked) {                                   // before any host or device arithmetic on the key's points
    const int rc = ctx_check_key(c, vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
  }
  c->has_key = true;
  c->n_inputs = n_inputs;
  memcpy(c->alpha, vk_alpha_g1, 192);
  c->abc.assign(vk_abc, vk_abc + (n_inputs + 1) * 24);
  uint64_t g2[24];
  memcpy(g2, FqParams::G2_GEN_X64, 96);
  memcpy(g2 + 12, FqParams::G2_GEN_Y64, 96);
  neg_point(g2, c->neg_g2);
  neg_point(vk_beta_g2, c->neg_beta);
  neg_point(vk_delta_g2, c->neg_delta);
  uint64_t* d_abi = nullptr;
  const size_t bytes = (n_inputs + 1) * 192;
  PAIR_HIP(hipMalloc(&c->d_abc, (n_inputs + 1) * sizeof(AbcDev)));
  PAIR_HIP(hipMalloc(&d_abi, bytes));
  hipError_t e = hipMemcpyAsync(d_abi, vk_abc, bytes, hipMemcpyHostToDevice, c->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_abc_prep, dim3(blocks_for(n_inputs + 1, 64)), dim3(64), 0, c->st, d_abi, n_inputs + 1, c->d_abc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->st);
  (void)hipFree(d_abi);
  PAIR_HIP(e);
  return ZKHIP_OK;
}

int pairing_ctx_new(const uint64_t* vk_alpha_g1, const uint64_t* vk_beta_g2, const uint64_t* vk_delta_g2, const uint64_t* vk_abc, size_t n_inputs,
                    bool checked, PairingCtx** out, char* errbuf, size_t errlen) {
  PairingCtx* c = new PairingCtx();
  const int rc = ctx_init(c, vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs, checked, errbuf, errlen);
  if (rc != ZKHIP_OK) { pairing_ctx_free(c); return rc; }
  *out = c;
  return ZKHIP_OK;
}

// d_g1 / d_g2 hold `count` products of `pairs` pairs: Miller loop, final exponentiation, GT values to the host.
// flags: null, or the checked route's word per product (non-zero: the product's pairs are read as points at infinity); codes_out: null,
// or where the checked route's count x 4 codes go, in the same synchronisation as the GT values
static int run_products(PairingCtx* c, int pairs, size_t count, uint64_t* out, const uint32_t* flags, uint8_t* codes_out, char* errbuf, size_t errlen) {
  const size_t n = count * (size_t)pairs;
  hipLaunchKernelGGL(k_pair_prep, dim3(blocks_for(n, 64)), dim3(64), 0, c->st, c->d_g1, c->d_g2, c->d_const + 72, n, c->d_pairs, c->d_inf, flags,
                     pairs);
  hipLaunchKernelGGL(k_miller, dim3(blocks_for(count, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, c->d_pairs, c->d_inf, pairs, count,
                     c->d_const, c->d_f);
  hipLaunchKernelGGL(k_final_exp, dim3(blocks_for(count, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, c->d_f, c->d_const + 6, c->fe_bits, count,
                     c->d_gt);
  PAIR_HIP(hipGetLastError());
  PAIR_HIP(hipMemcpyAsync(out, c->d_gt, count * 72 * 8, hipMemcpyDeviceToHost, c->st));
  if (codes_out) PAIR_HIP(hipMemcpyAsync(codes_out, c->d_codes, count * 4, hipMemcpyDeviceToHost, c->st));
  PAIR_HIP(hipStreamSynchronize(c->st));
  return ZKHIP_OK;
}

int pairing_products(PairingCtx* c, const uint64_t* g1, const uint64_t* g2, int pairs, size_t count, uint64_t* out, char* errbuf, size_t errlen) {
  for (size_t lo = 0; lo < count; lo += PAIRING_CHUNK) {
    const size_t m = count - lo < PAIRING_CHUNK ? count - lo : PAIRING_CHUNK;
    int rc = ctx_reserve(c, m, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    PAIR_HIP(hipMemcpyAsync(c->d_g1, g1 + lo * pairs * 24, m * pairs * 192, hipMemcpyHostToDevice, c->st));
    PAIR_HIP(hipMemcpyAsync(c->d_g2, g2 + lo * pairs * 24, m * pairs * 192, hipMemcpyHostToDevice, c->st));
    if ((rc = run_products(c, pairs, m, out + lo * 72, nullptr, nullptr, errbuf, errlen)) != ZKHIP_OK) return rc;
  }
  return ZKHIP_OK;
}

// checked == false: ok[i] = 1 / 0.  checked == true: ok[i] is the status byte of zkhip.h (ZKHIP_VERIFY_*), k_point_check runs on the staged
// chunk in front of k_acc_terms and its codes flag the refused proofs for the kernels behind.
int pairing_verify_batch(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, bool checked, uint8_t* ok, char* errbuf,
                         size_t errlen) {
  using host::HFq;
  if (checked && !c->checked) {
    if (errbuf) snprintf(errbuf, errlen, "checked batches need a handle of zkhip_verifier_new_checked");
    return ZKHIP_ERR_STATE;
  }
  const size_t ni = c->n_inputs;
  // the chunk also bounds the terms of a launch: 2^21 of them are 0.9 GB of work space
  size_t chunk = PAIRING_CHUNK;
  if (ni && chunk * ni > ((size_t)1 << 21)) chunk = (((size_t)1 << 21) / ni) ? ((size_t)1 << 21) / ni : 1;
  uint64_t one[72] = {0};
  HFq::one().to_limbs(one);
  for (size_t lo = 0; lo < count; lo += chunk) {
    const size_t m = count - lo < chunk ? count - lo : chunk;
    int rc = ctx_reserve(c, m, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    if (ni && m * ni > c->in_cap) {
      if (c->d_inputs) (void)hipFree(c->d_inputs);
      if (c->d_terms) (void)hipFree(c->d_terms);
      c->d_inputs = nullptr; c->d_terms = nullptr; c->in_cap = 0;
      PAIR_HIP(hipMalloc(&c->d_inputs, m * ni * 48));
      PAIR_HIP(hipMalloc(&c->d_terms, m * ni * sizeof(XYZZ)));
      c->in_cap = m * ni;
    }
    c->h_g1.resize(m * 96); c->h_g2.resize(m * 96); c->h_gt.resize(m * 72);
    for (size_t j = 0; j < m; j++) {
      const uint64_t* pr = proofs + (lo + j) * 72;
      uint64_t* p1 = &c->h_g1[j * 96];
      uint64_t* p2 = &c->h_g2[j * 96];
      memcpy(p1, pr, 192);           memcpy(p2, pr + 24, 192);            // e(A, B)
      memset(p1 + 24, 0, 192);       memcpy(p2 + 24, c->neg_g2, 192);     // e(acc, -g2): k_acc_sum writes acc
      memcpy(p1 + 48, c->alpha, 192); memcpy(p2 + 48, c->neg_beta, 192);  // e(alpha, -beta)
      memcpy(p1 + 72, pr + 48, 192); memcpy(p2 + 72, c->neg_delta, 192);  // e(C, -delta)
    }
    PAIR_HIP(hipMemcpyAsync(c->d_g1, c->h_g1.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
    PAIR_HIP(hipMemcpyAsync(c->d_g2, c->h_g2.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
    const uint32_t* flags = checked ? reinterpret_cast<const uint32_t*>(c->d_codes) : nullptr;
    if (ni) PAIR_HIP(hipMemcpyAsync(c->d_inputs, inputs + lo * ni * 6, m * ni * 48, hipMemcpyHostToDevice, c->st));
    if (checked) {
      c->h_codes.resize(m * 4);
      hipLaunchKernelGGL(k_point_check, dim3(blocks_for(m * 3, 64)), dim3(64), 0, c->st, c->d_g1, c->d_g2, c->d_inputs, ni, m * 3, 0, c->d_const,
                         c->d_codes);
    }
    if (ni) hipLaunchKernelGGL(k_acc_terms, dim3(blocks_for(m * ni, 64)), dim3(64), 0, c->st, c->d_inputs, c->d_abc, ni, m * ni, c->d_terms, flags);
    hipLaunchKernelGGL(k_acc_sum, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_terms, c->d_abc, ni, m, c->d_g1, flags);
    if ((rc = run_products(c, 4, m, c->h_gt.data(), flags, checked ? c->h_codes.data() : nullptr, errbuf, errlen)) != ZKHIP_OK) return rc;
    for (size_t j = 0; j < m; j++) {
      const bool is_one = memcmp(&c->h_gt[j * 72], one, sizeof one) == 0;
      if (!checked) { ok[lo + j] = is_one ? 1 : 0; continue; }
      const uint8_t refused = verify_refusal(&c->h_codes[j * 4]);
      ok[lo + j] = refused ? refused : (uint8_t)(is_one ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_REJECT);
    }
  }
  return ZKHIP_OK;
}

// One random-combination check of the whole batch.  Per chunk the device scales A and C by rho (k_rho_scale), runs the existing
// Miller loop with ONE pair per proof on (rho_i A_i, B_i) and reduces the unreduced values to one product (k_gt_product) and the
// rho_i C_i to one sum (k_g1_sum), relaunched until one value is left; the host multiplies and adds the chunks' results, forms the
// sums in Fr while the device works (checked route: once the codes are back, over the proofs nothing refuses), and finishes with the
// three shared pairs and ONE final exponentiation (pairing_host.hpp combined_value).
int pairing_verify_all(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                       uint8_t* status, uint64_t* value, char* errbuf, size_t errlen) {
  using namespace host;
  if ((checked || status) && !c->checked) {
    if (errbuf) snprintf(errbuf, errlen, "a per-proof status needs a handle of zkhip_verifier_new_checked");
    return ZKHIP_ERR_STATE;
  }
  const size_t ni = c->n_inputs;
  CombineSums sums(ni);
  Fq6 product = Fq6::one();
  HJac s_c = HJac::infinity();
  auto add_sums = [&](size_t lo, size_t m, const uint8_t* codes) {
    for (size_t j = 0; j < m; j++)
      if (!codes || !verify_refusal(codes + j * 4)) sums.add(rho + (lo + j) * 2, inputs + (lo + j) * ni * 6);
  };
  for (size_t lo = 0; lo < count; lo += PAIRING_CHUNK) {
    const size_t m = count - lo < PAIRING_CHUNK ? count - lo : PAIRING_CHUNK;
    int rc = ctx_reserve(c, m, errbuf, errlen);
    if (rc == ZKHIP_OK) rc = ctx_reserve_comb(c, m, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    // the staged chunk has the layout of pairing_verify_batch (k_point_check reads it): A and C in the first and the fourth G1 slot
    c->h_g1.resize(m * 96); c->h_b.resize(m * 24);
    if (checked) c->h_g2.resize(m * 96);
    for (size_t j = 0; j < m; j++) {
      const uint64_t* pr = proofs + (lo + j) * 72;
      memcpy(&c->h_g1[j * 96], pr, 192);
      memcpy(&c->h_g1[j * 96 + 72], pr + 48, 192);
      memcpy(&c->h_b[j * 24], pr + 24, 192);
      if (checked) memcpy(&c->h_g2[j * 96], pr + 24, 192);
    }
    PAIR_HIP(hipMemcpyAsync(c->d_g1, c->h_g1.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
    PAIR_HIP(hipMemcpyAsync(c->d_b, c->h_b.data(), m * 192, hipMemcpyHostToDevice, c->st));
    PAIR_HIP(hipMemcpyAsync(c->d_rho, rho + lo * 2, m * 16, hipMemcpyHostToDevice, c->st));
    const uint32_t* flags = nullptr;
    if (checked) {
      if (ni && m * ni > c->in_cap) {
        if (c->d_inputs) (void)hipFree(c->d_inputs);
        if (c->d_terms) (void)hipFree(c->d_terms);
        c->d_inputs = nullptr; c->d_terms = nullptr; c->in_cap = 0;
        PAIR_HIP(hipMalloc(&c->d_inputs, m * ni * 48));
        PAIR_HIP(hipMalloc(&c->d_terms, m * ni * sizeof(XYZZ)));
        c->in_cap = m * ni;
      }
      PAIR_HIP(hipMemcpyAsync(c->d_g2, c->h_g2.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
      if (ni) PAIR_HIP(hipMemcpyAsync(c->d_inputs, inputs + lo * ni * 6, m * ni * 48, hipMemcpyHostToDevice, c->st));
      c->h_codes.resize(m * 4);
      hipLaunchKernelGGL(k_point_check, dim3(blocks_for(m * 3, 64)), dim3(64), 0, c->st, c->d_g1, c->d_g2, c->d_inputs, ni, m * 3, 0, c->d_const,
                         c->d_codes);
      flags = reinterpret_cast<const uint32_t*>(c->d_codes);
    }
    hipLaunchKernelGGL(k_rho_scale, dim3(blocks_for(2 * m, 64)), dim3(64), 0, c->st, c->d_g1, c->d_rho, m, c->d_ra, c->d_rc, flags);
    hipLaunchKernelGGL(k_pair_prep, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_ra, c->d_b, c->d_const + 72, m, c->d_pairs, c->d_inf, flags, 1);
    hipLaunchKernelGGL(k_miller, dim3(blocks_for(m, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, c->d_pairs, c->d_inf, 1, m, c->d_const, c->d_f);
    {
      const Fq* in = c->d_f;
      Fq* out = c->d_f2;
      for (size_t n = m;;) {
        const size_t strips = (n + PAIRING_STRIP - 1) / PAIRING_STRIP;
        hipLaunchKernelGGL(k_gt_product, dim3(blocks_for(strips, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, in, n, out,
                           strips == 1 ? c->d_res : nullptr);
        if (strips == 1) break;
        n = strips;
        Fq* t = const_cast<Fq*>(in); in = out; out = t;      // the values of the level before are dead: their buffer takes the next level
      }
    }
    {
      const XYZZ* in = c->d_rc;
      XYZZ* out = c->d_rc2;
      for (size_t n = m;;) {
        const size_t strips = (n + PAIRING_STRIP - 1) / PAIRING_STRIP;
        hipLaunchKernelGGL(k_g1_sum, dim3(blocks_for(strips, 64)), dim3(64), 0, c->st, in, n, out, strips == 1 ? c->d_res + 72 : nullptr);
        if (strips == 1) break;
        n = strips;
        XYZZ* t = const_cast<XYZZ*>(in); in = out; out = t;
      }
    }
    PAIR_HIP(hipGetLastError());
    uint64_t res[72 + 24];
    PAIR_HIP(hipMemcpyAsync(res, c->d_res, sizeof res, hipMemcpyDeviceToHost, c->st));
    if (checked) PAIR_HIP(hipMemcpyAsync(c->h_codes.data(), c->d_codes, m * 4, hipMemcpyDeviceToHost, c->st));
    if (!checked) add_sums(lo, m, nullptr);
    PAIR_HIP(hipStreamSynchronize(c->st));
    if (checked) {
      add_sums(lo, m, c->h_codes.data());
      if (status) for (size_t j = 0; j < m; j++) status[lo + j] = verify_refusal(&c->h_codes[j * 4]);
    }
    product = product * fq6_from_limbs(res);
    s_c = s_c.add(jac_from_limbs(res + 72));
  }
  const auto t0 = std::chrono::steady_clock::now();
  const CombineKey key = {c->alpha, c->neg_g2, c->neg_beta, c->neg_delta, c->abc.data(), ni};
  fq6_to_limbs(combined_value(key, sums, s_c, product), value);
  c->finish_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ZKHIP_OK;
}

int pairing_fq6_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, char* errbuf, size_t errlen) {
  uint64_t *da = nullptr, *db = nullptr, *dr = nullptr;
  hipError_t e = hipMalloc(&da, n * 576);
  if (e == hipSuccess) e = hipMalloc(&db, n * 576);
  if (e == hipSuccess) e = hipMalloc(&dr, n * 576);
  if (e == hipSuccess) e = hipMemcpy(da, a, n * 576, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(db, b, n * 576, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fq6_selftest, dim3(blocks_for(n, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, 0, op, da, db, n, dr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dr, n * 576, hipMemcpyDeviceToHost);
  for (void* p : {(void*)da, (void*)db, (void*)dr}) if (p) (void)hipFree(p);
  PAIR_HIP(e);
  return ZKHIP_OK;
}

}  // namespace zkhip
