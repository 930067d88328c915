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
#include <memory>
#include <utility>
#include <vector>

#include "device_buffer.hpp"
#include "ec.cuh"
#include "fp_inv.cuh"
#include "host_field.hpp"
#include "pairing.cuh"
#include "pairing.h"
#include "pairing_host.hpp"
#include "pairing_locate.hpp"

namespace zkhip {

constexpr int PAIRING_BLOCK = 128;
constexpr int PAIRING_WG = PAIRING_BLOCK / PAIRING_GROUP;      // verifications per workgroup
// (PAIRING_STRIP, the strip of the combined batches' reduction trees, PAIRING_CHUNK and the rules of the chunk loops are pairing.cuh's:
// the lane bodies and the host shim read them too)

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

// ---- located batches: the values of `count` tree nodes as ABI limbs, 96 per node: the unreduced product (6 x 12, as the last
// k_gt_product launch writes it) and the sum as an affine point (24, all zero for infinity, as the last k_g1_sum launch).  The host
// names each node by where its values lie in the retained buffers.  A group of eight lanes owns a node, the cut of the kernels
// above: six coefficient lanes reduce one coefficient each, the seventh inverts for the point, the eighth idles.  No LDS, no barrier;
// a round has a few hundred nodes at the most, so the launch is latency, and the lanes of one node write 768 contiguous bytes.
struct TreeNodeRef {
  const Fq* f;         // six coefficients [4]
  const XYZZ* c;       // X [10], Y [4]
};
__global__ void __launch_bounds__(64) k_tree_nodes_abi(const TreeNodeRef* __restrict__ refs, size_t count, uint64_t* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t node = t / PAIRING_GROUP;
  const int k = (int)(t % PAIRING_GROUP);
  if (node >= count) return;
  const TreeNodeRef r = refs[node];
  if (k < 6) fp_to_abi<FqParams>(r.f[k], out + node * 96 + k * 12);         // [4] -> canonical
  else if (k == 6) xyzz_to_affine_abi(*r.c, out + node * 96 + 72);
}

namespace {
int bit_length(const uint64_t* e, int limbs) {
  int top = limbs * 64 - 1;
  while (top > 0 && !((e[top / 64] >> (top % 64)) & 1)) top--;
  return top + 1;
}
}  // namespace

struct PairingCtx {
  DeviceStream st;                            // in front of the buffers: destroyed behind them
  DeviceBuffer<uint64_t> d_const;             // r (6), the final exponent (66), 1/4 and -1/4 (24)
  int fe_bits = 0;
  // the work space of a chunk (reserve_chunk)
  DeviceBuffer<uint64_t> d_g1, d_g2, d_gt;
  DeviceBuffer<MillerConst> d_pairs;
  DeviceBuffer<uint32_t> d_inf;
  DeviceBuffer<Fq> d_f;
  DeviceBuffer<uint8_t> d_codes;              // checked batches: four codes per proof (k_point_check), one word per proof as the flag array
  // verifier handles
  bool has_key = false;
  bool checked = false;                       // the key passed k_point_check (pairing_ctx_new with checked set)
  size_t n_inputs = 0;
  DeviceBuffer<AbcDev> d_abc;
  DeviceBuffer<uint64_t> d_inputs;
  DeviceBuffer<XYZZ> d_terms;
  uint64_t alpha[24], neg_g2[24], neg_beta[24], neg_delta[24];
  std::vector<uint64_t> abc;                  // the key's ABC points, ABI limbs (the host finish of a combined batch)
  std::vector<uint64_t> h_g1, h_g2, h_gt;
  std::vector<uint8_t> h_codes;
  // combined batches (pairing_verify_all)
  DeviceBuffer<uint64_t> d_rho, d_ra, d_b, d_res;   // scalars, rho A and B per pair, the chunk's product | sum
  DeviceBuffer<XYZZ> d_rc, d_rc2;                   // rho C, and the other buffer of the sum tree
  DeviceBuffer<Fq> d_f2;                            // the other buffer of the product tree
  std::vector<uint64_t> h_b;
  double finish_ms = 0;
  // located batches (pairing_verify_located): every level of a chunk's two trees, chunk after chunk of the batch in flight
  struct KeptTrees {
    DeviceBuffer<Fq> f;                             // pairing_tree_nodes(m) x 6 coefficients
    DeviceBuffer<XYZZ> c;                           // pairing_tree_nodes(m)
  };
  std::vector<std::unique_ptr<KeptTrees>> kept;
  DeviceBuffer<TreeNodeRef> d_refs;                 // the nodes of a round and their values (k_tree_nodes_abi)
  DeviceBuffer<uint64_t> d_nodes;
};

void pairing_ctx_free(PairingCtx* c) { delete c; }     // every buffer, then the stream

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
  DeviceBuffer<uint64_t> d_pts;
  DeviceBuffer<uint8_t> d_kc;
  hipError_t e = d_pts.reserve(n * 24);
  if (e == hipSuccess) e = d_kc.reserve(n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_pts, pts.data(), n * 192, hipMemcpyHostToDevice, c->st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_point_check, dim3(blocks_for(n, 64)), dim3(64), 0, c->st, d_pts.get(), nullptr, nullptr, 0, n, 1, c->d_const.get(), d_kc.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(codes.data(), d_kc, n, hipMemcpyDeviceToHost, c->st);
  if (e == hipSuccess) e = hipStreamSynchronize(c->st);
  ZK_HIP_TRY("pairing", e);
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
  ZK_HIP_TRY("pairing", c->st.create());
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
  ZK_HIP_TRY("pairing", c->d_const.reserve(sizeof k / 8));
  ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_const, k, sizeof k, hipMemcpyHostToDevice, c->st));
  ZK_HIP_TRY("pairing", hipStreamSynchronize(c->st));
  if (!vk_alpha_g1) return ZKHIP_OK;
  if (checked) {                                   // before any host or device arithmetic on the key's points
    const int rc = ctx_check_key(c, vk_alpha_g1, vk_beta_g2, vk_delta_g2, vk_abc, n_inputs, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
  }
  c->has_key = true;
  c->n_inputs = n_inputs;
  memcpy(c->alpha, vk_alpha_g1, 192);
  c->abc.assign(vk_abc, vk_abc + (n_inputs + 1) * 24);
  host::neg_g2_generator(c->neg_g2);
  host::neg_point_abi(vk_beta_g2, c->neg_beta);
  host::neg_point_abi(vk_delta_g2, c->neg_delta);
  DeviceBuffer<uint64_t> d_abi;
  ZK_HIP_TRY("pairing", c->d_abc.reserve(n_inputs + 1));
  ZK_HIP_TRY("pairing", d_abi.reserve((n_inputs + 1) * 24));
  ZK_HIP_TRY("pairing", hipMemcpyAsync(d_abi, vk_abc, (n_inputs + 1) * 192, hipMemcpyHostToDevice, c->st));
  hipLaunchKernelGGL(k_abc_prep, dim3(blocks_for(n_inputs + 1, 64)), dim3(64), 0, c->st, d_abi.get(), n_inputs + 1, c->d_abc.get());
  ZK_HIP_TRY("pairing", hipGetLastError());
  ZK_HIP_TRY("pairing", hipStreamSynchronize(c->st));
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

// ---- the stages of a chunk.  `combined` is pairing_verify_all's route, `checked` the one with k_point_check in front.

// The work space of a chunk of m products.  The inputs are on the device for k_acc_terms and for k_point_check; only the per-proof
// route has terms, only the combined route its scalars, scaled points and the two buffers of each of its trees.  keep >= 0, the
// located route: the trees of this chunk of the batch go, every level, into retained buffers of their own instead.
static int reserve_chunk(PairingCtx* c, size_t m, bool combined, bool checked, char* errbuf, size_t errlen, int keep = -1) {
  ZK_HIP_TRY("pairing", c->d_g1.reserve(m * 4 * 24));
  ZK_HIP_TRY("pairing", c->d_g2.reserve(m * 4 * 24));
  ZK_HIP_TRY("pairing", c->d_gt.reserve(m * 72));
  ZK_HIP_TRY("pairing", c->d_pairs.reserve(m * 4));
  ZK_HIP_TRY("pairing", c->d_inf.reserve(m * 4));
  if (keep < 0) ZK_HIP_TRY("pairing", c->d_f.reserve(m * 6));      // (a kept chunk's Miller values are level 0 of its retained tree)
  ZK_HIP_TRY("pairing", c->d_codes.reserve(m * 4));
  if (!combined || checked) ZK_HIP_TRY("pairing", c->d_inputs.reserve(m * c->n_inputs * 6));
  if (!combined) {
    ZK_HIP_TRY("pairing", c->d_terms.reserve(m * c->n_inputs));
    return ZKHIP_OK;
  }
  ZK_HIP_TRY("pairing", c->d_rho.reserve(m * 2));
  ZK_HIP_TRY("pairing", c->d_ra.reserve(m * 24));
  ZK_HIP_TRY("pairing", c->d_b.reserve(m * 24));
  if (keep >= 0) {
    while (c->kept.size() <= (size_t)keep) c->kept.emplace_back(new PairingCtx::KeptTrees());
    ZK_HIP_TRY("pairing", c->kept[keep]->f.reserve(pairing_tree_nodes(m) * 6));
    ZK_HIP_TRY("pairing", c->kept[keep]->c.reserve(pairing_tree_nodes(m)));
    return ZKHIP_OK;
  }
  ZK_HIP_TRY("pairing", c->d_res.reserve(72 + 24));
  ZK_HIP_TRY("pairing", c->d_rc.reserve(m));
  ZK_HIP_TRY("pairing", c->d_rc2.reserve(pairing_strips(m)));
  ZK_HIP_TRY("pairing", c->d_f2.reserve(pairing_strips(m) * 6));
  return ZKHIP_OK;
}

// m proofs into the four-slot layout that k_point_check and run_products read: A and C in the first and the fourth G1 slot, B in the
// first G2 slot.  The per-proof route fills the other slots with its three shared pairs; the combined route keeps B apart, one point
// per pair, and needs the G2 slots only for k_point_check (with_g2).
static void stage_chunk(PairingCtx* c, const uint64_t* proofs, size_t m, bool combined, bool with_g2) {
  c->h_g1.resize(m * 96);
  if (with_g2) c->h_g2.resize(m * 96);
  if (combined) c->h_b.resize(m * 24);
  for (size_t j = 0; j < m; j++) {
    const uint64_t* pr = proofs + j * 72;
    uint64_t* p1 = &c->h_g1[j * 96];
    memcpy(p1, pr, 192);                                                  // A
    memcpy(p1 + 72, pr + 48, 192);                                        // C
    if (with_g2) memcpy(&c->h_g2[j * 96], pr + 24, 192);                  // B
    if (combined) {
      memcpy(&c->h_b[j * 24], pr + 24, 192);
      continue;
    }
    uint64_t* p2 = &c->h_g2[j * 96];                                      // e(A, B) and e(C, -delta) stand in slots 0 and 3
    memset(p1 + 24, 0, 192);        memcpy(p2 + 24, c->neg_g2, 192);      // e(acc, -g2): k_acc_sum writes acc
    memcpy(p1 + 48, c->alpha, 192); memcpy(p2 + 48, c->neg_beta, 192);    // e(alpha, -beta)
    memcpy(p2 + 72, c->neg_delta, 192);
  }
}

// the staged G2 slots and the chunk's inputs to the device: what k_point_check reads besides the G1 slots
static int upload_g2_and_inputs(PairingCtx* c, const uint64_t* inputs, size_t m, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_g2, c->h_g2.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
  if (c->n_inputs) ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_inputs, inputs, m * c->n_inputs * 48, hipMemcpyHostToDevice, c->st));
  return ZKHIP_OK;
}

// k_point_check on the staged chunk; its codes, read as one word per proof, are the flags of the kernels behind
static const uint32_t* enqueue_point_check(PairingCtx* c, size_t m) {
  c->h_codes.resize(m * 4);
  hipLaunchKernelGGL(k_point_check, dim3(blocks_for(m * 3, 64)), dim3(64), 0, c->st, c->d_g1.get(), c->d_g2.get(), c->d_inputs.get(), c->n_inputs,
                     m * 3, 0, c->d_const.get(), c->d_codes.get());
  return reinterpret_cast<const uint32_t*>(c->d_codes.get());
}

// A reduction tree over the n values in `a`: launch(in, n_k, out, last) for level after level until one strip is left
// (pairing_tree_levels).  The values of the level before are dead, so their buffer takes the next level: the first level writes b,
// which holds pairing_strips(n) values, the second a, and so on.
template <class T, class Launch>
static void reduce_tree(T* a, T* b, size_t n, Launch launch) {
  for (int k = 0, levels = pairing_tree_levels(n); k < levels; k++, n = pairing_strips(n)) {
    launch(const_cast<const T*>(a), n, b, k + 1 == levels);
    std::swap(a, b);
  }
}

// what came back for a chunk -> ok[j].  Unchecked: 1 / 0.  Checked: the status byte of zkhip.h - what refuses the proof, or the
// pairing's verdict.
static void chunk_verdicts(const PairingCtx* c, size_t m, bool checked, uint8_t* ok) {
  for (size_t j = 0; j < m; j++) {
    const bool is_one = host::gt_is_one(&c->h_gt[j * 72]);
    if (!checked) { ok[j] = is_one ? 1 : 0; continue; }
    const uint8_t refused = verify_refusal(&c->h_codes[j * 4]);
    ok[j] = refused ? refused : (uint8_t)(is_one ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_REJECT);
  }
}

// d_g1 / d_g2 hold `count` products of `pairs` pairs: Miller loop, final exponentiation, GT values to the host.
// flags: null, or the checked route's word per product (non-zero: the product's pairs are read as points at infinity); codes_out: null,
// or where the checked route's count x 4 codes go, in the same synchronisation as the GT values
static int run_products(PairingCtx* c, int pairs, size_t count, uint64_t* out, const uint32_t* flags, uint8_t* codes_out, char* errbuf, size_t errlen) {
  const size_t n = count * (size_t)pairs;
  hipLaunchKernelGGL(k_pair_prep, dim3(blocks_for(n, 64)), dim3(64), 0, c->st, c->d_g1.get(), c->d_g2.get(), c->d_const + 72, n, c->d_pairs.get(),
                     c->d_inf.get(), flags, pairs);
  hipLaunchKernelGGL(k_miller, dim3(blocks_for(count, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, c->d_pairs.get(), c->d_inf.get(), pairs, count,
                     c->d_const.get(), c->d_f.get());
  hipLaunchKernelGGL(k_final_exp, dim3(blocks_for(count, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, c->d_f.get(), c->d_const + 6, c->fe_bits, count,
                     c->d_gt.get());
  ZK_HIP_TRY("pairing", hipGetLastError());
  ZK_HIP_TRY("pairing", hipMemcpyAsync(out, c->d_gt, count * 72 * 8, hipMemcpyDeviceToHost, c->st));
  if (codes_out) ZK_HIP_TRY("pairing", hipMemcpyAsync(codes_out, c->d_codes, count * 4, hipMemcpyDeviceToHost, c->st));
  ZK_HIP_TRY("pairing", hipStreamSynchronize(c->st));
  return ZKHIP_OK;
}

int pairing_products(PairingCtx* c, const uint64_t* g1, const uint64_t* g2, int pairs, size_t count, uint64_t* out, char* errbuf, size_t errlen) {
  return for_each_chunk(count, PAIRING_CHUNK, [&](size_t lo, size_t m) -> int {
    const int rc = reserve_chunk(c, m, false, false, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_g1, g1 + lo * pairs * 24, m * pairs * 192, hipMemcpyHostToDevice, c->st));
    ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_g2, g2 + lo * pairs * 24, m * pairs * 192, hipMemcpyHostToDevice, c->st));
    return run_products(c, pairs, m, out + lo * 72, nullptr, nullptr, errbuf, errlen);
  });
}

// checked == false: ok[i] = 1 / 0.  checked == true: ok[i] is the status byte of zkhip.h (ZKHIP_VERIFY_*), k_point_check runs on the staged
// chunk in front of k_acc_terms and its codes flag the refused proofs for the kernels behind.
int pairing_verify_batch(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, bool checked, uint8_t* ok, char* errbuf,
                         size_t errlen) {
  if (checked && !c->checked) {
    if (errbuf) snprintf(errbuf, errlen, "checked batches need a handle of zkhip_verifier_new_checked");
    return ZKHIP_ERR_STATE;
  }
  const size_t ni = c->n_inputs;
  return for_each_chunk(count, pairing_batch_chunk(ni), [&](size_t lo, size_t m) -> int {
    int rc = reserve_chunk(c, m, false, checked, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    stage_chunk(c, proofs + lo * 72, m, false, true);
    c->h_gt.resize(m * 72);
    ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_g1, c->h_g1.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
    if ((rc = upload_g2_and_inputs(c, inputs + lo * ni * 6, m, errbuf, errlen)) != ZKHIP_OK) return rc;
    const uint32_t* flags = checked ? enqueue_point_check(c, m) : nullptr;
    if (ni) hipLaunchKernelGGL(k_acc_terms, dim3(blocks_for(m * ni, 64)), dim3(64), 0, c->st, c->d_inputs.get(), c->d_abc.get(), ni, m * ni,
                               c->d_terms.get(), flags);
    hipLaunchKernelGGL(k_acc_sum, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_terms.get(), c->d_abc.get(), ni, m, c->d_g1.get(), flags);
    if ((rc = run_products(c, 4, m, c->h_gt.data(), flags, checked ? c->h_codes.data() : nullptr, errbuf, errlen)) != ZKHIP_OK) return rc;
    chunk_verdicts(c, m, checked, ok + lo);
    return ZKHIP_OK;
  });
}

// The front of a combined chunk, up to the values its trees start from: the chunk staged and uploaded, the point checks on the checked
// route, rho A and rho C (k_rho_scale), and the one-pair Miller loop.  f0: m x 6 unreduced Miller values; rc0: m sums' summands.
static int enqueue_combined_leaves(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, const uint64_t* rho, size_t m, bool checked, Fq* f0,
                                   XYZZ* rc0, char* errbuf, size_t errlen) {
  int rc;
  stage_chunk(c, proofs, m, true, checked);
  ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_g1, c->h_g1.data(), m * 96 * 8, hipMemcpyHostToDevice, c->st));
  ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_b, c->h_b.data(), m * 192, hipMemcpyHostToDevice, c->st));
  ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_rho, rho, m * 16, hipMemcpyHostToDevice, c->st));
  if (checked && (rc = upload_g2_and_inputs(c, inputs, m, errbuf, errlen)) != ZKHIP_OK) return rc;
  const uint32_t* flags = checked ? enqueue_point_check(c, m) : nullptr;
  hipLaunchKernelGGL(k_rho_scale, dim3(blocks_for(2 * m, 64)), dim3(64), 0, c->st, c->d_g1.get(), c->d_rho.get(), m, c->d_ra.get(), rc0, flags);
  hipLaunchKernelGGL(k_pair_prep, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_ra.get(), c->d_b.get(), c->d_const + 72, m, c->d_pairs.get(),
                     c->d_inf.get(), flags, 1);
  hipLaunchKernelGGL(k_miller, dim3(blocks_for(m, PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, c->d_pairs.get(), c->d_inf.get(), 1, m,
                     c->d_const.get(), f0);
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
  const int rc_all = for_each_chunk(count, PAIRING_CHUNK, [&](size_t lo, size_t m) -> int {
    int rc = reserve_chunk(c, m, true, checked, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    if ((rc = enqueue_combined_leaves(c, inputs + lo * ni * 6, proofs + lo * 72, rho + lo * 2, m, checked, c->d_f.get(), c->d_rc.get(), errbuf, errlen)) != ZKHIP_OK)
      return rc;
    reduce_tree(c->d_f.get(), c->d_f2.get(), m, [&](const Fq* in, size_t n, Fq* out, bool last) {
      hipLaunchKernelGGL(k_gt_product, dim3(blocks_for(pairing_strips(n), PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, in, n, out,
                         last ? c->d_res.get() : nullptr);
    });
    reduce_tree(c->d_rc.get(), c->d_rc2.get(), m, [&](const XYZZ* in, size_t n, XYZZ* out, bool last) {
      hipLaunchKernelGGL(k_g1_sum, dim3(blocks_for(pairing_strips(n), 64)), dim3(64), 0, c->st, in, n, out, last ? c->d_res + 72 : nullptr);
    });
    ZK_HIP_TRY("pairing", hipGetLastError());
    uint64_t res[72 + 24];
    ZK_HIP_TRY("pairing", hipMemcpyAsync(res, c->d_res, sizeof res, hipMemcpyDeviceToHost, c->st));
    if (checked) ZK_HIP_TRY("pairing", hipMemcpyAsync(c->h_codes.data(), c->d_codes, m * 4, hipMemcpyDeviceToHost, c->st));
    if (!checked) add_sums(lo, m, nullptr);
    ZK_HIP_TRY("pairing", hipStreamSynchronize(c->st));
    if (checked) {
      add_sums(lo, m, c->h_codes.data());
      if (status) for (size_t j = 0; j < m; j++) status[lo + j] = verify_refusal(&c->h_codes[j * 4]);
    }
    product = product * fq6_from_limbs(res);
    s_c = s_c.add(jac_from_limbs(res + 72));
    return ZKHIP_OK;
  });
  if (rc_all != ZKHIP_OK) return rc_all;
  const auto t0 = std::chrono::steady_clock::now();
  const CombineKey key = {c->alpha, c->neg_g2, c->neg_beta, c->neg_delta, c->abc.data(), ni};
  fq6_to_limbs(combined_value(key, sums, s_c, product), value);
  c->finish_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return ZKHIP_OK;
}

// ---- located batches.  The combined check with every level of every chunk's trees retained; a batch that fails is searched from the
// chunk roots down (locate.hpp): a round's nodes come back through k_tree_nodes_abi in one launch and one copy, the host finishes
// each (pairing_locate.hpp test_nodes), and what the cost rule hands over goes through pairing_verify_batch.

// k_tree_nodes_abi on `n` nodes, and their 96 limbs each on the way to `out`; the caller synchronises
static int enqueue_tree_nodes(PairingCtx* c, const TreeNodeRef* refs, size_t n, uint64_t* out, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("pairing", c->d_refs.reserve(n));
  ZK_HIP_TRY("pairing", c->d_nodes.reserve(n * 96));
  ZK_HIP_TRY("pairing", hipMemcpyAsync(c->d_refs, refs, n * sizeof(TreeNodeRef), hipMemcpyHostToDevice, c->st));
  hipLaunchKernelGGL(k_tree_nodes_abi, dim3(blocks_for(n * PAIRING_GROUP, 64)), dim3(64), 0, c->st, c->d_refs.get(), n, c->d_nodes.get());
  ZK_HIP_TRY("pairing", hipGetLastError());
  ZK_HIP_TRY("pairing", hipMemcpyAsync(out, c->d_nodes, n * 96 * 8, hipMemcpyDeviceToHost, c->st));
  return ZKHIP_OK;
}

int pairing_verify_located(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                           uint8_t* verdict, zkhip_locate_stats* stats, uint64_t* value, std::vector<host::LocateTraceNode>* trace, char* errbuf,
                           size_t errlen) {
  using namespace host;
  if (checked && !c->checked) {
    if (errbuf) snprintf(errbuf, errlen, "checked batches need a handle of zkhip_verifier_new_checked");
    return ZKHIP_ERR_STATE;
  }
  if (count > PAIRING_LOCATE_MAX) {
    if (errbuf) snprintf(errbuf, errlen, "a located batch holds at most %zu proofs", PAIRING_LOCATE_MAX);
    return ZKHIP_ERR_ARG;
  }
  const size_t ni = c->n_inputs;
  *stats = zkhip_locate_stats();
  if (trace) trace->clear();
  struct ReleaseKept {               // the retained trees stay until the call returns, on every path, and no longer
    PairingCtx* c;
    ~ReleaseKept() { c->kept.clear(); }
  } release_kept = {c};
  std::vector<size_t> chunks, first;
  std::vector<uint8_t> refused(checked ? count : 0);               // the refusal byte of every proof, 0 where nothing refuses it
  const uint8_t* skip = checked ? refused.data() : nullptr;
  std::vector<CombineSums> sums;                                   // chunk by chunk: a chunk's root is tested with its own
  std::vector<Fq6> root_f;
  std::vector<HJac> root_c;
  const int rc_all = for_each_chunk(count, PAIRING_CHUNK, [&](size_t lo, size_t m) -> int {
    const size_t ci = chunks.size();
    int rc = reserve_chunk(c, m, true, checked, errbuf, errlen, (int)ci);
    if (rc != ZKHIP_OK) return rc;
    Fq* const tf = c->kept[ci]->f.get();
    XYZZ* const tc = c->kept[ci]->c.get();
    if ((rc = enqueue_combined_leaves(c, inputs + lo * ni * 6, proofs + lo * 72, rho + lo * 2, m, checked, tf, tc, errbuf, errlen)) != ZKHIP_OK) return rc;
    size_t n = m;
    for (int k = 0, levels = pairing_tree_levels(m); k < levels; k++, n = pairing_strips(n)) {      // level k -> level k + 1, at its offset
      const size_t in = pairing_level_offset(m, k), out = pairing_level_offset(m, k + 1);
      hipLaunchKernelGGL(k_gt_product, dim3(blocks_for(pairing_strips(n), PAIRING_WG)), dim3(PAIRING_BLOCK), 0, c->st, tf + in * 6, n, tf + out * 6,
                         (uint64_t*)nullptr);
      hipLaunchKernelGGL(k_g1_sum, dim3(blocks_for(pairing_strips(n), 64)), dim3(64), 0, c->st, tc + in, n, tc + out, (uint64_t*)nullptr);
    }
    ZK_HIP_TRY("pairing", hipGetLastError());
    const size_t root = pairing_tree_nodes(m) - 1;
    const TreeNodeRef ref = {tf + root * 6, tc + root};
    uint64_t res[96];
    if ((rc = enqueue_tree_nodes(c, &ref, 1, res, errbuf, errlen)) != ZKHIP_OK) return rc;
    if (checked) ZK_HIP_TRY("pairing", hipMemcpyAsync(c->h_codes.data(), c->d_codes, m * 4, hipMemcpyDeviceToHost, c->st));
    if (!checked) sums.push_back(range_sums(ni, inputs, rho, nullptr, lo, lo + m));
    ZK_HIP_TRY("pairing", hipStreamSynchronize(c->st));
    if (checked) {
      for (size_t j = 0; j < m; j++) refused[lo + j] = verify_refusal(&c->h_codes[j * 4]);
      sums.push_back(range_sums(ni, inputs, rho, skip, lo, lo + m));
    }
    root_f.push_back(fq6_from_limbs(res));
    root_c.push_back(jac_from_limbs(res + 72));
    chunks.push_back(m);
    first.push_back(lo);
    return ZKHIP_OK;
  });
  if (rc_all != ZKHIP_OK) return rc_all;
  auto t0 = std::chrono::steady_clock::now();
  const CombineKey key = {c->alpha, c->neg_g2, c->neg_beta, c->neg_delta, c->abc.data(), ni};
  CombineSums all(ni);
  Fq6 product = Fq6::one();
  HJac s_c = HJac::infinity();
  for (size_t i = 0; i < chunks.size(); i++) {
    all.sigma = all.sigma + sums[i].sigma;
    for (size_t j = 0; j < ni; j++) all.s[j] = all.s[j] + sums[i].s[j];
    product = product * root_f[i];
    s_c = s_c.add(root_c[i]);
  }
  const Fq6 total = combined_value(key, all, s_c, product);
  fq6_to_limbs(total, value);
  c->finish_ms = ms_since(t0);
  const uint8_t accept = checked ? (uint8_t)ZKHIP_VERIFY_ACCEPT : 1, reject = checked ? (uint8_t)ZKHIP_VERIFY_REJECT : 0;
  for (size_t i = 0; i < count; i++) verdict[i] = checked && refused[i] ? refused[i] : accept;
  if (total.is_one()) return ZKHIP_OK;

  t0 = std::chrono::steady_clock::now();
  const unsigned threads = locate_threads();
  const std::vector<uint8_t> known(1, 0);                          // one chunk: the batch's value is its root's, and it is not one
  if (trace && chunks.size() == 1) {
    LocateTraceNode tn;
    tn.node = {0, (uint32_t)pairing_tree_levels(count), 0};
    tn.passed = false;
    fq6_to_limbs(total, tn.value);
    trace->push_back(tn);
  }
  std::vector<uint8_t> state;
  locate::Stats st;
  char* const eb = errbuf;
  const size_t el = errlen;
  const int rc = locate::descend(
      chunks, PAIRING_STRIP, LOCATE_COST, threads, chunks.size() == 1 ? &known : nullptr,
      [&](const std::vector<locate::Node>& nodes, std::vector<uint8_t>& passed) -> int {
        char* errbuf = eb;
        const size_t errlen = el;
        const size_t n = nodes.size();
        std::vector<size_t> lo(n), hi(n);
        std::vector<Fq6> f(n);
        std::vector<HJac> sc(n);
        std::vector<TreeNodeRef> refs(n);
        std::vector<uint64_t> limbs(n * 96);
        bool roots = true;
        for (size_t i = 0; i < n; i++) {
          const locate::Node& nd = nodes[i];
          const size_t m = chunks[nd.chunk];
          if ((int)nd.level > pairing_tree_levels(m) || nd.index >= pairing_level_size(m, (int)nd.level)) {
            if (errbuf) snprintf(errbuf, errlen, "located batch: a node outside its tree");
            return ZKHIP_ERR_STATE;
          }
          node_range(nd, first[nd.chunk], m, &lo[i], &hi[i]);
          const size_t at = pairing_level_offset(m, (int)nd.level) + nd.index;
          refs[i] = {c->kept[nd.chunk]->f.get() + at * 6, c->kept[nd.chunk]->c.get() + at};
          roots = roots && (int)nd.level == pairing_tree_levels(m);
        }
        std::vector<const CombineSums*> given;
        if (roots) {                                               // the chunk round: the roots came back with their chunks, the sums are kept
          for (size_t i = 0; i < n; i++) { f[i] = root_f[nodes[i].chunk]; sc[i] = root_c[nodes[i].chunk]; given.push_back(&sums[nodes[i].chunk]); }
        } else {
          const int r = enqueue_tree_nodes(c, refs.data(), n, limbs.data(), errbuf, errlen);
          if (r != ZKHIP_OK) return r;
          ZK_HIP_TRY("pairing", hipStreamSynchronize(c->st));
          for (size_t i = 0; i < n; i++) { f[i] = fq6_from_limbs(&limbs[i * 96]); sc[i] = jac_from_limbs(&limbs[i * 96 + 72]); }
        }
        test_nodes(key, inputs, rho, skip, nodes, lo, hi, f, sc, threads, passed, trace, given);
        return ZKHIP_OK;
      },
      [&](const std::vector<size_t>& list) -> int {                // the per-proof route on the proofs still in doubt, gathered
        const auto t1 = std::chrono::steady_clock::now();
        int r;
        if (list.back() - list.front() + 1 == list.size()) {      // one run of proofs: they stand gathered where they are
          r = pairing_verify_batch(c, inputs + list.front() * ni * 6, proofs + list.front() * 72, list.size(), checked, verdict + list.front(), eb, el);
        } else {
          std::vector<uint64_t> gi(list.size() * ni * 6), gp(list.size() * 72);
          std::vector<uint8_t> out(list.size());
          for (size_t i = 0; i < list.size(); i++) {
            if (ni) memcpy(&gi[i * ni * 6], inputs + list[i] * ni * 6, ni * 48);
            memcpy(&gp[i * 72], proofs + list[i] * 72, 576);
          }
          r = pairing_verify_batch(c, gi.data(), gp.data(), list.size(), checked, out.data(), eb, el);
          for (size_t i = 0; r == ZKHIP_OK && i < list.size(); i++) verdict[list[i]] = out[i];
        }
        stats->finish_ms = ms_since(t1);
        return r;
      },
      state, st);
  if (rc != ZKHIP_OK) return rc;
  for (size_t i = 0; i < count; i++)
    if (state[i] == locate::INVALID) verdict[i] = reject;
  for (size_t i = 0; i < count; i++) stats->invalid += verdict[i] == reject;
  stats->chunks_failed = st.chunks_failed; stats->rounds = st.rounds; stats->node_tests = st.node_tests; stats->finish_proofs = st.finish_proofs;
  stats->descent_ms = ms_since(t0) - stats->finish_ms;
  return ZKHIP_OK;
}

int pairing_fq6_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("pairing", selftest_launch(k_fq6_selftest, PAIRING_WG, PAIRING_BLOCK, op, a, b, n, out));
  return ZKHIP_OK;
}

}  // namespace zkhip
