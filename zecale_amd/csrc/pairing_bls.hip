// Nested (BLS12-377) Groth16 verification in batches on the device: the optimal-ate pairing of circuit/bls12_377.hpp (the reference's
// nsnark::verify, libzecale/tests/circuits/dummy_application_test.cpp:32-44) as kernels over the lane bodies of pairing_bls.cuh.
//
// A verification owns a GROUP of sixteen lanes (pairing_bls.cuh explains the cut); a workgroup of 128 threads holds 8 of them, a wave 4.
// The group's state lives in LDS: the accumulator twice (an operation reads one copy and writes the other, so ONE barrier separates
// two operations) and the lines of the four pairs; the final exponentiation keeps eight Fq12 registers there.  Every loop has a fixed
// trip count (the 63 bits of u, the program's length); the only synchronisation is the workgroup barrier, which every thread of a
// workgroup reaches the same number of times: groups past the end of the batch recompute the last verification and store nothing.
// No waits, no spins, no atomics.
//
// In front run the one-lane-per-proof kernels without LDS or barriers: k_nested_prep (curve checks of A, B, C - a lane leaves at its
// first failure - and the 69 lines of B) and k_nested_acc (acc = ABC_0 + sum x_i ABC_i along the host's chain).  They write one status
// byte each per proof; a proof with a status continues on stand-in values and the host ignores its product.
//
// Checked batches put k_nested_point_check in front: one lane per proof point (encoding, curve, [r] P = O) and per proof's inputs, no
// LDS and no barrier, so a lane leaves at its first failure.  It writes one code per element; a proof with any code set is REFUSED:
// k_nested_prep_checked (in k_nested_prep's place) converts none of its limbs and gives it the stand-ins of an off-curve proof, and its
// status byte comes from the codes alone.  The unchecked route launches what it always launched.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "device_buffer.hpp"
#include "pairing_bls.cuh"
#include "pairing_bls.h"

namespace zkhip {

constexpr int NESTED_BLOCK = 128;
constexpr int NESTED_WG = NESTED_BLOCK / NESTED_GROUP;      // verifications per workgroup
constexpr size_t NESTED_CHUNK = 8192;                       // verifications per launch sequence (bounds the work space: 15.5 KB of lines each)

// where the pairs of a product find their G1 point (x, y in device form) and their lines: base + slot * stride (strides in elements;
// zero for what the key shares among all proofs)
struct NestedMillerArgs {
  const Fr* g1[NESTED_MAX_PAIRS];
  size_t g1_stride[NESTED_MAX_PAIRS];
  const NestedLine* lines[NESTED_MAX_PAIRS];
  size_t line_stride[NESTED_MAX_PAIRS];
  const NestedLine* standin;            // pair 0's lines for a slot whose own were never written (status NESTED_OFF_CURVE), or null
  const uint8_t* status;
};

// ---- ABI limbs -> device form, one lane per element (keys, constants, the G1 points of a product)
__global__ void __launch_bounds__(64) k_nested_from_abi(const uint64_t* __restrict__ in, size_t n, Fr* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fp_from_abi<FrParams>(in + i * 6);
}

// ---- the lines of one G2 point per lane (products); status: NESTED_DEGENERATE when a denominator of its schedule is zero
__global__ void __launch_bounds__(64) k_nested_g2_lines(const uint64_t* __restrict__ g2, size_t n, NestedLine* __restrict__ lines,
                                                        uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t* q = g2 + i * 24;
  const Fr2 qx{fp_from_abi<FrParams>(q), fp_from_abi<FrParams>(q + 6)}, qy{fp_from_abi<FrParams>(q + 12), fp_from_abi<FrParams>(q + 18)};
  status[i] = g2_lines_lane(qx, qy, lines + i * NESTED_LINES) ? 0 : NESTED_DEGENERATE;
}

// ---- one lane per proof (a | b | c, 48 ABI limbs): A and C to device form (slots 0 and 2 of the proof's three G1 points), the curve
// checks, the lines of B.  consts[12] is -1/5.
__global__ void __launch_bounds__(64) k_nested_prep(const uint64_t* __restrict__ proofs, size_t count, const Fr* __restrict__ consts,
                                                    Fr* __restrict__ g1 /* count x 3 x 2 */, NestedLine* __restrict__ lines,
                                                    uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t* pr = proofs + i * 48;
  const Fr ax = fp_from_abi<FrParams>(pr), ay = fp_from_abi<FrParams>(pr + 6);
  const Fr cx = fp_from_abi<FrParams>(pr + 36), cy = fp_from_abi<FrParams>(pr + 42);
  g1[i * 6 + 0] = ax; g1[i * 6 + 1] = ay;
  g1[i * 6 + 4] = cx; g1[i * 6 + 5] = cy;
  if (!nested_g1_on_curve(ax, ay)) { status[i] = NESTED_OFF_CURVE; return; }
  const Fr2 bx{fp_from_abi<FrParams>(pr + 12), fp_from_abi<FrParams>(pr + 18)}, by{fp_from_abi<FrParams>(pr + 24), fp_from_abi<FrParams>(pr + 30)};
  if (!nested_g2_on_curve(bx, by, consts[12])) { status[i] = NESTED_OFF_CURVE; return; }
  if (!nested_g1_on_curve(cx, cy)) { status[i] = NESTED_OFF_CURVE; return; }
  status[i] = g2_lines_lane(bx, by, lines + i * NESTED_LINES) ? 0 : NESTED_DEGENERATE;
}

// ---- checked batches: encoding, curve and order of every proof point, one lane per point (pairing_bls.cuh nested_point_check), and
// the inputs, one lane per proof.  No LDS, no barrier, no atomics; a lane leaves at its first failure.  Lanes [0, count) take the B
// points, [count, 3 count) the A and C points (proof (t - count) / 2), [3 count, 4 count) the inputs: a wave holds one kind of point
// but for the two at the seams, so it runs the Fr2 body or the Fr body and not both in turn.  codes: four bytes per proof (A, B, C,
// inputs).  consts[12] is -1/5.
__global__ void __launch_bounds__(64) k_nested_point_check(const uint64_t* __restrict__ proofs, const uint64_t* __restrict__ inputs, size_t n_inputs,
                                                           size_t count, const Fr* __restrict__ consts, uint8_t* __restrict__ codes) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 4 * count) return;
  if (t < count) {
    codes[t * 4 + 1] = (uint8_t)nested_point_check(proofs + t * 48 + 12, true, consts[12]);
  } else if (t < 3 * count) {
    const size_t j = (t - count) >> 1;
    const bool c = ((t - count) & 1) != 0;
    codes[j * 4 + (c ? 2 : 0)] = (uint8_t)nested_point_check(proofs + j * 48 + (c ? 36 : 0), false, consts[12]);
  } else {
    const size_t j = t - 3 * count;
    codes[j * 4 + 3] = (uint8_t)nested_inputs_check(inputs + j * n_inputs * 6, n_inputs);
  }
}

// ---- k_nested_prep behind k_nested_point_check: a proof with a code set is REFUSED - none of its limbs is converted, its G1 slots get
// the key's alpha (a valid point) and its status NESTED_OFF_CURVE, which makes the Miller loop read the stand-in lines for its B.  The
// others passed the curve checks already: device form and the lines of B.
__global__ void __launch_bounds__(64) k_nested_prep_checked(const uint64_t* __restrict__ proofs, size_t count, const uint32_t* __restrict__ codes,
                                                            const Fr* __restrict__ standin /* x, y */, Fr* __restrict__ g1, NestedLine* __restrict__ lines,
                                                            uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if (codes[i] != 0) {
    g1[i * 6 + 0] = standin[0]; g1[i * 6 + 1] = standin[1];
    g1[i * 6 + 4] = standin[0]; g1[i * 6 + 5] = standin[1];
    status[i] = NESTED_OFF_CURVE;
    return;
  }
  const uint64_t* pr = proofs + i * 48;
  g1[i * 6 + 0] = fp_from_abi<FrParams>(pr); g1[i * 6 + 1] = fp_from_abi<FrParams>(pr + 6);
  g1[i * 6 + 4] = fp_from_abi<FrParams>(pr + 36); g1[i * 6 + 5] = fp_from_abi<FrParams>(pr + 42);
  const Fr2 bx{fp_from_abi<FrParams>(pr + 12), fp_from_abi<FrParams>(pr + 18)}, by{fp_from_abi<FrParams>(pr + 24), fp_from_abi<FrParams>(pr + 30)};
  status[i] = g2_lines_lane(bx, by, lines + i * NESTED_LINES) ? 0 : NESTED_DEGENERATE;
}

// ---- one lane per proof: the input accumulator into slot 1 of the proof's G1 points; its own status byte
__global__ void __launch_bounds__(64) k_nested_acc(const uint64_t* __restrict__ inputs, size_t n_inputs, size_t count, const Fr* __restrict__ abc0,
                                                   const Fr* __restrict__ chain, Fr* __restrict__ g1, uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  Fr out[2];
  const bool fine = nested_acc_lane(abc0, chain, inputs + i * n_inputs * 6, n_inputs, out);
  g1[i * 6 + 2] = out[0]; g1[i * 6 + 3] = out[1];
  status[i] = fine ? 0 : NESTED_DEGENERATE;
}

// ---- f = prod_p f_{u,Q_p}(P_p): multi_miller_loop over precomputed lines, `np` pairs per product
__global__ void __launch_bounds__(NESTED_BLOCK) k_nested_miller(NestedMillerArgs args, int np, size_t count, Fr* __restrict__ f_out) {
  __shared__ Fr sF[NESTED_WG][2][12];
  __shared__ Fr sL[NESTED_WG][NESTED_MAX_PAIRS][5];
  const int g = threadIdx.x / NESTED_GROUP, k = threadIdx.x % NESTED_GROUP;
  size_t slot = (size_t)blockIdx.x * NESTED_WG + g;
  const bool live = slot < count;
  if (!live) slot = count - 1;
  const int p = k - 12;                                     // lanes 12 .. 15 prepare the lines of pair p
  const bool ln = p >= 0 && p < np;
  const NestedLine* lines = nullptr;
  Fr px = fp_zero<FrParams>(), py = fp_zero<FrParams>();
  if (ln) {
    lines = args.lines[p] + slot * args.line_stride[p];
    if (p == 0 && args.standin && (args.status[slot] & NESTED_OFF_CURVE)) lines = args.standin;
    const Fr* pt = args.g1[p] + slot * args.g1_stride[p];
    px = pt[0]; py = pt[1];
  }
  if (k < 12) sF[g][0][k] = k == 0 ? fp_one<FrParams>() : fp_zero<FrParams>();
  __syncthreads();
  int cur = 0, at = 0;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
#pragma unroll 1
    for (int add = 0; add < 2; add++) {
      if (add && !((NESTED_U >> i) & 1)) break;             // the same bit for every thread
      // the accumulator's squaring on the coefficient lanes and the pairs' lines on lanes 12 .. 15 touch disjoint state
      if (!add && k < 12) sF[g][cur ^ 1][k] = fq12_mul_coeff(k, sF[g][cur], sF[g][cur]);
      if (ln) nested_line_at(lines[at], px, py, sL[g][p]);
      __syncthreads();
      if (!add) cur ^= 1;
#pragma unroll 1
      for (int q = 0; q < np; q++) {                        // f <- f * line_q: read copy `cur`, write the other, barrier
        if (k < 12) sF[g][cur ^ 1][k] = fq12_mul_line_coeff(k, sF[g][cur], sL[g][q]);
        __syncthreads();
        cur ^= 1;
      }
      at++;
    }
  }
  if (live && k < 12) f_out[slot * 12 + k] = sF[g][cur][k];
}

// ---- f^(3 (q^12 - 1) / r): the program of pairing_bls.cuh over eight Fq12 registers in LDS, then ABI limbs
__global__ void __launch_bounds__(NESTED_BLOCK) k_nested_final_exp(const Fr* __restrict__ f_in, const Fq12Op* __restrict__ prog, int n_ops,
                                                                   const Fr* __restrict__ frob, size_t count, uint64_t* __restrict__ gt) {
  __shared__ Fr sR[NESTED_WG][FQ12_REGS][12];
  const int g = threadIdx.x / NESTED_GROUP, k = threadIdx.x % NESTED_GROUP;
  size_t slot = (size_t)blockIdx.x * NESTED_WG + g;
  const bool live = slot < count;
  if (!live) slot = count - 1;
  if (k < 12) sR[g][0][k] = f_in[slot * 12 + k];
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < n_ops; i++) {
    const Fq12Op o = prog[i];                               // the same operation for every thread
    if (k < 12) fq12_op_lane(o, k, sR[g], frob);
    __syncthreads();
  }
  if (live && k < 12) fp_to_abi<FrParams>(sR[g][0][k], gt + slot * 72 + k * 6);       // [8] -> canonical
}

// ---- combined batches (nested_combine_host.hpp states the equation): rho_i A_i and rho_i C_i, then two reduction trees.
// One lane per (proof, element): lanes 0 .. count - 1 scale A, the next count scale C, so a wave does one kind of work.  A's lane writes
// rho A affine, in device form, over A in the proof's first G1 slot (the pair's point in the Miller loop) and the proof's skip byte:
// set when the prep left a status (off its curve or refused, a degenerate line schedule) or when rho A is the point at infinity - the
// pair then contributes one, the slot keeps A.  C's lane keeps XYZZ for k_nested_g1_sum: infinity for a proof with a status.
__global__ void __launch_bounds__(64) k_nested_rho_scale(Fr* __restrict__ g1 /* count x 3 x 2 */, const uint64_t* __restrict__ rho, size_t count,
                                                         const uint8_t* __restrict__ status, NestedXYZZ<Fr>* __restrict__ rc,
                                                         uint8_t* __restrict__ skip) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * count) return;
  const bool is_c = t >= count;
  const size_t j = is_c ? t - count : t;
  if (status[j] != 0) {
    if (is_c) rc[j] = nested_xyzz_infinity<Fr>();
    else skip[j] = 1;
    return;
  }
  Fr* pt = g1 + j * 6 + (is_c ? 4 : 0);
  const NestedXYZZ<Fr> v = nested_rho_scale(pt[0], pt[1], rho + j * 2);
  if (is_c) { rc[j] = v; return; }
  const bool inf = nf_is_zero_2p(v.ZZ);
  skip[j] = inf ? 1 : 0;
  if (!inf) nested_xyzz_to_affine(v, pt);
}

// `count` unreduced Miller values -> ceil(count / NESTED_STRIP) products.  A group of sixteen lanes owns a strip: twelve coefficient
// lanes, the running product and the next operand twice in LDS (a product reads one copy of each and writes the other), ONE barrier per
// product - the cut of k_nested_miller.  Groups past the last strip recompute it and store nothing, so every thread reaches every
// barrier; a strip that runs past the end of the values, or a value that `skip` flags (first level only), multiplies by one.  abi (the
// launch that is left with one strip): the product as ABI limbs.  in and out are different buffers.
__global__ void __launch_bounds__(NESTED_BLOCK) k_nested_gt_product(const Fr* __restrict__ in, size_t count, const uint8_t* __restrict__ skip,
                                                                    Fr* __restrict__ out, uint64_t* __restrict__ abi) {
  __shared__ Fr sF[NESTED_WG][2][12];
  __shared__ Fr sB[NESTED_WG][2][12];
  const int g = threadIdx.x / NESTED_GROUP, k = threadIdx.x % NESTED_GROUP;
  const size_t strips = nested_strips(count);
  size_t strip = (size_t)blockIdx.x * NESTED_WG + g;
  const bool live = strip < strips;
  if (!live) strip = strips - 1;
  const size_t first = strip * NESTED_STRIP;
  if (k < 12) {
    sF[g][0][k] = nested_gt_strip_operand(k, in, first, 0, count, skip);
    sB[g][0][k] = nested_gt_strip_operand(k, in, first, 1, count, skip);
  }
  __syncthreads();
  int cur = 0;
#pragma unroll 1
  for (int i = 1; i < NESTED_STRIP; i++) {
    if (k < 12) {
      sF[g][cur ^ 1][k] = fq12_mul_coeff(k, sF[g][cur], sB[g][cur]);        // [8] x [8] -> [8]
      if (i + 1 < NESTED_STRIP) sB[g][cur ^ 1][k] = nested_gt_strip_operand(k, in, first, i + 1, count, skip);
    }
    __syncthreads();
    cur ^= 1;
  }
  if (live && k < 12) {
    if (abi) fp_to_abi<FrParams>(sF[g][cur][k], abi + k * 6);               // [8] -> canonical
    else out[strip * 12 + k] = sF[g][cur][k];
  }
}

// `count` XYZZ values -> ceil(count / NESTED_STRIP) sums, one lane per strip (pairing_bls.cuh nested_g1_strip_sum).  abi (the launch
// that is left with one strip): the sum as affine ABI limbs, all zero for infinity.  in and out are different buffers.
__global__ void __launch_bounds__(64) k_nested_g1_sum(const NestedXYZZ<Fr>* __restrict__ in, size_t count, NestedXYZZ<Fr>* __restrict__ out,
                                                      uint64_t* __restrict__ abi) {
  const size_t strips = nested_strips(count);
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= strips) return;
  const NestedXYZZ<Fr> acc = nested_g1_strip_sum(in, s * NESTED_STRIP, count);
  if (abi) nested_xyzz_to_affine_abi(acc, abi);
  else out[s] = acc;
}

// ---- the lane bodies on operands given as ABI limbs (zkhip_internal_fq12_selftest)
__global__ void __launch_bounds__(NESTED_BLOCK) k_fq12_selftest(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t n,
                                                                uint64_t* __restrict__ out) {
  __shared__ Fr sA[NESTED_WG][12];
  __shared__ Fr sB[NESTED_WG][12];
  __shared__ Fr sL[NESTED_WG][5];
  const int g = threadIdx.x / NESTED_GROUP, k = threadIdx.x % NESTED_GROUP;
  size_t slot = (size_t)blockIdx.x * NESTED_WG + g;
  const bool live = slot < n;
  if (!live) slot = n - 1;
  if (k < 12) {
    sA[g][k] = fp_from_abi<FrParams>(a + slot * 72 + k * 6);
    sB[g][k] = fp_from_abi<FrParams>(b + slot * 72 + k * 6);
    const int li = k == 0 ? 0 : k == 1 ? 1 : k == 3 ? 2 : k == 7 ? 3 : k == 9 ? 4 : -1;
    if (li >= 0) sL[g][li] = sB[g][k];
  }
  __syncthreads();
  if (live && k < 12) {
    const Fr r = op == 0 ? fq12_mul_coeff(k, sA[g], sB[g]) : op == 1 ? fq12_mul_coeff(k, sA[g], sA[g]) : fq12_mul_line_coeff(k, sA[g], sL[g]);
    fp_to_abi<FrParams>(r, out + slot * 72 + k * 6);
  }
}

// the constants and the key on the device, in elements of d_fr
constexpr size_t NK_FROB = 0, NK_FIFTH = 12, NK_ALPHA = 13, NK_ABC0 = 15, NK_LINES = 17, NK_CHAIN = NK_LINES + 3 * NESTED_LINES * 4;

struct NestedCtx {
  DeviceStream st;                            // in front of the buffers: destroyed behind them
  DeviceBuffer<Fr> d_fr;                      // constants, then the key (NK_*)
  DeviceBuffer<Fq12Op> d_prog;
  int n_ops = 0;
  bool has_key = false;
  size_t n_inputs = 0;
  // the work space of a chunk (nctx_reserve)
  DeviceBuffer<uint64_t> d_in1, d_in2, d_gt;  // staged ABI limbs: proofs or G1 points / inputs or G2 points; GT values
  DeviceBuffer<Fr> d_g1, d_f;
  DeviceBuffer<NestedLine> d_lines;
  DeviceBuffer<uint8_t> d_status;             // four per product: per proof of a chunk of m at [0, m) and [m, 2 m) (prep, accumulator); per G2 point (products)
  DeviceBuffer<uint8_t> d_codes;              // checked batches: four codes per proof (k_nested_point_check), read as one word per proof behind it
  std::vector<uint64_t> h_gt;
  std::vector<uint8_t> h_status, h_codes;
  // combined batches (nctx_reserve_comb: reserved only when nested_verify_all runs)
  DeviceBuffer<uint64_t> d_rho, d_res;        // the chunk's scalars; its product (72 limbs) | its sum (12 limbs)
  DeviceBuffer<NestedXYZZ<Fr>> d_rc, d_rc2;   // rho C, and the other buffer of the sum tree
  DeviceBuffer<Fr> d_f2;                      // the other buffer of the product tree (d_f is the first)
  DeviceBuffer<uint8_t> d_skip;               // one byte per proof: its pair contributes one
};

// work space for `count` products of four pairs (a proof is one): 4 G2 points of 24 limbs or a proof's 48; 16 inputs of 6 limbs at most;
// the codes only for a checked batch
static int nctx_reserve(NestedCtx* c, size_t count, bool checked, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("nested pairing", c->d_in1.reserve(count * 48));
  ZK_HIP_TRY("nested pairing", c->d_in2.reserve(count * 96));
  ZK_HIP_TRY("nested pairing", c->d_gt.reserve(count * 72));
  ZK_HIP_TRY("nested pairing", c->d_g1.reserve(count * 8));
  ZK_HIP_TRY("nested pairing", c->d_f.reserve(count * 12));
  ZK_HIP_TRY("nested pairing", c->d_lines.reserve(count * 4 * NESTED_LINES));
  ZK_HIP_TRY("nested pairing", c->d_status.reserve(count * 4));
  if (checked) ZK_HIP_TRY("nested pairing", c->d_codes.reserve(count * 4));
  return ZKHIP_OK;
}

// the combined route's extra work space for a chunk of `count` proofs: scalars, scaled points and the trees' second buffers
static int nctx_reserve_comb(NestedCtx* c, size_t count, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("nested pairing", c->d_rho.reserve(count * 2));
  ZK_HIP_TRY("nested pairing", c->d_res.reserve(72 + 12));
  ZK_HIP_TRY("nested pairing", c->d_rc.reserve(count));
  ZK_HIP_TRY("nested pairing", c->d_rc2.reserve(nested_strips(count)));
  ZK_HIP_TRY("nested pairing", c->d_f2.reserve(nested_strips(count) * 12));
  ZK_HIP_TRY("nested pairing", c->d_skip.reserve(count));
  return ZKHIP_OK;
}

void nested_ctx_free(NestedCtx* c) { delete c; }       // every buffer, then the stream

size_t nested_ctx_num_inputs(const NestedCtx* c) { return c ? c->n_inputs : 0; }

static int nctx_init(NestedCtx* c, const NestedKeyData* key, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("nested pairing", c->st.create());
  const bool has_key = key->alpha != nullptr;
  const size_t n = has_key ? NK_CHAIN + key->n_inputs * NESTED_INPUT_BITS_DEV * 2 : NK_ALPHA;
  std::vector<uint64_t> abi(n * 6);
  memcpy(&abi[NK_FROB * 6], key->frob, 12 * 48);
  memcpy(&abi[NK_FIFTH * 6], key->fifth_neg, 48);
  if (has_key) {
    memcpy(&abi[NK_ALPHA * 6], key->alpha, 96);
    memcpy(&abi[NK_ABC0 * 6], key->abc0, 96);
    memcpy(&abi[NK_LINES * 6], key->lines, (size_t)3 * NESTED_LINES * 4 * 48);
    if (key->n_inputs) memcpy(&abi[NK_CHAIN * 6], key->chain, key->n_inputs * NESTED_INPUT_BITS_DEV * 2 * 48);
  }
  const std::vector<Fq12Op> prog = fq12_final_exp_program();
  c->n_ops = (int)prog.size();
  DeviceBuffer<uint64_t> d_abi;
  ZK_HIP_TRY("nested pairing", c->d_fr.reserve(n));
  ZK_HIP_TRY("nested pairing", c->d_prog.reserve(prog.size()));
  ZK_HIP_TRY("nested pairing", d_abi.reserve(n * 6));
  ZK_HIP_TRY("nested pairing", hipMemcpyAsync(d_abi, abi.data(), n * 48, hipMemcpyHostToDevice, c->st));
  ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_prog, prog.data(), prog.size() * sizeof(Fq12Op), hipMemcpyHostToDevice, c->st));
  hipLaunchKernelGGL(k_nested_from_abi, dim3(blocks_for(n, 64)), dim3(64), 0, c->st, d_abi.get(), n, c->d_fr.get());
  ZK_HIP_TRY("nested pairing", hipGetLastError());
  ZK_HIP_TRY("nested pairing", hipStreamSynchronize(c->st));       // (abi and prog are read by the copies until here)
  c->has_key = has_key;
  c->n_inputs = has_key ? key->n_inputs : 0;
  return ZKHIP_OK;
}

int nested_ctx_new(const NestedKeyData* key, NestedCtx** out, char* errbuf, size_t errlen) {
  NestedCtx* c = new NestedCtx();
  const int rc = nctx_init(c, key, errbuf, errlen);
  if (rc != ZKHIP_OK) { nested_ctx_free(c); return rc; }
  *out = c;
  return ZKHIP_OK;
}

// Miller loop and final exponentiation of `count` products, GT values and `n_status` status bytes to the host
static int nested_run(NestedCtx* c, const NestedMillerArgs& args, int pairs, size_t count, uint64_t* out, size_t n_status, char* errbuf, size_t errlen) {
  hipLaunchKernelGGL(k_nested_miller, dim3(blocks_for(count, NESTED_WG)), dim3(NESTED_BLOCK), 0, c->st, args, pairs, count, c->d_f.get());
  hipLaunchKernelGGL(k_nested_final_exp, dim3(blocks_for(count, NESTED_WG)), dim3(NESTED_BLOCK), 0, c->st, c->d_f.get(), c->d_prog.get(), c->n_ops,
                     c->d_fr + NK_FROB, count, c->d_gt.get());
  ZK_HIP_TRY("nested pairing", hipGetLastError());
  c->h_status.resize(n_status);
  ZK_HIP_TRY("nested pairing", hipMemcpyAsync(out, c->d_gt, count * 72 * 8, hipMemcpyDeviceToHost, c->st));
  ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->h_status.data(), c->d_status, n_status, hipMemcpyDeviceToHost, c->st));
  ZK_HIP_TRY("nested pairing", hipStreamSynchronize(c->st));
  return ZKHIP_OK;
}

int nested_products(NestedCtx* c, const uint64_t* g1, const uint64_t* g2, int pairs, size_t count, uint64_t* out, uint8_t* status, char* errbuf,
                    size_t errlen) {
  return for_each_chunk(count, NESTED_CHUNK, [&](size_t lo, size_t m) -> int {
    const size_t n = m * (size_t)pairs;
    int rc = nctx_reserve(c, m, false, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_in1, g1 + lo * pairs * 12, n * 96, hipMemcpyHostToDevice, c->st));
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_in2, g2 + lo * pairs * 24, n * 192, hipMemcpyHostToDevice, c->st));
    hipLaunchKernelGGL(k_nested_from_abi, dim3(blocks_for(n * 2, 64)), dim3(64), 0, c->st, c->d_in1.get(), n * 2, c->d_g1.get());
    hipLaunchKernelGGL(k_nested_g2_lines, dim3(blocks_for(n, 64)), dim3(64), 0, c->st, c->d_in2.get(), n, c->d_lines.get(), c->d_status.get());
    NestedMillerArgs args = {};
    for (int p = 0; p < pairs; p++) {
      args.g1[p] = c->d_g1 + p * 2; args.g1_stride[p] = (size_t)pairs * 2;
      args.lines[p] = c->d_lines + (size_t)p * NESTED_LINES; args.line_stride[p] = (size_t)pairs * NESTED_LINES;
    }
    if ((rc = nested_run(c, args, pairs, m, out + lo * 72, n, errbuf, errlen)) != ZKHIP_OK) return rc;
    for (size_t j = 0; j < m; j++) {
      uint8_t s = 0;
      for (int p = 0; p < pairs; p++) s |= c->h_status[j * pairs + p];
      status[lo + j] = s;
    }
    return ZKHIP_OK;
  });
}

// checked: k_nested_point_check runs on the staged chunk in front, k_nested_prep_checked takes k_nested_prep's place, and ok[i] is the
// status byte of zkhip.h; a refused proof has status[i] = 0 (it is decided: nothing of it goes to the host).  Unchecked: the launches
// and results of before.
int nested_verify_batch(NestedCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, bool checked, uint8_t* ok, uint8_t* status,
                        char* errbuf, size_t errlen) {
  if (!c->has_key) {
    if (errbuf) snprintf(errbuf, errlen, "nested pairing: a context without a key");
    return ZKHIP_ERR_STATE;
  }
  const size_t ni = c->n_inputs;
  uint64_t one[72] = {0};
  memcpy(one, FrParams::ONE64, 48);
  const NestedLine* key_lines = reinterpret_cast<const NestedLine*>(c->d_fr + NK_LINES);
  return for_each_chunk(count, NESTED_CHUNK, [&](size_t lo, size_t m) -> int {
    int rc = nctx_reserve(c, m, checked, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_in1, proofs + lo * 48, m * 48 * 8, hipMemcpyHostToDevice, c->st));
    if (ni) ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_in2, inputs + lo * ni * 6, m * ni * 48, hipMemcpyHostToDevice, c->st));
    if (checked) {
      hipLaunchKernelGGL(k_nested_point_check, dim3(blocks_for(4 * m, 64)), dim3(64), 0, c->st, c->d_in1.get(), c->d_in2.get(), ni, m, c->d_fr.get(),
                         c->d_codes.get());
      hipLaunchKernelGGL(k_nested_prep_checked, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_in1.get(), m,
                         reinterpret_cast<const uint32_t*>(c->d_codes.get()), c->d_fr + NK_ALPHA, c->d_g1.get(), c->d_lines.get(), c->d_status.get());
      c->h_codes.resize(m * 4);
      ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->h_codes.data(), c->d_codes, m * 4, hipMemcpyDeviceToHost, c->st));     // (nested_run synchronises)
    } else {
      hipLaunchKernelGGL(k_nested_prep, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_in1.get(), m, c->d_fr.get(), c->d_g1.get(), c->d_lines.get(),
                         c->d_status.get());
    }
    hipLaunchKernelGGL(k_nested_acc, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_in2.get(), ni, m, c->d_fr + NK_ABC0, c->d_fr + NK_CHAIN,
                       c->d_g1.get(), c->d_status + m);
    NestedMillerArgs args = {};
    args.g1[0] = c->d_g1;     args.g1_stride[0] = 6; args.lines[0] = c->d_lines;                    args.line_stride[0] = NESTED_LINES;   // e(A, B)
    args.g1[1] = c->d_g1 + 2; args.g1_stride[1] = 6; args.lines[1] = key_lines + 2 * NESTED_LINES;  args.line_stride[1] = 0;              // e(acc, -g2)
    args.g1[2] = c->d_fr + NK_ALPHA; args.g1_stride[2] = 0; args.lines[2] = key_lines;              args.line_stride[2] = 0;              // e(alpha, -beta)
    args.g1[3] = c->d_g1 + 4; args.g1_stride[3] = 6; args.lines[3] = key_lines + NESTED_LINES;      args.line_stride[3] = 0;              // e(C, -delta)
    args.standin = key_lines;
    args.status = c->d_status;
    c->h_gt.resize(m * 72);
    if ((rc = nested_run(c, args, 4, m, c->h_gt.data(), 2 * m, errbuf, errlen)) != ZKHIP_OK) return rc;
    for (size_t j = 0; j < m; j++) {
      const uint8_t prep = c->h_status[j];
      const uint8_t s = (prep & NESTED_OFF_CURVE) ? NESTED_OFF_CURVE : (uint8_t)(prep | c->h_status[m + j]);
      const bool is_one = memcmp(&c->h_gt[j * 72], one, sizeof one) == 0;
      if (!checked) {
        status[lo + j] = s;
        ok[lo + j] = (s == 0 && is_one) ? 1 : 0;
        continue;
      }
      const uint8_t refused = verify_refusal(&c->h_codes[j * 4]);
      status[lo + j] = refused ? 0 : s;
      ok[lo + j] = refused ? refused : (uint8_t)(is_one ? ZKHIP_VERIFY_ACCEPT : ZKHIP_VERIFY_REJECT);
    }
    return ZKHIP_OK;
  });
}

size_t nested_verify_all_chunks(size_t count) { return (count + NESTED_CHUNK - 1) / NESTED_CHUNK; }

// One random-combination check of the whole batch, the device's share.  Per chunk: the staging and the prep kernel of the per-proof
// route (k_nested_point_check in front when checked), k_nested_rho_scale, the existing Miller loop with ONE pair per proof on
// (rho_i A_i, B_i), and the two trees, relaunched on their partial results - two buffers taking turns - until one value is left.  The
// input accumulator (k_nested_acc, the key's chains) is not touched.  The host finish is the caller's (nested_combine_host.hpp).
int nested_verify_all(NestedCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                      uint64_t* chunk_products, uint64_t* chunk_sums, uint8_t* left_out, uint8_t* refusal, char* errbuf, size_t errlen) {
  if (!c->has_key) {
    if (errbuf) snprintf(errbuf, errlen, "nested pairing: a context without a key");
    return ZKHIP_ERR_STATE;
  }
  const size_t ni = c->n_inputs;
  const NestedLine* key_lines = reinterpret_cast<const NestedLine*>(c->d_fr + NK_LINES);
  return for_each_chunk(count, NESTED_CHUNK, [&](size_t lo, size_t m) -> int {
    int rc = nctx_reserve(c, m, checked, errbuf, errlen);
    if (rc == ZKHIP_OK) rc = nctx_reserve_comb(c, m, errbuf, errlen);
    if (rc != ZKHIP_OK) return rc;
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_in1, proofs + lo * 48, m * 48 * 8, hipMemcpyHostToDevice, c->st));
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_rho, rho + lo * 2, m * 16, hipMemcpyHostToDevice, c->st));
    if (checked) {
      if (ni) ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->d_in2, inputs + lo * ni * 6, m * ni * 48, hipMemcpyHostToDevice, c->st));
      hipLaunchKernelGGL(k_nested_point_check, dim3(blocks_for(4 * m, 64)), dim3(64), 0, c->st, c->d_in1.get(), c->d_in2.get(), ni, m, c->d_fr.get(),
                         c->d_codes.get());
      hipLaunchKernelGGL(k_nested_prep_checked, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_in1.get(), m,
                         reinterpret_cast<const uint32_t*>(c->d_codes.get()), c->d_fr + NK_ALPHA, c->d_g1.get(), c->d_lines.get(), c->d_status.get());
    } else {
      hipLaunchKernelGGL(k_nested_prep, dim3(blocks_for(m, 64)), dim3(64), 0, c->st, c->d_in1.get(), m, c->d_fr.get(), c->d_g1.get(), c->d_lines.get(),
                         c->d_status.get());
    }
    hipLaunchKernelGGL(k_nested_rho_scale, dim3(blocks_for(2 * m, 64)), dim3(64), 0, c->st, c->d_g1.get(), c->d_rho.get(), m, c->d_status.get(),
                       c->d_rc.get(), c->d_skip.get());
    NestedMillerArgs args = {};
    args.g1[0] = c->d_g1; args.g1_stride[0] = 6; args.lines[0] = c->d_lines; args.line_stride[0] = NESTED_LINES;              // f(rho A, B)
    args.standin = key_lines;
    args.status = c->d_status;
    hipLaunchKernelGGL(k_nested_miller, dim3(blocks_for(m, NESTED_WG)), dim3(NESTED_BLOCK), 0, c->st, args, 1, m, c->d_f.get());
    {
      const Fr* in = c->d_f;
      Fr* out = c->d_f2;
      const uint8_t* skip = c->d_skip;
      for (size_t n = m;;) {
        const size_t strips = nested_strips(n);
        hipLaunchKernelGGL(k_nested_gt_product, dim3(blocks_for(strips, NESTED_WG)), dim3(NESTED_BLOCK), 0, c->st, in, n, skip, out,
                           strips == 1 ? c->d_res.get() : nullptr);
        if (strips == 1) break;
        n = strips;
        skip = nullptr;
        Fr* t = const_cast<Fr*>(in); in = out; out = t;       // the values of the level before are dead: their buffer takes the next level
      }
    }
    {
      const NestedXYZZ<Fr>* in = c->d_rc;
      NestedXYZZ<Fr>* out = c->d_rc2;
      for (size_t n = m;;) {
        const size_t strips = nested_strips(n);
        hipLaunchKernelGGL(k_nested_g1_sum, dim3(blocks_for(strips, 64)), dim3(64), 0, c->st, in, n, out, strips == 1 ? c->d_res + 72 : nullptr);
        if (strips == 1) break;
        n = strips;
        NestedXYZZ<Fr>* t = const_cast<NestedXYZZ<Fr>*>(in); in = out; out = t;
      }
    }
    ZK_HIP_TRY("nested pairing", hipGetLastError());
    const size_t chunk = lo / NESTED_CHUNK;
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(chunk_products + chunk * 72, c->d_res, 72 * 8, hipMemcpyDeviceToHost, c->st));
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(chunk_sums + chunk * 12, c->d_res + 72, 12 * 8, hipMemcpyDeviceToHost, c->st));
    ZK_HIP_TRY("nested pairing", hipMemcpyAsync(left_out + lo, c->d_status, m, hipMemcpyDeviceToHost, c->st));
    if (checked) {
      c->h_codes.resize(m * 4);
      ZK_HIP_TRY("nested pairing", hipMemcpyAsync(c->h_codes.data(), c->d_codes, m * 4, hipMemcpyDeviceToHost, c->st));
    }
    ZK_HIP_TRY("nested pairing", hipStreamSynchronize(c->st));
    if (checked && refusal) for (size_t j = 0; j < m; j++) refusal[lo + j] = verify_refusal(&c->h_codes[j * 4]);
    return ZKHIP_OK;
  });
}

int nested_fq12_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, char* errbuf, size_t errlen) {
  ZK_HIP_TRY("nested pairing", selftest_launch(k_fq12_selftest, NESTED_WG, NESTED_BLOCK, op, a, b, n, out));
  return ZKHIP_OK;
}

}  // namespace zkhip
