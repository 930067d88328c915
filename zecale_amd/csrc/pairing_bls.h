// Internal interface of the nested (BLS12-377) pairing engine (pairing_bls.hip).  The public C ABI is include/zkhip.h; the host
// arithmetic that prepares a key (curve checks, lines, doubling chains) lives with the C ABI in api_nested_verify.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkhip.h"

namespace zkhip {

// A stream and the device work space of one batch in flight, plus (verifier handles) the prepared key: everything a
// zkhip_nested_verifier owns.  Lives on the device that was current when it was made; the caller binds its thread first.
struct NestedCtx;

// Everything in ABI limbs (6 per field element), host memory.  Without a key (alpha null) the context serves nested_products only.
struct NestedKeyData {
  const uint64_t* frob;        // 12 elements: tower.hpp Fq12Consts::frob
  const uint64_t* fifth_neg;   // -1/5: the twist's coefficient 1/u = -(1/5) u
  const uint64_t* alpha;       // 2 elements, or null
  const uint64_t* abc0;        // 2 elements
  const uint64_t* lines;       // 3 x 69 x 4 elements: the lines (lambda'_0, lambda'_1, b_0, b_1) of -beta, -delta and the negated generator
  const uint64_t* chain;       // n_inputs x 253 x 2 elements: 2^j ABC_i, i = 1 .. n_inputs
  size_t n_inputs;
};
int nested_ctx_new(const NestedKeyData* key, NestedCtx** out, char* errbuf, size_t errlen);
void nested_ctx_free(NestedCtx* c);
size_t nested_ctx_num_inputs(const NestedCtx* c);

// status bits of a proof (nested_verify_batch) or of a product (nested_products)
constexpr uint8_t NESTED_OFF_CURVE = 1;      // a proof point is off its curve: verdict 0
constexpr uint8_t NESTED_DEGENERATE = 2;     // a chord-and-tangent step of the host route is degenerate for it: not decided here

// out[i] = prod_{p < pairs} e(g1[i][p], g2[i][p]), reduced, 12 x 6 ABI limbs.  g1: 12 limbs per point, g2: 24.  pairs in 1 .. 4; every point on
// its curve.  status[i]: NESTED_DEGENERATE when the schedule of one of its G2 points is (out[i] is then meaningless).
int nested_products(NestedCtx* c, const uint64_t* g1, const uint64_t* g2, int pairs, size_t count, uint64_t* out, uint8_t* status, char* errbuf,
                    size_t errlen);
// ok[i] = e(A_i, B_i) e(acc_i, -g2) e(alpha, -beta) e(C_i, -delta) == 1 where status[i] is 0; 0 where it is NESTED_OFF_CURVE; undecided
// where it has NESTED_DEGENERATE.  proofs: count x 48 limbs, inputs: count x n_inputs x 6.
// checked: every proof point and input is validated on the device first and ok[i] is the status byte of zkhip.h (ZKHIP_VERIFY_*); where
// it names a refusal status[i] is 0, where status[i] has NESTED_DEGENERATE ok[i] is undecided as before.
int nested_verify_batch(NestedCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, bool checked, uint8_t* ok, uint8_t* status,
                        char* errbuf, size_t errlen);
// ONE random-combination check of the whole batch, the device's share (nested_combine_host.hpp states the equation and holds the host
// finish).  rho: count x 2 words, none zero.  Per chunk of NESTED_CHUNK proofs (nested_verify_all_chunks of them): chunk_products gets
// 72 ABI limbs, the UNREDUCED prod_i f(rho_i A_i, B_i) over the chunk's proofs that are not left out, and chunk_sums 12 ABI limbs, the
// affine sum of their rho_i C_i (all zero: infinity).  left_out[i] (count bytes): 0, or the status bits of a proof that is left out -
// NESTED_OFF_CURVE (a point off its curve; on the checked route a refused proof) or NESTED_DEGENERATE (the line schedule of its B).
// A proof with rho_i A_i = O contributes one to the product and is NOT left out.  checked: k_nested_point_check runs in front and
// refusal (count bytes, or null) gets the refusal byte of zkhip.h, 0 for a proof nothing refuses.
int nested_verify_all(NestedCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                      uint64_t* chunk_products, uint64_t* chunk_sums, uint8_t* left_out, uint8_t* refusal, char* errbuf, size_t errlen);
size_t nested_verify_all_chunks(size_t count);
// op 0: a b, 1: a^2, 2: a (b0 + b1 w + b3 w^3 + b7 w^7 + b9 w^9) through the lane bodies of pairing_bls.cuh; a, b, out: n x 72 ABI limbs
int nested_fq12_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, char* errbuf, size_t errlen);

}  // namespace zkhip
