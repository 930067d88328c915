// Internal interface of the pairing engine (pairing.hip).  The public C ABI is include/zkhip.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/zkhip.h"

namespace zkhip {
namespace host {
struct LocateTraceNode;      // pairing_locate.hpp
}

// A stream and the device work space of one batch in flight, plus (verifier handles) the key: everything a zkhip_verifier owns.
// Lives on the device that was current when it was made; the caller binds its thread to that device before every call.
struct PairingCtx;

// vk_* null: a context for pairing_products only.  Otherwise the key of zkhip_verifier_new (ABI limbs, host memory).
// checked: the key's n_inputs + 4 points go through the point-check kernel first; ZKHIP_ERR_ARG names the first one that fails.
int pairing_ctx_new(const uint64_t* vk_alpha_g1, const uint64_t* vk_beta_g2, const uint64_t* vk_delta_g2, const uint64_t* vk_abc,
                    size_t n_inputs, bool checked, PairingCtx** out, char* errbuf, size_t errlen);
bool pairing_ctx_checked(const PairingCtx* c);     // made with checked set, and the key passed
// the message of a refused key: element 0, 1, 2 = alpha, beta, delta, 3 + i = ABC[i]; code = ZKHIP_VERIFY_ENCODING, _OFF_CURVE or _NOT_ORDER_R
void pairing_key_refusal(size_t element, int code, char* buf, size_t len);
void pairing_ctx_free(PairingCtx* c);
size_t pairing_ctx_num_inputs(const PairingCtx* c);

// out[i] = prod_{p < pairs} t(g1[i][p], g2[i][p]), reduced GT value, 6 x 12 ABI limbs.  pairs in 1 .. 4.
int pairing_products(PairingCtx* c, const uint64_t* g1, const uint64_t* g2, int pairs, size_t count, uint64_t* out, char* errbuf, size_t errlen);
// ok[i] = e(A_i, B_i) e(acc_i, -g2) e(alpha, -beta) e(C_i, -delta) == 1.  checked (a context whose key was checked, else
// ZKHIP_ERR_STATE): every proof point is validated on the device first and ok[i] is the status byte of zkhip.h (ZKHIP_VERIFY_*).
int pairing_verify_batch(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, bool checked, uint8_t* ok, char* errbuf,
                         size_t errlen);
// ONE random-combination check of the whole batch (pairing_host.hpp states the equation): value = its reduced GT value, 72 ABI limbs,
// one iff the batch passes.  rho: count x 2 words, none zero.  checked (a context whose key was checked, else ZKHIP_ERR_STATE):
// k_point_check runs in front, a refused proof is left out of the product and the sums, and status (count bytes, or null) gets its
// refusal byte, 0 for a proof nothing refuses.  status without checked: ZKHIP_ERR_STATE.
int pairing_verify_all(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                       uint8_t* status, uint64_t* value, char* errbuf, size_t errlen);
// Per-proof verdicts by way of the combined check (zkhip.h "located batches"), count <= PAIRING_LOCATE_MAX: pairing_verify_all with the
// levels of its trees retained, and on a batch that fails the descent of locate.hpp.  verdict[i]: 1 / 0, or with checked the status
// byte of pairing_verify_batch.  value: the batch's reduced GT value.  trace: null, or where every node tested goes.
int pairing_verify_located(PairingCtx* c, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho, bool checked,
                           uint8_t* verdict, zkhip_locate_stats* stats, uint64_t* value, std::vector<host::LocateTraceNode>* trace, char* errbuf,
                           size_t errlen);
// the host's time behind the last chunk of the last pairing_verify_all: the shared pairs and the final exponentiation
double pairing_ctx_last_finish_ms(const PairingCtx* c);
// the key of a verifier context in the form of pairing_host.hpp's CombineKey (G2 points negated), for the host route on a handle
void pairing_ctx_key(const PairingCtx* c, const uint64_t** alpha, const uint64_t** neg_g2, const uint64_t** neg_beta, const uint64_t** neg_delta,
                     const uint64_t** abc);
// op 0: a b, 1: a^2, 2: a (b0 + b3 w^3 + b4 w^4) through the lane bodies of pairing.cuh; a, b, out: n x 72 ABI limbs
int pairing_fq6_selftest(int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, char* errbuf, size_t errlen);

}  // namespace zkhip
