// Stand-alone program (its own main) over the HOST code the nested verifier leans on, for a build with the address and
// undefined-behaviour sanitizers (tests/test_nested_host_route_sanitized.py): the key check and preparation of a handle
// (nested_key.hpp), the host verifier zkhip_bls12_377_groth16_verify - the fallback of proofs the device does not decide, its
// rejecting path (an exception inside the circuit DSL) and a key without inputs included - and the computation of route 0 of
// zkhip_internal_nested_pairing_product (g2_precompute, multi_miller_loop, final_exponentiation).  Linked with
// zecale_amd/csrc/aggregator.cpp; no device code.  Test infrastructure only.
//
// stdin: text, one statement per line:  k  then 60 + 12 (k + 1) key limbs, 6 k input limbs, 48 proof limbs, all hexadecimal.
// stdout: per statement "refused <why>" for a key that is refused, else
//         "<limbs of lines> <limbs of chain> <xor of the chain's limbs> <verdict> <xor of the limbs of e(A, B)>".
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../include/zkhip.h"
#include "../zecale_amd/csrc/nested_key.hpp"

namespace C = zkhip::circuit;
using C::NF;

int main() {
  unsigned long long k;
  while (scanf("%llu", &k) == 1) {
    if (k > 16) return 2;
    std::vector<uint64_t> vk(60 + 12 * (k + 1)), in(6 * k), pr(48);
    for (std::vector<uint64_t>* v : {&vk, &in, &pr})
      for (uint64_t& x : *v) {
        unsigned long long t;
        if (scanf("%llx", &t) != 1) return 2;
        x = t;
      }
    // what zkhip_nested_verifier_new derives from the key before it touches a device
    zkhip::nested_key::PreparedKey pk;
    std::string why;
    if (!zkhip::nested_key::prepare_key(vk.data(), k, &pk, &why)) {
      printf("refused %s\n", why.c_str());
      continue;
    }
    uint64_t chain = 0;
    for (uint64_t l : pk.chain) chain ^= l;
    printf("%zu %zu %016llx ", pk.lines.size(), pk.chain.size(), (unsigned long long)chain);
    int ok = -1;
    const int rc = zkhip_bls12_377_groth16_verify(vk.data(), vk.data() + 12, vk.data() + 36, vk.data() + 60, k ? in.data() : nullptr, k,
                                                  pr.data(), pr.data() + 12, pr.data() + 36, &ok);
    if (rc != ZKHIP_OK) return 3;
    // route 0 on the pair (A, B)
    const std::vector<C::G2Lines<NF>> lines = C::g2_precompute<NF>({C::g2_from<NF>(pr.data() + 12, false)});
    const std::vector<C::MillerPair<NF>> ps{{&lines[0], C::g1_from<NF>(pr.data(), false)}};
    const C::Fq12<NF> e = C::final_exponentiation(C::multi_miller_loop(ps));
    uint64_t acc = 0, limbs[6];
    for (int c = 0; c < 12; c++) {
      e.c[c].v.to_limbs(limbs);
      for (uint64_t l : limbs) acc ^= l;
    }
    printf("%d %016llx\n", ok, (unsigned long long)acc);
  }
  return 0;
}
