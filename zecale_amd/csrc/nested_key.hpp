// What a nested (BLS12-377) verifier handle derives from its key ON THE HOST, before a device is touched: the curve checks, the lines of
// -beta, -delta and the negated generator (g2_precompute<NF>) and the doubling chains 2^j ABC_i.  Host code only (the circuit DSL with
// the native field), so that a CPU program can run it by itself; api_nested_verify.hip is its one user in the library.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdexcept>
#include <string>
#include <vector>

#include "circuit/sections.hpp"

namespace zkhip {
namespace nested_key {

namespace C = zkhip::circuit;
using C::HFr;
using C::NF;

inline bool g1_on_curve(const C::G1<NF>& p) {
  try { C::g1_assert_on_curve(p); } catch (const std::exception&) { return false; }
  return true;
}
inline bool g2_on_curve(const C::G2<NF>& p) {
  try { C::g2_assert_on_curve(p); } catch (const std::exception&) { return false; }
  return true;
}
inline void put(std::vector<uint64_t>& v, const HFr& x) { v.resize(v.size() + 6); x.to_limbs(&v[v.size() - 6]); }

// the 69 lines of each point, flattened (lambda'_0, lambda'_1, b_0, b_1); empty with `which` set when a schedule is degenerate
inline std::vector<uint64_t> lines_of(const std::vector<C::G2<NF>>& Qs, int* which) {
  *which = -1;
  for (size_t k = 0; k < Qs.size(); k++) {
    std::vector<HFr> ninv;
    if (!C::g2_schedule_norm_invs(C::v2_of(Qs[k].x), C::v2_of(Qs[k].y), ninv)) { *which = (int)k; return {}; }
  }
  const std::vector<C::G2Lines<NF>> l = C::g2_precompute<NF>(Qs);
  std::vector<uint64_t> out;
  for (const auto& ls : l) {
    if (ls.size() != 69) throw std::runtime_error("the Miller schedule does not have 69 lines");
    for (const auto& lc : ls) { put(out, lc.lam.c0.v); put(out, lc.lam.c1.v); put(out, lc.b.c0.v); put(out, lc.b.c1.v); }
  }
  return out;
}

// Everything a handle derives from its key.  False with the element's name in *why for a key that is refused.
struct PreparedKey { std::vector<uint64_t> lines, chain; };
inline bool prepare_key(const uint64_t* vk, size_t k, PreparedKey* out, std::string* why) {
  char msg[160];
  const C::G1<NF> alpha = C::g1_from<NF>(vk, false);
  const C::G2<NF> beta = C::g2_from<NF>(vk + 12, false), delta = C::g2_from<NF>(vk + 36, false);
  if (!g1_on_curve(alpha)) { *why = "nested key refused: alpha: off its curve"; return false; }
  if (!g2_on_curve(beta)) { *why = "nested key refused: beta: off its curve"; return false; }
  if (!g2_on_curve(delta)) { *why = "nested key refused: delta: off its curve"; return false; }
  for (size_t i = 0; i <= k; i++) {
    if (g1_on_curve(C::g1_from<NF>(vk + 60 + i * 12, false))) continue;
    snprintf(msg, sizeof msg, "nested key refused: ABC[%zu]: off its curve", i);
    *why = msg;
    return false;
  }
  // the doubling chains 2^j ABC_i, j = 0 .. 252, affine as the host's accumulator walks them
  for (size_t i = 1; i <= k; i++) {
    HFr x = HFr::from_limbs(vk + 60 + i * 12), y = HFr::from_limbs(vk + 60 + i * 12 + 6);
    for (int j = 0; j < C::NESTED_INPUT_BITS; j++) {
      put(out->chain, x); put(out->chain, y);
      if (j + 1 == C::NESTED_INPUT_BITS) break;
      if ((y + y).is_zero()) {
        snprintf(msg, sizeof msg, "nested key refused: ABC[%zu]: its doubling chain is degenerate (2^%d ABC[%zu] has y = 0)", i, j, i);
        *why = msg;
        return false;
      }
      const HFr xx = x * x, lam = (xx + xx + xx) * (y + y).inv();
      const HFr x3 = lam * lam - (x + x), y3 = lam * (x - x3) - y;
      x = x3; y = y3;
    }
  }
  const C::BlsG2Gen& gg = C::bls_g2_gen();
  const C::G2<NF> gen{C::Fq2<NF>::constant(gg.x0, gg.x1), C::Fq2<NF>::constant(gg.y0, gg.y1)};
  int which = -1;
  out->lines = lines_of({C::g2_neg(beta), C::g2_neg(delta), C::g2_neg(gen)}, &which);
  if (which >= 0) {
    snprintf(msg, sizeof msg, "nested key refused: %s: a slope denominator of its line schedule is zero", which == 0 ? "beta" : which == 1 ? "delta" : "the generator");
    *why = msg;
    return false;
  }
  return true;
}

}  // namespace nested_key
}  // namespace zkhip
