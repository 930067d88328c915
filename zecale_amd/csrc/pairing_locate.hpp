// Located batches over BW6-761: what the descent of locate.hpp needs from this curve, shared by the device route (pairing.hip), the
// host route (api_verify.hip) and the test shim (tests/locate_host_shim.cpp).  A node test is host::combined_value on the node's
// unreduced product, its sum of rho_i C_i and the scalar sums of its range, compared with one.  Host code; g++ compiles it.
#pragma once
#include <chrono>
#include <thread>
#include <vector>

#include "locate.hpp"
#include "pairing.cuh"
#include "pairing_host.hpp"

namespace zkhip {
namespace host {

// The cost rule's constants, host clock on the MI355X box (profiles/verify_locate.txt): one node test, and the per-proof route on up
// to 4,096 / 8,192 / 12,288 / 16,384 proofs - its time rises in steps of 4,096, a workgroup of 16 verifications per compute unit.
constexpr locate::Cost LOCATE_COST = {36.9, 4096, {181.1, 274.0, 325.5, 342.1}};

// threads of a round of node tests: the rule of the host route of the combined check
inline unsigned locate_threads() {
  const unsigned hw = std::thread::hardware_concurrency();
  return hw > 16 ? 16 : hw ? hw : 1;
}

struct LocateTraceNode {
  locate::Node node;
  bool passed;
  uint64_t value[72];                // the reduced value of the node's combined check
};

// sigma and the sums of rho_i x_ij over the proofs [lo, hi) of the batch that `skip` (null, or one byte per proof) does not leave out
inline CombineSums range_sums(size_t n_inputs, const uint64_t* inputs, const uint64_t* rho, const uint8_t* skip, size_t lo, size_t hi) {
  CombineSums sums(n_inputs);
  for (size_t i = lo; i < hi; i++)
    if (!skip || !skip[i]) sums.add(rho + i * 2, inputs + i * n_inputs * 6);
  return sums;
}

// the proofs [lo, hi) of the batch that node `n` covers; first: where the node's chunk starts, m: its size
inline void node_range(const locate::Node& n, size_t first, size_t m, size_t* lo, size_t* hi) {
  *lo = first + locate::range_lo(PAIRING_STRIP, (int)n.level, n.index);
  *hi = first + locate::range_hi(m, PAIRING_STRIP, (int)n.level, n.index);
}

// One round: node i covers [lo[i], hi[i]) and has the unreduced product f[i] and the sum s_c[i].  The tests are dealt to `threads`
// threads as combined_proofs_host deals its proofs.  given: empty, or per node the sums of its range where the caller has them (a chunk's
// root: the chunk's own), null where not.  trace: null, or where the nodes go with their values.
inline void test_nodes(const CombineKey& key, const uint64_t* inputs, const uint64_t* rho, const uint8_t* skip, const std::vector<locate::Node>& nodes,
                       const std::vector<size_t>& lo, const std::vector<size_t>& hi, const std::vector<Fq6>& f, const std::vector<HJac>& s_c,
                       unsigned threads, std::vector<uint8_t>& passed, std::vector<LocateTraceNode>* trace,
                       const std::vector<const CombineSums*>& given = std::vector<const CombineSums*>()) {
  const size_t n = nodes.size();
  if (threads < 1) threads = 1;
  if (threads > n) threads = n ? (unsigned)n : 1;
  std::vector<Fq6> value(n);
  auto work = [&](unsigned t) {
    for (size_t i = t; i < n; i += threads) {
      value[i] = !given.empty() && given[i] ? combined_value(key, *given[i], s_c[i], f[i])
                                            : combined_value(key, range_sums(key.n_inputs, inputs, rho, skip, lo[i], hi[i]), s_c[i], f[i]);
      passed[i] = value[i].is_one() ? 1 : 0;
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  if (!trace) return;
  for (size_t i = 0; i < n; i++) {
    LocateTraceNode tn;
    tn.node = nodes[i];
    tn.passed = passed[i] != 0;
    fq6_to_limbs(value[i], tn.value);
    trace->push_back(tn);
  }
}

// one proof on the host under a CombineKey (its G2 points negated): e(A, B) e(acc, -g2) e(alpha, -beta) e(C, -delta) == 1
inline bool verify_one_host(const CombineKey& key, const uint64_t* inputs, const uint64_t* proof) {
  HJac acc = jac_from_limbs(key.abc);
  for (size_t i = 0; i < key.n_inputs; i++) {
    uint64_t k[6];
    HFr::from_limbs(inputs + i * 6).to_canonical(k);
    acc = acc.add(jac_from_limbs(key.abc + (i + 1) * 24).mul_canonical(k, 6));
  }
  uint64_t acc_aff[24];
  jac_to_limbs(acc, acc_aff);
  return pairing_product_is_one({proof, acc_aff, key.alpha, proof + 48}, {proof + 24, key.neg_g2, key.neg_beta, key.neg_delta});
}

// the per-proof share of the combined check for every proof on its own, dealt to `threads` threads: f[i] = f(rho_i A_i, B_i) unreduced
// and c[i] = rho_i C_i (the body of combined_proofs_host); a proof that `skip` leaves out is one and infinity
inline void combined_leaves_host(const uint64_t* proofs, size_t count, const uint64_t* rho, const uint8_t* skip, unsigned threads,
                                 std::vector<Fq6>& f, std::vector<HJac>& c) {
  f.assign(count, Fq6::one());
  c.assign(count, HJac::infinity());
  if (threads < 1) threads = 1;
  if (threads > count) threads = count ? (unsigned)count : 1;
  auto work = [&](unsigned t) {
    for (size_t i = t; i < count; i += threads) {
      if (skip && skip[i]) continue;
      const uint64_t* pr = proofs + i * 72;
      uint64_t ra[24];
      jac_to_limbs(jac_from_limbs(pr).mul_canonical(rho + i * 2, 2), ra);
      f[i] = miller_product({ra}, {pr + 24});
      c[i] = jac_from_limbs(pr + 48).mul_canonical(rho + i * 2, 2);
    }
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The located route on the host alone, for a batch of at most PAIRING_LOCATE_MAX proofs.  skip: null, or per proof non-zero for a
// proof that is left out everywhere (its state stays CLEARED: the caller knows why it left it out).  finish(list) -> int: the per-proof
// route on the listed proofs.  state: locate::CLEARED / INVALID / FINISHED per proof; value: the batch's reduced value.
template <class Finish>
int located_batch_host(const CombineKey& key, const uint64_t* inputs, const uint64_t* proofs, size_t count, const uint64_t* rho,
                       const uint8_t* skip, unsigned threads, const locate::Cost& cost, Finish finish, std::vector<uint8_t>& state,
                       zkhip_locate_stats& stats, std::vector<LocateTraceNode>* trace, uint64_t* value) {
  stats = zkhip_locate_stats();
  if (trace) trace->clear();
  std::vector<Fq6> leaf_f;
  std::vector<HJac> leaf_c;
  combined_leaves_host(proofs, count, rho, skip, threads, leaf_f, leaf_c);
  std::vector<size_t> chunks, first;
  for (size_t lo = 0; lo < count; lo += PAIRING_CHUNK) { first.push_back(lo); chunks.push_back(count - lo < PAIRING_CHUNK ? count - lo : PAIRING_CHUNK); }
  auto node_value = [&](size_t lo, size_t hi, Fq6& f, HJac& c) {
    f = Fq6::one();
    c = HJac::infinity();
    for (size_t i = lo; i < hi; i++) { f = f * leaf_f[i]; c = c.add(leaf_c[i]); }
  };
  Fq6 product;
  HJac s_c;
  node_value(0, count, product, s_c);
  const Fq6 total = combined_value(key, range_sums(key.n_inputs, inputs, rho, skip, 0, count), s_c, product);
  if (value) fq6_to_limbs(total, value);
  state.assign(count, locate::CLEARED);
  if (total.is_one()) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  double fin_ms = 0;
  const std::vector<uint8_t> known(1, 0);
  if (trace && chunks.size() == 1) {
    LocateTraceNode tn;
    tn.node = {0, (uint32_t)locate::root_level(count, PAIRING_STRIP), 0};
    tn.passed = false;
    fq6_to_limbs(total, tn.value);
    trace->push_back(tn);
  }
  locate::Stats st;
  const int rc = locate::descend(
      chunks, PAIRING_STRIP, cost, threads, chunks.size() == 1 ? &known : nullptr,
      [&](const std::vector<locate::Node>& nodes, std::vector<uint8_t>& passed) -> int {
        std::vector<size_t> lo(nodes.size()), hi(nodes.size());
        std::vector<Fq6> f(nodes.size());
        std::vector<HJac> c(nodes.size());
        for (size_t i = 0; i < nodes.size(); i++) {
          node_range(nodes[i], first[nodes[i].chunk], chunks[nodes[i].chunk], &lo[i], &hi[i]);
          node_value(lo[i], hi[i], f[i], c[i]);
        }
        test_nodes(key, inputs, rho, skip, nodes, lo, hi, f, c, threads, passed, trace);
        return 0;
      },
      [&](const std::vector<size_t>& list) -> int {
        const auto t1 = std::chrono::steady_clock::now();
        const int r = finish(list);
        fin_ms = ms_since(t1);
        return r;
      },
      state, st);
  stats.chunks_failed = st.chunks_failed; stats.rounds = st.rounds; stats.node_tests = st.node_tests; stats.finish_proofs = st.finish_proofs;
  stats.finish_ms = fin_ms;
  stats.descent_ms = ms_since(t0) - fin_ms;
  return rc;
}

}  // namespace host
}  // namespace zkhip
