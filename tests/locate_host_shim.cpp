// Host-side test shim of the located batches: the integer rules of the retained trees (zecale_amd/csrc/pairing.cuh), the descent and
// its cost rule (locate.hpp) driven by a fake tester, and the host route on real proofs (pairing_locate.hpp), compiled by g++ so that
// tests/test_locate_model.py can check them without a GPU.  Test infrastructure only.
#include <string.h>

#include <vector>

#include "../zecale_amd/csrc/locate.hpp"
#include "../zecale_amd/csrc/pairing.cuh"
#include "../zecale_amd/csrc/pairing_host.hpp"
#include "../zecale_amd/csrc/pairing_locate.hpp"
using namespace zkhip;

// the rules hold at compile time as well
static_assert(pairing_tree_nodes(1) == 2 && pairing_tree_nodes(8) == 9 && pairing_tree_nodes(9) == 12, "");
static_assert(pairing_level_offset(16384, 5) + 1 == pairing_tree_nodes(16384) && pairing_tree_nodes(16384) == 16384 + 2048 + 256 + 32 + 4 + 1, "");
static_assert(locate::root_level(513, 8) == pairing_tree_levels(513), "");

extern "C" {
int strip() { return PAIRING_STRIP; }
size_t chunk() { return PAIRING_CHUNK; }
size_t locate_max() { return PAIRING_LOCATE_MAX; }
size_t strips(size_t n) { return pairing_strips(n); }
int tree_levels(size_t n) { return pairing_tree_levels(n); }
size_t tree_nodes(size_t n) { return pairing_tree_nodes(n); }
size_t level_offset(size_t n, int k) { return pairing_level_offset(n, k); }
size_t level_size(size_t n, int k) { return pairing_level_size(n, k); }
void node_range_of(size_t m, int level, size_t index, size_t* lo, size_t* hi) {
  *lo = locate::range_lo(PAIRING_STRIP, level, index);
  *hi = locate::range_hi(m, PAIRING_STRIP, level, index);
}

// the cost rule; cost = node_ms, then the per-proof route's time on up to 1, 2, 3, 4 steps of `step` proofs
static locate::Cost make_cost(const double cost[5], size_t step) { return {cost[0], step, {cost[1], cost[2], cost[3], cost[4]}}; }
void default_cost(double cost[5], size_t* step) {
  cost[0] = host::LOCATE_COST.node_ms;
  for (int i = 0; i < 4; i++) cost[1 + i] = host::LOCATE_COST.step_ms[i];
  *step = host::LOCATE_COST.step;
}
double rule_finish_ms(const double cost[5], size_t step, size_t proofs) { return locate::finish_ms(make_cost(cost, step), proofs); }
double rule_descent_ms(const double cost[5], size_t step, size_t rounds, size_t tests, unsigned threads, size_t widen, size_t proofs) {
  return locate::descent_ms(make_cost(cost, step), rounds, tests, threads, widen, proofs);
}
int rule_prefers_finish(const double cost[5], size_t step, size_t rounds, size_t tests, unsigned threads, size_t proofs, size_t tested, size_t failed) {
  return locate::prefers_finish(make_cost(cost, step), rounds, tests, threads, proofs, PAIRING_STRIP, tested, failed) ? 1 : 0;
}

// The descent over `count` proofs in chunks of `chunk_size` with a FAKE tester: a node fails iff its range holds an index with bad[i]
// set.  roots_known: hand the descent the root's verdict as the routes do for a batch of one chunk.  state: per proof CLEARED 0 /
// INVALID 1 / FINISHED 2; leaf_tested: per proof 1 when it was tested as a node of level 0; stats: chunks_failed, rounds, node_tests,
// finish_proofs; round_sizes (cap 64): the tests of each round.  Returns the number of rounds, negative on an error.
int fake_descend(size_t count, size_t chunk_size, const uint8_t* bad, unsigned threads, const double cost[5], size_t step, int roots_known,
                 uint8_t* state, uint8_t* leaf_tested, uint32_t stats[4], uint32_t* round_sizes) {
  std::vector<size_t> chunks, first;
  for (size_t lo = 0; lo < count; lo += chunk_size) { first.push_back(lo); chunks.push_back(count - lo < chunk_size ? count - lo : chunk_size); }
  const std::vector<uint8_t> known(1, 0);
  std::vector<uint8_t> st_out;
  locate::Stats st;
  int rounds = 0;
  memset(leaf_tested, 0, count);
  if (roots_known && chunks.size() == 1) round_sizes[rounds++] = 1;
  const int rc = locate::descend(
      chunks, PAIRING_STRIP, make_cost(cost, step), threads, roots_known && chunks.size() == 1 ? &known : nullptr,
      [&](const std::vector<locate::Node>& nodes, std::vector<uint8_t>& passed) -> int {
        if (rounds >= 64) return -1;
        round_sizes[rounds++] = (uint32_t)nodes.size();
        for (size_t i = 0; i < nodes.size(); i++) {
          size_t lo, hi;
          host::node_range(nodes[i], first[nodes[i].chunk], chunks[nodes[i].chunk], &lo, &hi);
          if (lo >= hi || hi > count) return -2;
          if (nodes[i].level == 0) leaf_tested[lo] = 1;
          passed[i] = 1;
          for (size_t j = lo; j < hi; j++) if (bad[j]) passed[i] = 0;
        }
        return 0;
      },
      [&](const std::vector<size_t>& list) -> int {
        for (size_t i = 0; i < list.size(); i++) if (list[i] >= count || (i && list[i] <= list[i - 1])) return -3;
        return 0;
      },
      st_out, st);
  if (rc) return rc;
  memcpy(state, st_out.data(), count);
  stats[0] = st.chunks_failed; stats[1] = st.rounds; stats[2] = st.node_tests; stats[3] = st.finish_proofs;
  return rounds;
}

// The host route on real proofs (what zkhip_groth16_verify_batch_located runs behind its curve check), with the tree's constants and
// the cost rule of the library.  state as above, with FINISHED proofs resolved by the host's per-proof check: 1 invalid, 0 valid.
// trace: up to cap nodes; returns their number, negative on an error.
long located_host(const uint64_t* alpha, const uint64_t* beta, const uint64_t* delta, const uint64_t* abc, size_t n_inputs, const uint64_t* inputs,
                  const uint64_t* proofs, size_t count, const uint64_t* rho, unsigned threads, uint8_t* invalid, zkhip_locate_stats* stats,
                  zkhip_locate_node* trace, size_t cap, uint64_t* value) {
  using namespace host;
  uint64_t neg_g2[24], neg_beta[24], neg_delta[24];
  neg_g2_generator(neg_g2); neg_point_abi(beta, neg_beta); neg_point_abi(delta, neg_delta);
  const CombineKey key = {alpha, neg_g2, neg_beta, neg_delta, abc, n_inputs};
  std::vector<uint8_t> state;
  std::vector<LocateTraceNode> tr;
  std::vector<uint8_t> finished(count, 0);
  const int rc = located_batch_host(
      key, inputs, proofs, count, rho, nullptr, threads, LOCATE_COST,
      [&](const std::vector<size_t>& list) -> int {
        for (size_t i : list) finished[i] = verify_one_host(key, inputs + i * n_inputs * 6, proofs + i * 72) ? 0 : 1;
        return 0;
      },
      state, *stats, &tr, value);
  if (rc) return -1;
  for (size_t i = 0; i < count; i++) invalid[i] = state[i] == locate::INVALID || (state[i] == locate::FINISHED && finished[i]);
  for (size_t i = 0; i < tr.size() && i < cap; i++) {
    trace[i].chunk = tr[i].node.chunk; trace[i].level = tr[i].node.level; trace[i].passed = tr[i].passed; trace[i].reserved = 0;
    trace[i].index = tr[i].node.index;
    memcpy(trace[i].value, tr[i].value, sizeof tr[i].value);
  }
  return (long)tr.size();
}
}

#ifdef LOCATE_SHIM_MAIN
// stand-alone form for a sanitizer build (g++ -fsanitize=address,undefined -DLOCATE_SHIM_MAIN): fake descents over ragged trees and
// several chunks with every single bad index, all bad and none, under a rule that always descends and one that finishes at once
#include <stdio.h>
int main() {
  const double descend_always[5] = {1.0, 1e12, 1e12, 1e12, 1e12}, finish_at_once[5] = {1e12, 1.0, 1.0, 1.0, 1.0};
  unsigned long long acc = 0;
  for (size_t count : {(size_t)1, (size_t)8, (size_t)9, (size_t)65, (size_t)513})
    for (size_t chunk_size : {(size_t)7, (size_t)64, (size_t)16384}) {
      std::vector<uint8_t> bad(count), state(count), leaf(count);
      uint32_t stats[4], rounds[64];
      for (size_t b = 0; b <= count + 1; b++) {
        for (size_t i = 0; i < count; i++) bad[i] = b == count ? 1 : i == b;       // b == count + 1: none
        for (const double* cost : {descend_always, finish_at_once}) {
          const int r = fake_descend(count, chunk_size, bad.data(), 16, cost, 4096, 1, state.data(), leaf.data(), stats, rounds);
          if (r < 0) { printf("error %d\n", r); return 1; }
          for (size_t i = 0; i < count; i++) {
            if (cost == descend_always && state[i] != bad[i]) { printf("verdicts differ\n"); return 1; }
            acc = acc * 31 + state[i] + leaf[i];
          }
          acc += stats[2] + stats[3];
        }
      }
    }
  printf("%016llx\n", acc);
  return 0;
}
#endif
