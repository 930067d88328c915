// Located batches: which proofs of a failed combined batch are invalid, found by descending the reduction trees the combined check
// built anyway.  A batch runs in chunks; a chunk of m proofs has a tree of arity `a` (the strip of the reduction kernels): level 0 holds
// the m proofs, level k + 1 one node per strip of level k, the last level the chunk's root.  Node s of level k covers the chunk's proofs
// [s a^k, min((s + 1) a^k, m)), and a node together with the scalar sums of its range is a complete combined check of that sub-batch
// under the same scalars - the same soundness bound, the same finishing code.  So a failed batch is searched from the roots down: a
// node that passes clears its whole range, a node that fails hands its children to the next round, a leaf that fails is an invalid
// proof.
//
// This header is the descent alone.  It knows no curve and no field: the caller hands in how a round of nodes is tested and how a set
// of proofs is finished on the per-proof route, so the verifier of either curve can use it.  Plain C++, host only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace zkhip {
namespace locate {

struct Node {
  uint32_t chunk, level;
  size_t index;                      // within its level
};

// ---- the integer rules (constexpr: a test shim reads them)
constexpr size_t strips(size_t n, size_t arity) { return (n + arity - 1) / arity; }
// the level of the root of a tree over m >= 1 leaves: the number of reductions until one strip is left (pairing_tree_levels)
constexpr int root_level(size_t m, size_t arity) {
  int levels = 1;
  for (; strips(m, arity) > 1; m = strips(m, arity)) levels++;
  return levels;
}
constexpr size_t span(size_t arity, int level) {
  size_t w = 1;
  for (; level > 0; level--) w *= arity;
  return w;
}
// the leaves [lo, hi) of a chunk of m that node `index` of `level` covers
constexpr size_t range_lo(size_t arity, int level, size_t index) { return index * span(arity, level); }
constexpr size_t range_hi(size_t m, size_t arity, int level, size_t index) {
  return (index + 1) * span(arity, level) < m ? (index + 1) * span(arity, level) : m;
}

// ---- the cost rule.  Before a round the descent compares two host clock times (those of the BW6-761 verifier are measured in
// profiles/verify_locate.txt; another verifier brings its own):
//   the rounds that are left, each ceil(tests / threads) node tests long;
//   the per-proof route on the proofs under the frontier.
// When the per-proof route is cheaper, those proofs go to it.  The tests of a round stay what they are while one child fails under
// every node that failed - a few bad proofs.  A round of two or more nodes in which EVERY node failed says the opposite, that the bad
// proofs are many and spread: the rounds below it are then taken eight times as wide each, up to one test per proof, which hands a
// batch with many bad proofs over after the one round that showed it.
constexpr int COST_STEPS = 4;
struct Cost {
  double node_ms;                    // one node test: the range's sums, the three shared pairs, one final exponentiation
  size_t step;                       // the per-proof route's time rises in steps of this many proofs (a workgroup per compute unit)
  double step_ms[COST_STEPS];        // the per-proof route on up to 1, 2, 3, 4 steps of proofs; 4 steps are its chunk, chunks add up
};
constexpr double finish_ms(const Cost& c, size_t proofs) {
  return (double)(proofs / (c.step * COST_STEPS)) * c.step_ms[COST_STEPS - 1] +
         (proofs % (c.step * COST_STEPS) ? c.step_ms[(proofs % (c.step * COST_STEPS) - 1) / c.step] : 0.0);
}
// `rounds` rounds dealt to `threads` threads, the first of `tests` node tests, each later one `widen` times as wide (never more tests
// than the `proofs` under the frontier): a round takes as long as its longest thread
constexpr double descent_ms(const Cost& c, size_t rounds, size_t tests, unsigned threads, size_t widen, size_t proofs) {
  double ms = 0;
  for (size_t r = 0; r < rounds; r++) {
    ms += (double)((tests + threads - 1) / threads) * c.node_ms;
    tests = tests * widen < proofs ? tests * widen : tests < proofs ? proofs : tests;
  }
  return ms;
}
// true: stop descending and finish the `proofs` proofs under the `tests` nodes of the coming round on the per-proof route.  rounds:
// what is left of the descent, this round included; tested, failed: the round before (0, 0: none).  A tie descends.
constexpr bool prefers_finish(const Cost& c, size_t rounds, size_t tests, unsigned threads, size_t proofs, size_t arity, size_t tested, size_t failed) {
  return finish_ms(c, proofs) < descent_ms(c, rounds, tests, threads ? threads : 1, tested >= 2 && failed == tested ? arity : 1, proofs);
}

struct Stats {
  uint32_t chunks_failed = 0, rounds = 0, node_tests = 0, finish_proofs = 0;
};

enum : uint8_t { CLEARED = 0, INVALID = 1, FINISHED = 2 };

// The descent over a failed batch of chunks.size() chunks, chunk c holding chunks[c] proofs that follow those of the chunks before.
//   test(nodes, passed) -> int: tests every node of a round (passed[i] = 1 / 0), 0 or an error code that ends the descent;
//   finish(proofs) -> int: the per-proof route on the given proofs (ascending indices into the batch); the caller keeps their verdicts.
// roots_known: null, or the verdicts of the chunk roots where the caller has them already (a batch of one chunk: its root's value is
// the batch's) - the chunk round then costs nothing and is not put to the rule.
// state[i] for every proof of the batch: CLEARED (under a node that passed), INVALID (a leaf that failed) or FINISHED.
template <class Test, class Finish>
int descend(const std::vector<size_t>& chunks, size_t arity, const Cost& cost, unsigned threads, const std::vector<uint8_t>* roots_known,
            Test test, Finish finish, std::vector<uint8_t>& state, Stats& st) {
  std::vector<size_t> first(chunks.size() + 1, 0);
  for (size_t c = 0; c < chunks.size(); c++) first[c + 1] = first[c] + chunks[c];
  state.assign(first.back(), CLEARED);
  st = Stats();
  std::vector<Node> round;             // the nodes of the coming round: the chunk roots, then the children of the nodes that failed
  for (size_t c = 0; c < chunks.size(); c++)
    if (chunks[c]) round.push_back({(uint32_t)c, (uint32_t)root_level(chunks[c], arity), 0});
  std::vector<uint8_t> passed;
  size_t tested = 0, failed = 0;       // of the round before: what the rule reads
  for (bool chunk_round = true; !round.empty(); chunk_round = false) {
    const bool known = chunk_round && roots_known;
    size_t proofs = 0, deepest = 0;
    for (const Node& n : round) {
      proofs += range_hi(chunks[n.chunk], arity, n.level, n.index) - range_lo(arity, n.level, n.index);
      if (n.level > deepest) deepest = n.level;
    }
    if (!known && prefers_finish(cost, deepest + 1, round.size(), threads, proofs, arity, tested, failed)) {
      std::vector<size_t> list;
      list.reserve(proofs);
      for (const Node& n : round)
        for (size_t i = range_lo(arity, n.level, n.index), hi = range_hi(chunks[n.chunk], arity, n.level, n.index); i < hi; i++) {
          list.push_back(first[n.chunk] + i);
          state[first[n.chunk] + i] = FINISHED;
        }
      st.finish_proofs = (uint32_t)list.size();
      return finish(list);
    }
    if (known) passed = *roots_known;
    else {
      passed.assign(round.size(), 0);
      const int rc = test(round, passed);
      if (rc) return rc;
    }
    st.rounds++;
    st.node_tests += (uint32_t)round.size();
    std::vector<Node> next;
    tested = round.size();
    failed = 0;
    for (size_t i = 0; i < round.size(); i++) {
      if (passed[i]) continue;
      failed++;
      const Node& n = round[i];
      if (chunk_round) st.chunks_failed++;
      if (n.level == 0) { state[first[n.chunk] + n.index] = INVALID; continue; }
      const size_t below = strips(chunks[n.chunk], span(arity, n.level - 1));      // nodes of the level below: ceil(m / a^(level - 1))
      for (size_t s = n.index * arity; s < (n.index + 1) * arity && s < below; s++) next.push_back({n.chunk, n.level - 1, s});
    }
    round.swap(next);
  }
  return 0;
}

}  // namespace locate
}  // namespace zkhip
