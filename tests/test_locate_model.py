"""Located batches without a GPU: the integer rules of the retained trees (zecale_amd/csrc/pairing.cuh), the descent and its cost rule
(zecale_amd/csrc/locate.hpp) under a fake tester, and the host route on real proofs (pairing_locate.hpp) against the closed forms of
tests/combine_fixtures.py, all through the g++ shim tests/locate_host_shim.cpp; and zkhip_groth16_verify_batch_located through the
library.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import combine_fixtures as C
from tests import verify_fixtures as V

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")
STRIP = 8
ONE = V.EXT.one()
CLEARED, INVALID, FINISHED = 0, 1, 2
ALWAYS_DESCEND = (1.0, 1e12, 1e12, 1e12, 1e12)      # node_ms, then the per-proof route on 1 .. 4 steps: a node test costs nothing beside it
ALWAYS_FINISH = (1e12, 1.0, 1.0, 1.0, 1.0)
STEP = 4096


@pytest.fixture(scope="module")
def shim():
    from zecale_amd import zkhip
    so = os.path.join(HERE, "liblocate_host_shim.so")
    src = os.path.join(HERE, "locate_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("locate.hpp", "pairing_locate.hpp", "pairing.cuh", "pairing_host.hpp", "host_field.hpp", "ec.cuh",
                                             "fp29.cuh", "fp_inv.cuh", "bw6_params.h")] + [os.path.join(HERE, "..", "include", "zkhip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, sz, dp = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)
    for name in ("chunk", "locate_max", "strips", "tree_nodes", "level_offset", "level_size"):
        getattr(lib, name).restype = sz
    lib.strips.argtypes, lib.tree_levels.argtypes, lib.tree_nodes.argtypes = [sz], [sz], [sz]
    lib.level_offset.argtypes = lib.level_size.argtypes = [sz, ctypes.c_int]
    lib.node_range_of.argtypes = [sz, ctypes.c_int, sz, vp, vp]
    lib.default_cost.argtypes = [dp, vp]
    lib.rule_finish_ms.argtypes, lib.rule_finish_ms.restype = [dp, sz, sz], ctypes.c_double
    lib.rule_descent_ms.argtypes, lib.rule_descent_ms.restype = [dp, sz, sz, sz, ctypes.c_uint, sz, sz], ctypes.c_double
    lib.rule_prefers_finish.argtypes = [dp, sz, sz, sz, ctypes.c_uint, sz, sz, sz]
    lib.fake_descend.argtypes = [sz, sz, vp, ctypes.c_uint, dp, sz, ctypes.c_int, vp, vp, vp, vp]
    lib.located_host.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp, ctypes.c_uint, vp, ctypes.POINTER(zkhip.LocateStats),
                                 ctypes.POINTER(zkhip.LocateNode), sz, vp]
    lib.located_host.restype = ctypes.c_long
    return lib


def _cost(c):
    return (ctypes.c_double * 5)(*c)


def level_sizes(n):
    """the sizes of the levels of a tree over n values: n, then strips iterated until one node is WRITTEN (n = 1: 1, 1)"""
    sizes = [n]
    while True:
        sizes.append(-(-sizes[-1] // STRIP))
        if sizes[-1] == 1:
            return sizes


# ---------------------------------------------------------------- the integer rules
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 512, 513, 16384])
def test_levels_of_the_retained_trees(shim, n):
    """Level k starts where the levels below it end, so no two levels overlap; the last level holds one node and ends the buffer; the
    level sizes are pairing_strips iterated, one level per launch of the reduction tree."""
    sizes = level_sizes(n)
    levels = shim.tree_levels(n)
    assert levels == len(sizes) - 1
    assert [shim.level_size(n, k) for k in range(levels + 1)] == sizes
    assert all(shim.level_size(n, k + 1) == shim.strips(shim.level_size(n, k)) for k in range(levels))
    offsets = [shim.level_offset(n, k) for k in range(levels + 1)]
    assert offsets[0] == 0 and all(offsets[k + 1] == offsets[k] + sizes[k] for k in range(levels))
    assert sizes[-1] == 1 and all(s > 1 for s in sizes[1:-1])
    assert shim.tree_nodes(n) == sum(sizes) == offsets[-1] + 1
    # a node's range: disjoint within a level, and a level covers the values exactly
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    for k in range(levels + 1):
        end = 0
        for s in range(sizes[k]):
            shim.node_range_of(n, k, s, ctypes.byref(lo), ctypes.byref(hi))
            assert lo.value == end == s * STRIP ** k and lo.value < hi.value <= n
            end = hi.value
        assert end == n


def test_constants(shim):
    assert (shim.strip(), shim.chunk(), shim.locate_max()) == (STRIP, 16384, 1 << 20)
    assert shim.tree_nodes(16384) == 16384 + 2048 + 256 + 32 + 4 + 1
    # 27 limbs of 32 bits per field element, six of them per product and four per sum: about 1.2 KB per proof
    assert 1.2e3 < shim.tree_nodes(16384) * (6 + 4) * 27 * 4 / 16384 < 1.25e3


# ---------------------------------------------------------------- the descent under a fake tester
def _fake(shim, count, bad, cost=ALWAYS_DESCEND, chunk=16384, threads=16, roots_known=True):
    flags = np.zeros(count, dtype=np.uint8)
    flags[list(bad)] = 1
    state, leaf = np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.uint8)
    stats, rounds = np.zeros(4, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
    r = shim.fake_descend(count, chunk, flags.ctypes.data, threads, _cost(cost), STEP, int(roots_known), state.ctypes.data, leaf.ctypes.data,
                          stats.ctypes.data, rounds.ctypes.data)
    assert r >= 0, r
    names = ("chunks_failed", "rounds", "node_tests", "finish_proofs")
    return state, leaf, dict(zip(names, (int(x) for x in stats))), [int(x) for x in rounds[:r]]


def bad_sets(count):
    """first; last; the end of one strip and the start of the next; two in one strip; a whole strip; the lone node of a ragged last
    strip; all - those that fit the count"""
    sets = {"first": {0}, "last": {count - 1}, "all": set(range(count))}
    if count > STRIP:
        sets.update({"7 and 8": {7, 8}, "two in one strip": {1, 5}, "a whole strip": set(range(STRIP))})
    if count % STRIP == 1 and count > 1:
        sets["ragged last strip"] = {count - 1}
    return sets


def path_fanouts(count, i):
    """the tests on the way to proof i of a one-chunk batch: the root, then at every level below it the children of the node above"""
    sizes = level_sizes(count)
    total = 1
    for k in range(len(sizes) - 2, -1, -1):
        parent = i // STRIP ** (k + 1)
        total += min((parent + 1) * STRIP, sizes[k]) - parent * STRIP
    return total


@pytest.mark.parametrize("count", [1, 8, 9, 65, 513])
def test_descent_finds_exactly_the_bad_set(shim, count):
    state, _, st, rounds = _fake(shim, count, set())
    assert not state.any() and st["finish_proofs"] == 0
    depth = len(level_sizes(count)) - 1
    for name, bad in bad_sets(count).items():
        state, leaf, st, rounds = _fake(shim, count, bad)
        assert {i for i in range(count) if state[i] == INVALID} == bad and set(state) <= {CLEARED, INVALID}, name
        assert st["finish_proofs"] == 0 and st["chunks_failed"] == 1 and st["rounds"] == depth + 1 == len(rounds), name
        assert st["node_tests"] == sum(rounds) and rounds[0] == 1, name
        assert all(leaf[i] for i in bad), name
        if len(bad) == 1:
            assert st["node_tests"] == path_fanouts(count, min(bad)), name
        # the same batch in chunks of 7 (ragged, more than one root) and without the root's verdict handed in
        for kw in (dict(chunk=7), dict(roots_known=False)):
            again = _fake(shim, count, bad, **kw)[0]
            assert (again == state).all(), (name, kw)


@pytest.mark.parametrize("count", [1, 8, 9, 65, 513])
def test_a_rule_that_prefers_finishing_hands_every_proof_over_once(shim, count):
    """All proofs bad under a rule that always finishes: the batch of one chunk knows its root already, so the first round it
    considers - the root's children - goes to the per-proof route whole; nothing is both finished and tested as a leaf."""
    state, leaf, st, rounds = _fake(shim, count, set(range(count)), cost=ALWAYS_FINISH)
    assert st["finish_proofs"] == count and (state == FINISHED).all() and not leaf.any()
    assert rounds == [1] and st["node_tests"] == 1
    # several chunks: the rule is asked before the chunk round
    state, leaf, st, rounds = _fake(shim, count, set(range(count)), cost=ALWAYS_FINISH, chunk=7)
    assert st["finish_proofs"] == count and (state == FINISHED).all() and not leaf.any()
    assert st["node_tests"] == (1 if count <= 7 else 0)
    # the library's own constants on 513 bad proofs: both halves fail, and it hands over before the 9 nodes of level 2
    cost, step = (ctypes.c_double * 5)(), ctypes.c_size_t()
    shim.default_cost(cost, ctypes.byref(step))
    assert step.value == STEP
    if count == 513:
        state, leaf, st, rounds = _fake(shim, count, set(range(count)), cost=tuple(cost))
        assert rounds == [1, 2] and st["finish_proofs"] == count and not leaf.any() and (state == FINISHED).all()
        one = _fake(shim, count, {100}, cost=tuple(cost))
        assert one[2]["finish_proofs"] == 0 and one[2]["rounds"] == 5 and {i for i in range(count) if one[0][i] == INVALID} == {100}


def test_cost_rule_at_its_boundary(shim):
    """finish_ms rises in steps and chunks add up; descent_ms is rounds x ceil(tests / threads) x node_ms while the tests of a round
    stay what they are, and eight times as wide round after round (up to one test per proof) once every node of a round of two or
    more failed; the rule hands over exactly when the per-proof route is the cheaper of the two, and a tie descends.  Boundaries
    in both directions."""
    cost, step = _cost((10.0, 100.0, 150.0, 190.0, 200.0)), 100
    assert [shim.rule_finish_ms(cost, step, n) for n in (0, 1, 100, 101, 200, 201, 300, 301, 400, 401, 800, 950)] == \
        [0.0, 100.0, 100.0, 150.0, 150.0, 190.0, 190.0, 200.0, 200.0, 300.0, 400.0, 550.0]
    D = lambda rounds, tests, threads, widen, proofs: shim.rule_descent_ms(cost, step, rounds, tests, threads, widen, proofs)
    assert [D(1, 1, 16, 1, 10 ** 6), D(5, 8, 16, 1, 10 ** 6), D(5, 16, 16, 1, 10 ** 6), D(5, 17, 16, 1, 10 ** 6), D(3, 8, 1, 1, 10 ** 6)] == \
        [10.0, 50.0, 50.0, 100.0, 240.0]
    # widened: 4, 32, 256 tests, and never more than one per proof
    assert D(3, 4, 16, 8, 10 ** 6) == (1 + 2 + 16) * 10.0 and D(3, 4, 16, 8, 100) == (1 + 2 + 7) * 10.0 and D(2, 9, 16, 8, 9) == 20.0
    P = lambda rounds, tests, threads, proofs, tested, failed: shim.rule_prefers_finish(cost, step, rounds, tests, threads, proofs, tested, failed)
    # ten rounds of 8 tests cost 100 ms: a tie with the first step descends; an eleventh round tips it, a second thread-load of tests too
    assert P(10, 8, 16, 100, 8, 1) == 0 and P(11, 8, 16, 100, 8, 1) == 1
    assert P(10, 17, 16, 100, 16, 2) == 1 and P(10, 16, 16, 100, 16, 2) == 0
    # the same eleven rounds against the second step of the per-proof route (150 ms) descend again
    assert P(11, 8, 16, 101, 8, 1) == 0
    # every node of the round before failed: 16, 128, 400 tests are 1 + 8 + 25 thread-loads against 200 ms - hand over; one node
    # that passed, or a round of one node (a root known to fail), and the width stays: three rounds, 30 ms - descend
    assert P(3, 16, 16, 400, 2, 2) == 1 and P(3, 16, 16, 400, 3, 2) == 0 and P(3, 16, 16, 400, 1, 1) == 0
    # all failed, but the leaves are next and fit the threads: 9 tests in one load - descend
    assert P(1, 9, 16, 9, 2, 2) == 0 and P(1, 64, 16, 64, 8, 8) == 0 and P(1, 400, 16, 400, 50, 50) == 1
    assert P(5, 1, 0, 1, 0, 0) == 0                                            # no thread count known: one thread
    # the constants of profiles/verify_locate.txt, written out so that the cases stay what they are when the library's move
    first = _cost((36.4, 180.7, 275.2, 326.0, 342.7))
    L = lambda rounds, tests, proofs, tested, failed: shim.rule_prefers_finish(first, 4096, rounds, tests, 16, proofs, tested, failed)
    # one bad proof among 16,384: five rounds of at most 8 tests stay far below the per-proof route, at the root and below it
    assert L(5, 4, 16384, 1, 1) == 0 and L(4, 8, 4096, 4, 1) == 0 and L(1, 8, 8, 8, 1) == 0
    # all four quarters of a chunk failed, both halves of 1,024 proofs, all four roots of 65,536: to the per-proof route
    assert L(4, 32, 16384, 4, 4) == 1 and L(3, 16, 1024, 2, 2) == 1 and L(5, 16, 65536, 4, 4) == 1
    # the chunk round of 65,536 proofs itself descends
    assert L(6, 4, 65536, 0, 0) == 0
    # the library's own: a node test is cheaper than the per-proof route's first step, which does not fall with the count
    lib_cost, lib_step = (ctypes.c_double * 5)(), ctypes.c_size_t()
    shim.default_cost(lib_cost, ctypes.byref(lib_step))
    assert lib_step.value == 4096 and 0 < lib_cost[0] < lib_cost[1] <= lib_cost[2] <= lib_cost[3] <= lib_cost[4]
    assert shim.rule_prefers_finish(lib_cost, lib_step.value, 5, 4, 16, 16384, 1, 1) == 0


RUN_COST = (36.4, 180.7, 275.2, 326.0, 342.7)          # node test, per-proof route on 1 .. 4 steps: what profiles/verify_locate.txt was run with
MEASURED_COST = (36.9, 181.1, 274.0, 325.5, 342.1)     # what that run measured: the library's LOCATE_COST


def test_the_profiles_cases_decide_the_same_under_the_constants_it_ran_with_and_the_ones_it_measured(shim):
    """profiles/verify_locate.txt is one run: it was made with RUN_COST and measured MEASURED_COST, which the library holds.  Replayed
    under the fake tester at the tool's seeded positions (tools/verify_ab.py located_table), every case of the profile takes the same
    rounds with the same node tests and hands over the same proofs under either set - and those are the figures the profile prints."""
    lib_cost, lib_step = (ctypes.c_double * 5)(), ctypes.c_size_t()
    shim.default_cost(lib_cost, ctypes.byref(lib_step))
    assert tuple(lib_cost) == MEASURED_COST and lib_step.value == STEP
    printed = {(1024, 1): (5, 27, 0), (16384, 1): (6, 37, 0), (65536, 1): (6, 40, 0), (16384, "1 %"): (2, 5, 16384), (65536, "1 %"): (1, 4, 65536),
               (1024, "1 %"): (2, 3, 1024)}
    for count in (1024, 16384, 65536):
        for spec in (1, 2, 16, "1 %"):
            nbad = max(1, count // 100) if spec == "1 %" else spec
            where = np.random.RandomState(count + nbad).choice(count, nbad, replace=False)
            ran = _fake(shim, count, where, cost=RUN_COST)
            measured = _fake(shim, count, where, cost=MEASURED_COST)
            assert ran[2] == measured[2] and ran[3] == measured[3] and (ran[0] == measured[0]).all(), (count, spec)
            if (count, spec) in printed:
                st = measured[2]
                assert (st["rounds"], st["node_tests"], st["finish_proofs"]) == printed[(count, spec)], (count, spec)


def test_descent_stands_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: fake descents over ragged trees in one and in several chunks, every single bad
    index, all and none, under a rule that always descends and one that finishes at once) built with the address and
    undefined-behaviour sanitizers and run on the CPU."""
    exe = tmp_path / "locate_shim_sanitized"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DLOCATE_SHIM_MAIN", "-o", str(exe), os.path.join(HERE, "locate_host_shim.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert len(out.stdout.strip()) == 16


# ---------------------------------------------------------------- the host route on real proofs
def rho_words(rhos):
    return np.array([[r & (2 ** 64 - 1), r >> 64] for r in rhos], dtype=np.uint64).reshape(-1, 2)


def _located_host(shim, n_inputs, inputs, proofs, rhos, threads=16):
    from zecale_amd import zkhip
    vkl = V.vk_limbs(V.statements(n_inputs)[0])
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    al, be, de, abc, inp, pr, w = c(vkl["alpha"]), c(vkl["beta"]), c(vkl["delta"]), c(vkl["ABC"]), c(inputs), c(proofs), rho_words(rhos)
    count = len(pr)
    invalid, stats, value = np.zeros(count, dtype=np.uint8), zkhip.LocateStats(), np.zeros((6, 12), dtype=np.uint64)
    cap = 4096
    trace = (zkhip.LocateNode * cap)()
    n = shim.located_host(al.ctypes.data, be.ctypes.data, de.ctypes.data, abc.ctypes.data, n_inputs, inp.ctypes.data, pr.ctypes.data, count,
                          w.ctypes.data, threads, invalid.ctypes.data, ctypes.byref(stats), trace, cap, value.ctypes.data)
    assert 0 <= n <= cap, n
    nodes = [dict(chunk=int(t.chunk), level=int(t.level), index=int(t.index), passed=bool(t.passed), value=V.fq6_ints(np.array(t.value, dtype=np.uint64)))
             for t in trace[:n]]
    return invalid.astype(bool), stats.fields(), nodes, V.fq6_ints(value)


def check_trace(nodes, count, n_inputs, ks, rhos):
    """every node's value is g^(sum k_i rho_i over its range), it passed iff that is one, and a node's value is the product of its
    children's wherever they were tested; returns the nodes by (level, index).  One chunk."""
    by = {(t["level"], t["index"]): t for t in nodes}
    assert len(by) == len(nodes) and all(t["chunk"] == 0 for t in nodes)
    for (level, index), t in by.items():
        lo, hi = index * STRIP ** level, min((index + 1) * STRIP ** level, count)
        assert t["value"] == C.expected_value(n_inputs, ks[lo:hi], rhos[lo:hi]), (level, index)
        assert t["passed"] == (t["value"] == ONE), (level, index)
        kids = [by[(level - 1, s)] for s in range(index * STRIP, (index + 1) * STRIP) if (level - 1, s) in by] if level else []
        if kids:
            assert not t["passed"]
            prod = ONE
            for kid in kids:
                prod = V.EXT.mul(prod, kid["value"])
            assert prod == t["value"], (level, index)
    return by


@pytest.mark.parametrize("n_inputs,count", [(0, 9), (4, 9), (4, 65)])
def test_host_route_locates_tampered_proofs_and_every_node_has_its_value(shim, n_inputs, count):
    rhos = C.scalars(count, seed=count + n_inputs)
    depth = len(level_sizes(count)) - 1
    for tampered in ({0: 1}, {7: 2}, {8: 3}, {count - 1: 1}, {3: 1, count - 2: -2}):
        inp, prf, ks = C.batch(n_inputs, count, tampered)
        invalid, st, nodes, value = _located_host(shim, n_inputs, inp, prf, rhos)
        assert [i for i in range(count) if invalid[i]] == sorted(tampered), tampered
        assert value == C.expected_value(n_inputs, ks, rhos) != ONE
        by = check_trace(nodes, count, n_inputs, ks, rhos)
        assert st["finish_proofs"] == 0 and st["rounds"] == depth + 1 and st["node_tests"] == len(nodes) and st["chunks_failed"] == 1
        assert by[(depth, 0)]["value"] == value
        assert {i for (lv, i), t in by.items() if lv == 0 and not t["passed"]} == set(tampered)
        if len(tampered) == 1:
            assert st["node_tests"] == path_fanouts(count, min(tampered))
    inp, prf, ks = C.batch(n_inputs, count)
    invalid, st, nodes, value = _located_host(shim, n_inputs, inp, prf, rhos, threads=3)
    assert not invalid.any() and nodes == [] and value == ONE and st["rounds"] == st["node_tests"] == 0


def test_groth16_verify_batch_located_on_the_host():
    """The public host entry through the library, no device: the verdicts of a batch with tampered proofs, with supplied and with drawn
    scalars; an all-valid and an empty batch; a proof with a point off its curve gets 0 and does not disturb the others; a zero scalar is
    ZKHIP_ERR_ARG.  Equal scalars let C + D and C - D cancel in the batch's value - which is why supplied scalars prove nothing."""
    from oracle import pyref as R
    from tests.helpers import aff_limbs
    from zecale_amd import zkhip
    vkl = V.vk_limbs(V.statements(4)[0])
    inp, prf, ks = C.batch(4, 9, {2: 1, 8: -1})
    want = [k == 0 for k in ks]
    ok, st = zkhip.groth16_verify_batch_located(vkl, inp, prf, C.scalars(9))
    # (the library deals a round to the machine's threads, and the rule counts them: how far it descends is not asserted here)
    assert list(ok) == want and st["invalid"] == 2 and st["chunks_failed"] == 1 and st["rounds"] >= 2
    ok, st = zkhip.groth16_verify_batch_located(vkl, inp, prf)
    assert list(ok) == want and st["invalid"] == 2
    ok, st = zkhip.groth16_verify_batch_located(vkl, inp, prf, [77] * 9)
    assert ok.all() and st["rounds"] == 0
    good_in, good_pr, _ = C.batch(4, 9)
    ok, st = zkhip.groth16_verify_batch_located(vkl, good_in, good_pr)
    assert ok.all() and st["rounds"] == st["node_tests"] == st["invalid"] == 0
    ok, st = zkhip.groth16_verify_batch_located(vkl, good_in[:0], good_pr[:0])
    assert len(ok) == 0 and st["rounds"] == 0
    off = prf.copy(); off[4, 48:72] = aff_limbs((R.G1_GEN[0], (R.G1_GEN[1] + 1) % R.Q_MOD))
    ok, st = zkhip.groth16_verify_batch_located(vkl, inp, off, C.scalars(9))
    assert list(ok) == [w and i != 4 for i, w in enumerate(want)] and st["invalid"] == 2
    with pytest.raises(zkhip.ZkhipError) as e:
        zkhip.groth16_verify_batch_located(vkl, inp, prf, [3, 0, 5, 6, 7, 8, 9, 10, 11])
    assert e.value.code == -1
