"""Located batches on the GPU (zkhip_verifier_verify_batch_located: the combined check's kernels with every level of their trees
retained, k_tree_nodes_abi for the nodes of a round, and the descent of zecale_amd/csrc/locate.hpp) against the per-proof route, the
host route it is pinned on and the Python values of tests/combine_fixtures.py.  A tampered proof has C + k D and pairing product g^k,
so a node over the proofs [lo, hi) has the value g^(sum k_i rho_i over the range) - compared as a VALUE for every node tested.
STRIP values form a strip of either tree and CHUNK proofs a launch sequence with trees of its own: the batch sizes sit on both sides
of each."""
import numpy as np
import pytest

from tests import combine_fixtures as C
from tests import point_check_fixtures as F
from tests import verify_fixtures as V

pytestmark = pytest.mark.gpu

STRIP, CHUNK = 8, 16384
COUNTS = (1, 8, 9, 64, 65, 513)
N = 4
ONE = V.EXT.one()


@pytest.fixture(scope="module")
def handles(zk):
    h = {"plain": zk.Verifier(V.vk_limbs(V.statements(N)[0])), "checked": zk.Verifier(V.vk_limbs(V.statements(5)[0]), checked=True)}
    yield h
    for v in h.values():
        v.free()


def depth(count):
    """launches of a reduction tree over count values = the level of its root"""
    d = 1
    while -(-count // STRIP) > 1:
        count, d = -(-count // STRIP), d + 1
    return d


def bad_sets(count):
    """the placements of tests/test_locate_model.py: none; first; last; the end of one strip and the start of the next; two in one strip;
    a whole strip; the lone node of a ragged last strip; all"""
    sets = {"none": set(), "first": {0}, "last": {count - 1}, "all": set(range(count))}
    if count > STRIP:
        sets.update({"7 and 8": {7, 8}, "two in one strip": {1, 5}, "a whole strip": set(range(STRIP))})
    if count % STRIP == 1 and count > 1:
        sets["ragged last strip"] = {count - 1}
    return sets


# ---------------------------------------------------------------- verdicts equal to the per-proof route
@pytest.mark.parametrize("count", COUNTS)
def test_verdicts_equal_verify_batch(zk, handles, count):
    v = handles["plain"]
    for name, bad in bad_sets(count).items():
        inp, prf, ks = C.batch(N, count, {p: 1 + p % 3 for p in bad})
        want = v.verify_batch(inp, prf)
        assert list(want) == [k == 0 for k in ks], name
        got = v.verify_batch_located(inp, prf)
        assert got.dtype == want.dtype and list(got) == list(want), name
        st = v.last_locate_stats()
        assert st["invalid"] == len(bad) and (st["rounds"] > 0) == bool(bad), (name, st)


@pytest.mark.parametrize("count", COUNTS)
def test_codes_and_masks_equal_verify_batch_checked(zk, handles, count):
    v = handles["checked"]
    for name, bad in bad_sets(count).items():
        inp, prf, ks = C.batch(5, count, {p: 1 + p % 3 for p in bad})
        want = v.verify_batch_checked(inp, prf)
        assert list(want[0]) == [F.REJECT if k else F.ACCEPT for k in ks] and not want[1].any(), name
        got = v.verify_batch_located(inp, prf)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and (a == b).all(), name


def test_chunk_boundary_with_a_tampered_proof_on_each_side(zk, handles):
    """CHUNK + 1 proofs: two chunks, the second of one proof; tampered at the last index of the first chunk and at the first of the
    second.  Both chunk roots fail - every node of the chunk round - so the rule widens what is left and hands the batch over."""
    v, count = handles["plain"], CHUNK + 1
    inp, prf, ks = C.batch(N, count, {CHUNK - 1: 1, CHUNK: 2})
    got = v.verify_batch_located(inp, prf)
    st = v.last_locate_stats()
    want = v.verify_batch(inp, prf)
    assert (got == want).all() and [i for i in range(count) if not got[i]] == [CHUNK - 1, CHUNK]
    assert st["chunks_failed"] == 2 and st["invalid"] == 2 and st["rounds"] == 1 and st["finish_proofs"] == count
    trace = zk.locate_trace(v)
    assert [(t["chunk"], t["level"], t["index"], t["passed"]) for t in trace] == [(0, depth(CHUNK), 0, False), (1, 1, 0, False)]
    # tampered in the second chunk alone: one root of two fails, and its descent ends in the chunk's only leaf
    inp, prf, ks = C.batch(N, count, {CHUNK: 2})
    got = v.verify_batch_located(inp, prf)
    st = v.last_locate_stats()
    assert [i for i in range(count) if not got[i]] == [CHUNK] and st["chunks_failed"] == 1 and st["finish_proofs"] == 0 and st["rounds"] == 2
    assert [(t["chunk"], t["level"], t["index"], t["passed"]) for t in zk.locate_trace(v)] == [(0, depth(CHUNK), 0, True), (1, 1, 0, False), (1, 0, 0, False)]


def test_checked_batch_with_refused_and_tampered_proofs(zk, handles):
    """One refused proof of each class beside a tampered one: the refused proofs get their bytes, are left out of every node and every
    sum - the nodes' values are those of the tampered proof alone - and the tampered proof gets REJECT."""
    v = handles["checked"]
    ref = F.refused_cases(5)
    refused = {2: ref["a"][6], 11: ref["b"][4], 17: ref["c"][0]}
    assert [c.want & 0x0F for c in refused.values()] == [F.ENCODING, F.OFF_CURVE, F.NOT_ORDER_R]
    count, bad = 19, 12
    inp, prf, ks = C.batch(5, count, {bad: 1})
    want = [0] * count
    want[bad] = F.REJECT
    for pos, case in refused.items():
        inp[pos], prf[pos], want[pos] = case.inputs, case.proof, case.want
    rhos = C.scalars(count, seed=4)
    for route in ("gpu", "host"):
        (codes, masks), _ = zk.verify_batch_located_value(route, v, inp, prf, rhos)
        assert [int(c | m) for c, m in zip(codes, masks)] == want, route
        st = v.last_locate_stats()
        assert st["invalid"] == 1 and st["finish_proofs"] == 0 and st["rounds"] == depth(count) + 1, route
        for t in zk.locate_trace(v):
            lo, hi = t["index"] * STRIP ** t["level"], min((t["index"] + 1) * STRIP ** t["level"], count)
            assert V.fq6_ints(t["value"]) == (V.EXT.pow(list(C.g(5)), rhos[bad]) if lo <= bad < hi else ONE), (route, t["level"], t["index"])
    for a, b in zip(v.verify_batch_located(inp, prf), v.verify_batch_checked(inp, prf)):
        assert (a == b).all()


# ---------------------------------------------------------------- the descent ran
def test_one_tampered_proof_among_513_is_found_by_the_descent(zk, handles):
    v, count = handles["plain"], 513
    inp, prf, ks = C.batch(N, count, {300: 1})
    got = v.verify_batch_located(inp, prf)
    st = v.last_locate_stats()
    assert [i for i in range(count) if not got[i]] == [300]
    assert st["finish_proofs"] == 0 and st["rounds"] == depth(count) + 1 == 5 and st["invalid"] == 1 and st["chunks_failed"] == 1
    assert st["node_tests"] == 1 + 2 + 8 + 8 + 8 and st["finish_ms"] == 0 and st["descent_ms"] > 0


def test_all_tampered_go_to_the_per_proof_route(zk, handles):
    v, count = handles["plain"], 513
    inp, prf, ks = C.batch(N, count, {p: 1 + p % 3 for p in range(count)})
    got = v.verify_batch_located(inp, prf)
    st = v.last_locate_stats()
    assert not got.any() and st["finish_proofs"] == count and st["invalid"] == count and st["finish_ms"] > 0


# ---------------------------------------------------------------- by value
@pytest.mark.parametrize("count,bad", [(65, 0), (65, 7), (65, 8), (65, 64), (513, 512), (9, 8)])
def test_every_node_has_the_host_routes_value(zk, handles, count, bad):
    """Tampered first; at the end of a strip; at the start of the next; in the ragged last strip (of one node); last.  Every node the
    device route tested has, limb for limb, the value the host route gives it, and that is g^(sum k_i rho_i) over its range."""
    v = handles["plain"]
    rhos = C.scalars(count, seed=count + bad)
    inp, prf, ks = C.batch(N, count, {bad: 2})
    got, value = zk.verify_batch_located_value("gpu", v, inp, prf, rhos)
    gpu, gpu_st = zk.locate_trace(v), v.last_locate_stats()
    host_got, host_value = zk.verify_batch_located_value("host", v, inp, prf, rhos)
    host, host_st = zk.locate_trace(v), v.last_locate_stats()
    assert (got == host_got).all() and [i for i in range(count) if not got[i]] == [bad] and (got == v.verify_batch_located(inp, prf, rho=rhos)).all()
    assert (value == host_value).all() and (value == zk.verify_all_value("gpu", v, inp, prf, rhos)).all()
    assert len(gpu) == len(host) == gpu_st["node_tests"] == host_st["node_tests"] and gpu_st["rounds"] == host_st["rounds"] == depth(count) + 1
    g2 = V.EXT.pow(list(C.g(N)), 2 * rhos[bad])
    for a, b in zip(gpu, host):
        key = (a["chunk"], a["level"], a["index"], a["passed"])
        assert key == (b["chunk"], b["level"], b["index"], b["passed"])
        assert (a["value"] == b["value"]).all(), key
        lo, hi = a["index"] * STRIP ** a["level"], min((a["index"] + 1) * STRIP ** a["level"], count)
        assert V.fq6_ints(a["value"]) == (g2 if lo <= bad < hi else ONE) and a["passed"] == (not lo <= bad < hi), key
    assert (0, 0, bad, False) in [(a["chunk"], a["level"], a["index"], a["passed"]) for a in gpu]


def test_several_tampered_proofs_by_value(zk, handles):
    """Tamperings in two subtrees: every node's value is g^(sum k_i rho_i) over its own range, so no node holds another's proofs."""
    v, count = handles["plain"], 65
    rhos = C.scalars(count, seed=2)
    inp, prf, ks = C.batch(N, count, {3: 1, 5: -2, 40: 3, 64: 1})
    got = v.verify_batch_located(inp, prf, rho=rhos)
    assert [i for i in range(count) if not got[i]] == [3, 5, 40, 64]
    for t in zk.locate_trace(v):
        lo, hi = t["index"] * STRIP ** t["level"], min((t["index"] + 1) * STRIP ** t["level"], count)
        assert V.fq6_ints(t["value"]) == C.expected_value(N, ks[lo:hi], rhos[lo:hi]), (t["level"], t["index"])


# ---------------------------------------------------------------- an all-valid batch
def test_all_valid_batch(zk, handles):
    v, count = handles["plain"], 65
    rhos = C.scalars(count, seed=8)
    inp, prf, _ = C.batch(N, count)
    got = v.verify_batch_located(inp, prf, rho=rhos)
    st = v.last_locate_stats()
    assert got.dtype == np.bool_ and got.all()
    assert st["rounds"] == st["node_tests"] == st["finish_proofs"] == st["invalid"] == st["chunks_failed"] == 0
    assert zk.locate_trace(v) == []
    # the same value as verify_all's under the same scalars: one
    got, value = zk.verify_batch_located_value("gpu", v, inp, prf, rhos)
    assert got.all() and (value == zk.verify_all_value("gpu", v, inp, prf, rhos)).all() and V.fq6_ints(value) == ONE
    # and on a tampered batch, where the root carries it in the trace as well
    inp, prf, ks = C.batch(N, count, {9: 1})
    _, value = zk.verify_batch_located_value("gpu", v, inp, prf, rhos)
    root = zk.locate_trace(v)[0]
    assert (root["level"], root["index"]) == (depth(count), 0)
    assert (root["value"] == value).all() and (value == zk.verify_all_value("gpu", v, inp, prf, rhos)).all() and V.fq6_ints(value) != ONE
    c = handles["checked"]
    good_in, good_pr, _ = C.batch(5, 17)
    codes, masks = c.verify_batch_located(good_in, good_pr)
    assert not codes.any() and not masks.any() and c.last_locate_stats()["rounds"] == 0
    empty = v.verify_batch_located(inp[:0], prf[:0])
    assert len(empty) == 0


# ---------------------------------------------------------------- through verify_batch_combined
def test_verify_batch_combined_with_locate(zk, handles):
    v, count = handles["plain"], 17
    inp, prf, ks = C.batch(N, count, {0: 1, 7: 2, count - 1: 3})
    a, b = v.verify_batch_combined(inp, prf, locate=True), v.verify_batch_combined(inp, prf, locate=False)
    assert a.dtype == b.dtype and list(a) == list(b) == [k == 0 for k in ks]
    assert list(v.verify_batch_combined(inp, prf)) == list(b)
    c = handles["checked"]
    inp, prf, ks = C.batch(5, count, {3: 1})
    for x, y in zip(c.verify_batch_combined(inp, prf, locate=True), c.verify_batch_combined(inp, prf, locate=False)):
        assert x.dtype == y.dtype and (x == y).all()
