"""The combined (random-combination) check of a whole batch of nested (BLS12-377) proofs on the GPU (zkhip_nested_verifier_verify_all:
k_nested_rho_scale, the one-pair Miller loop, k_nested_gt_product and k_nested_g1_sum of zecale_amd/csrc/pairing_bls.hip, and the host
finish) against the host route it is pinned on and the value of tests/nested_combine_fixtures.py.  Batches repeat the cached statements
of a key; a tampered proof has C + k D, its pairing product is g^k, so a batch's combined value is g^(sum k_i rho_i) - compared as a
VALUE: an all-valid batch has value one whatever a reduction drops or repeats.  G = 4 verifications share a wave and WG = 8 a workgroup
of the Miller loop, STRIP values form a strip of either reduction tree, CHUNK proofs a launch sequence: the batch sizes sit on both
sides of each."""
import numpy as np
import pytest

from oracle import pyref as R
from tests import nested_combine_fixtures as C
from tests import nested_point_check_fixtures as F
from tests import nested_verify_fixtures as N

pytestmark = pytest.mark.gpu

G, STRIP, WG, CHUNK = 4, 8, 8, 8192
COUNTS = tuple(sorted({1, 2, G + 1, STRIP - 1, STRIP, STRIP + 1, WG + 1, STRIP * STRIP + 1}))
K = 3                                   # inputs of the key most tests use
ONE = N.EXT.one()
ORDER_TWO = (N.Q - 1, 0)


@pytest.fixture(scope="module")
def handles(zk):
    keys = {n: N.vk_limbs(C.source(n)[0]) for n in (0, K, 9)}
    h = {n: zk.NestedVerifier(keys[n], n) for n in (0, K, 9)}
    h["checked"] = zk.NestedVerifier(keys[K], K, checked=True)
    yield h
    for v in h.values():
        v.free()


def test_constants(zk):
    assert (zk.NESTED_VERIFIER_STRIP, zk.NESTED_VERIFIER_WORKGROUP, zk.NESTED_VERIFIER_CHUNK) == (STRIP, WG, CHUNK)


def _placements(count):
    """the first position, the last, the last element of a strip and the first of the next"""
    return sorted({0, count - 1} | {p for p in (STRIP - 1, STRIP) if p < count})


def _values(zk, v, inp, prf, rhos):
    gpu, host = zk.nested_verify_all_value("gpu", v, inp, prf, rhos), zk.nested_verify_all_value("host", v, inp, prf, rhos)
    assert (gpu == host).all()
    return N.fq12_ints(gpu)


# ---------------------------------------------------------------- 1, 2: values and verdicts
@pytest.mark.parametrize("count", COUNTS)
def test_value_and_verdict_with_a_tampered_proof_at_every_placement(zk, handles, count):
    """Explicit, pairwise different scalars.  With the tampered proof at position p the device's value equals the host route's limb
    for limb and g^(rho_p): a tree that drops, repeats or misplaces position p gives another power.  Verdict 0 there, 1 for the
    all-valid batch with supplied and with drawn scalars; the counter of degenerate line schedules and last_fallbacks stay 0."""
    v, rhos = handles[K], C.scalars(count, seed=count)
    assert len(set(rhos)) == count and 0 not in rhos
    for p in _placements(count):
        inp, prf, ks = C.batch(K, count, {p: 1})
        got = _values(zk, v, inp, prf, rhos)
        assert got == C.expected_value(K, ks, rhos) == N.EXT.pow(list(C.g(K)), rhos[p]) != ONE, (count, p)
        assert v.verify_all(inp, prf, rho=rhos) is False, (count, p)
        assert v.verify_all(inp, prf) is False, (count, p)
    inp, prf, _ = C.batch(K, count)
    assert N.fq12_ints(zk.nested_verify_all_value("gpu", v, inp, prf, rhos)) == ONE
    assert v.verify_all(inp, prf, rho=rhos) is True
    assert v.verify_all(inp, prf) is True
    assert v.last_degenerate() == 0 and v.last_fallbacks() == 0


def test_several_tampered_proofs_no_inputs_and_nine_inputs(zk, handles):
    """Every position's scalar reaches the value: tamperings k_i at many positions of a three-level batch give g^(sum k_i rho_i), on the
    three-input key, on the key without inputs (no input sums, S_acc = sigma ABC_0) and on tests/golden/nested_k9.json's key for nine."""
    count = STRIP * STRIP + 1
    rhos = C.scalars(count, seed=5)
    for n in (K, 0, 9):
        tampered = {p: 1 + p % 5 for p in range(0, count, 3)}
        inp, prf, ks = C.batch(n, count, tampered)
        assert _values(zk, handles[n], inp, prf, rhos) == C.expected_value(n, ks, rhos) != ONE, n
        inp, prf, _ = C.batch(n, WG + 1)
        assert handles[n].verify_all(inp, prf) is True, n


def test_empty_batch(zk, handles):
    v = handles[K]
    assert v.verify_all(np.zeros((0, K, 6), dtype=np.uint64), np.zeros((0, 48), dtype=np.uint64)) is True
    assert v.verify_all(np.zeros((0, K, 6), dtype=np.uint64), np.zeros((0, 48), dtype=np.uint64), rho=[]) is True


# ---------------------------------------------------------------- 3: why the scalars matter
def test_equal_scalars_let_two_tamperings_cancel(zk, handles):
    """C + D and C - D: under EQUAL supplied scalars the errors cancel, the value is one and the verdict 1 - which is why a caller's
    scalars prove nothing; under different scalars, and under drawn ones, the verdict is 0.  The value g^(rho_0 - rho_2) pins that the
    same rho_i scales A, C and the input sums of proof i."""
    v = handles[K]
    inp, prf, ks = C.batch(K, 3, {0: 1, 2: -1})
    assert _values(zk, v, inp, prf, [77, 5, 77]) == ONE
    assert v.verify_all(inp, prf, rho=[77, 5, 77]) is True
    assert _values(zk, v, inp, prf, [77, 5, 78]) == C.expected_value(K, ks, [77, 5, 78]) != ONE
    assert v.verify_all(inp, prf, rho=[77, 5, 78]) is False
    assert v.verify_all(inp, prf) is False


# ---------------------------------------------------------------- 4: the group law's edges in the sum tree
def test_group_law_edges_in_the_sum_tree(zk, handles):
    v = handles[K]
    rho = 0xF00DFACE0123456789ABCDEF02468ACE
    inp, prf, _ = C.batch(K, 2, {0: 1})
    # the same proof twice with the same scalar: the sum tree doubles; value g^(2 rho)
    twice_in, twice_pr = np.array([inp[0], inp[0]]), np.array([prf[0], prf[0]])
    assert _values(zk, v, twice_in, twice_pr, [rho, rho]) == N.EXT.pow(list(C.g(K)), 2 * rho % R.BLS_R) != ONE
    # a proof and its copy with C negated under the same scalar: the partial sum is the point at infinity
    neg = prf[1].copy(); neg[36:] = N.g1_limbs(N.g1neg(C.source(K)[1][1][0]["c"]))
    pair_in, pair_pr = np.array([inp[1], inp[1]]), np.array([prf[1], neg])
    assert _values(zk, v, pair_in, pair_pr, [rho, rho]) != ONE
    assert _values(zk, v, np.array([inp[0], inp[1], inp[1]]), np.array([prf[0], prf[1], neg]), [3, rho, rho]) != ONE
    # A = (-1, 0), of order 2, under an even scalar: rho A = O, the pair contributes one on the device as on the host; under an odd one
    # the point goes through the Miller loop
    two = prf[1].copy(); two[:12] = N.g1_limbs(ORDER_TWO)
    for r in (rho, rho + 1):
        assert _values(zk, v, inp[1:2], two[None], [r]) != ONE
        assert _values(zk, v, np.array([inp[1], inp[0], inp[1]]), np.array([two, prf[0], two]), [r, 9, r + 2]) != ONE
    assert v.verify_all(inp[1:2], two[None]) is False


def test_points_off_their_curves_fail_the_batch_and_are_left_out(zk, handles):
    """An unchecked handle: A, B or C with a coordinate + 1, or all zero (the nested format has no infinity): the proof fails the batch
    and is left out of the value, which equals the host route's and runs over the other proofs alone."""
    v, count = handles[K], WG + 2
    rhos = C.scalars(count, seed=12)
    inp, prf, ks = C.batch(K, count, {2: 1})
    want = C.expected_value(K, ks, rhos)
    for pos, lo, hi in ((0, 0, 6), (5, 12, 18), (count - 1, 42, 48)):
        bad = prf.copy(); bad[pos, lo:hi] = N.fl(N.fint(prf[pos, lo:hi]) + 1)
        assert _values(zk, v, inp, bad, rhos) == want, pos
        assert v.verify_all(inp, bad, rho=rhos) is False
    for lo, hi in ((0, 12), (12, 36), (36, 48)):
        bad = prf.copy(); bad[7, lo:hi] = 0
        assert _values(zk, v, inp, bad, rhos) == want, lo
    good_in, good_pr, _ = C.batch(K, count)
    bad = good_pr.copy(); bad[count - 1, 36:48] = 0
    assert _values(zk, v, good_in, bad, rhos) == ONE                   # valid apart from the proof left out ...
    assert v.verify_all(good_in, bad, rho=rhos) is False               # ... and still failed
    assert v.last_degenerate() == 0


# ---------------------------------------------------------------- 5: the chunk boundary
def test_chunk_boundary(zk, handles):
    """CHUNK + 1 proofs, tampered only at index CHUNK (a second chunk of one proof): the value is g^(2 rho_CHUNK), the verdict 0; the
    same batch untampered passes."""
    v, count = handles[K], CHUNK + 1
    rhos = C.rho_words(C.scalars(count, seed=3))
    rho_last = int(rhos[CHUNK, 0]) | int(rhos[CHUNK, 1]) << 64
    inp, prf, ks = C.batch(K, count, {CHUNK: 2})
    assert N.fq12_ints(zk.nested_verify_all_value("gpu", v, inp, prf, rhos)) == N.EXT.pow(list(C.g(K)), 2 * rho_last % R.BLS_R) != ONE
    assert v.verify_all(inp, prf) is False
    inp, prf, _ = C.batch(K, count)
    assert v.verify_all(inp, prf) is True


# ---------------------------------------------------------------- 6: the checked handle
def _checked_batch():
    """valid proofs, one tampered (nothing refuses it: the pairing rejects it), and refused ones of every class at the first, the last
    and middle positions; (inputs, proofs, ks, refusal bytes wanted)"""
    ref = F.refused_cases(K)
    refused = {0: ref["a"][0], 3: ref["b"][4], 4: ref["c"][6], 8: ref["inputs"][0], 9: ref["mixed"][4], 12: ref["a"][2], 18: ref["c"][1]}
    count = 19
    inp, prf, ks = C.batch(K, count, {6: 1})
    want = [0] * count
    for pos, case in refused.items():
        inp[pos], prf[pos], want[pos] = case.inputs, case.proof, case.want
    return inp, prf, ks, want


def test_checked_handle_leaves_refused_proofs_out(zk, handles):
    v = handles["checked"]
    inp, prf, ks, want = _checked_batch()
    count = len(prf)
    rhos = C.scalars(count, seed=6)
    codes, masks = v.verify_batch_checked(inp, prf)
    bytes_pp = [int(c | m) for c, m in zip(codes, masks)]
    assert [b if b >= 2 else 0 for b in bytes_pp] == want and bytes_pp[6] == F.REJECT
    ok, status = v.verify_all(inp, prf, rho=rhos, status=True)
    assert ok is False and list(status) == want
    assert v.verify_all(inp, prf, status=True) == (False, bytes(want))
    # the value runs over the proofs nothing refuses: the tampered one alone is not one
    assert _values(zk, v, inp, prf, rhos) == N.EXT.pow(list(C.g(K)), rhos[6]) != ONE
    # without the tampered proof the product over the unflagged proofs IS one - and the batch still fails, for its refused proofs
    inp2, prf2 = inp.copy(), prf.copy()
    inp2[6], prf2[6] = C.batch(K, 7)[0][6], C.batch(K, 7)[1][6]
    assert _values(zk, v, inp2, prf2, rhos) == ONE
    assert v.verify_all(inp2, prf2, rho=rhos, status=True) == (False, bytes(want))
    # an all-valid batch on the checked handle
    good_in, good_pr, _ = C.batch(K, WG + 1)
    assert v.verify_all(good_in, good_pr, status=True) == (True, bytes(WG + 1))
    assert v.verify_all(good_in, good_pr) is True
    assert v.verify_all(good_in[:0], good_pr[:0], status=True) == (True, b"")
    assert v.last_degenerate() == 0


def test_status_needs_a_checked_handle_and_scalars_must_not_be_zero(zk, handles):
    inp, prf, _ = C.batch(K, 3)
    with pytest.raises(zk.ZkhipError) as e:
        handles[K].verify_all(inp, prf, status=True)
    assert e.value.code == -4
    for v in (handles[K], handles["checked"]):
        with pytest.raises(zk.ZkhipError) as e:
            v.verify_all(inp, prf, rho=[5, 0, 7])
        assert e.value.code == -1


# ---------------------------------------------------------------- 7: degenerate statements
@pytest.mark.parametrize("x,negated,per_proof", [(4, False, False), (8, True, False)])
def test_degenerate_statements_are_accepted_by_the_group_law(zk, x, negated, per_proof):
    """Statements, valid by the group law, on which the host's affine accumulator meets +-2^2 ABC_1: verify_batch keeps its answer (the
    host's: 0) and hands them to the host (last_fallbacks counts them, on that route only); the combined route has no accumulator
    chain: value one, verify_all True, nothing handed over; verify_batch_combined is all ones."""
    vk, pr, xs = N.degenerate_statement(x, negated)
    items = [(pr, xs), N.degenerate_statement(3, negated)[1:], (pr, xs), N.degenerate_statement(5, negated)[1:], (pr, xs)]
    inp = np.array([N.input_limbs(i) for _, i in items], dtype=np.uint64).reshape(len(items), 1, 6)
    prf = np.array([N.proof_limbs(p) for p, _ in items], dtype=np.uint64)
    rhos = C.scalars(len(items), seed=x)
    v = zk.NestedVerifier(N.vk_limbs(vk), 1)
    try:
        assert list(v.verify_batch(inp, prf)) == [per_proof, True, per_proof, True, per_proof] and v.last_fallbacks() == 3
        assert _values(zk, v, inp, prf, rhos) == ONE
        assert v.last_fallbacks() == 3                                 # the combined route does not touch it
        assert v.verify_all(inp, prf, rho=rhos) is True and v.verify_all(inp, prf) is True
        assert v.last_degenerate() == 0 and v.last_fallbacks() == 3
        got = v.verify_batch_combined(inp, prf)
        assert got.dtype == np.bool_ and list(got) == [True] * len(items)
        assert list(v.verify_batch(inp, prf)) == [per_proof, True, per_proof, True, per_proof] and v.last_fallbacks() == 3
        wrong = inp.copy(); wrong[1] = N.input_limbs([6])
        assert v.verify_all(wrong, prf) is False
        assert list(v.verify_batch_combined(wrong, prf)) == list(v.verify_batch(wrong, prf)) == [per_proof, False, per_proof, True, per_proof]
    finally:
        v.free()


# ---------------------------------------------------------------- 8: one handle through a mixed sequence
def test_work_space_grows_and_is_reused_across_routes_on_one_handle(zk):
    """ONE fresh checked handle takes, in this order: verify_all with status at STRIP + 1 (the handle's first call: the combined route
    reserves its extra work space), verify_batch_checked at WG + 1, verify_all at 1, verify_batch at 2 WG + 1, verify_all with status
    at STRIP^2 + 1 - growing, shrinking, and changing the route that sizes the work space.  Every batch has a tampered proof in the
    middle and, from two proofs on, a refused one (an input >= r) at the end.  Every result equals that of the same call on a fresh
    handle of its own, and the bytes the checked calls give are the construction's."""
    key = N.vk_limbs(N.statements(K)[0])
    refused = F.refused_cases(K)["inputs"][0]
    calls = [("verify_all", STRIP + 1, True), ("verify_batch_checked", WG + 1, False), ("verify_all", 1, False), ("verify_batch", 2 * WG + 1, False),
             ("verify_all", STRIP * STRIP + 1, True)]

    def call(v, name, count, status):
        inp, prf, _ = C.batch(K, count, {count // 2: 1})
        if count > 1:
            inp[count - 1], prf[count - 1] = refused.inputs, refused.proof
        if name == "verify_all":
            out = v.verify_all(inp, prf, rho=C.scalars(count, seed=count), status=status)
            return (out[0], list(out[1])) if status else out
        if name == "verify_batch":
            return [bool(b) for b in v.verify_batch(inp, prf)]
        codes, masks = v.verify_batch_checked(inp, prf)
        return [int(c | m) for c, m in zip(codes, masks)]

    def bytes_wanted(count, tampered):
        want = [0] * count
        want[count // 2] = tampered
        if count > 1:
            want[count - 1] = refused.want
        return want

    shared = zk.NestedVerifier(key, K, checked=True)
    try:
        got = [call(shared, *c) for c in calls]
    finally:
        shared.free()
    for c, g in zip(calls, got):
        fresh = zk.NestedVerifier(key, K, checked=True)
        try:
            assert call(fresh, *c) == g, c
        finally:
            fresh.free()
    assert got[0] == (False, bytes_wanted(STRIP + 1, 0)) and got[4] == (False, bytes_wanted(STRIP * STRIP + 1, 0))
    assert got[1] == bytes_wanted(WG + 1, F.REJECT)
    assert got[2] is False and got[3][:2 * WG] == [j != WG for j in range(2 * WG)]


# ---------------------------------------------------------------- 9: per-proof verdicts by way of the combined check
def test_verify_batch_combined(zk, handles):
    v, count = handles[K], WG + 1
    inp, prf, ks = C.batch(K, count, {0: 1, 7: 2, count - 1: 3})
    want = v.verify_batch(inp, prf)
    assert list(want) == [k == 0 for k in ks]
    got = v.verify_batch_combined(inp, prf)
    assert got.dtype == want.dtype and list(got) == list(want)
    inp, prf, _ = C.batch(K, count)
    got = v.verify_batch_combined(inp, prf)
    assert got.dtype == np.bool_ and list(got) == [True] * count == list(v.verify_batch(inp, prf))
    # a checked handle: verify_batch_checked's codes and masks
    c = handles["checked"]
    inp, prf, _, _ = _checked_batch()
    for a, b in zip(c.verify_batch_combined(inp, prf), c.verify_batch_checked(inp, prf)):
        assert a.dtype == b.dtype and (a == b).all()
    good_in, good_pr, _ = C.batch(K, count)
    for a, b in zip(c.verify_batch_combined(good_in, good_pr), c.verify_batch_checked(good_in, good_pr)):
        assert a.dtype == b.dtype and (a == b).all() and not a.any()
