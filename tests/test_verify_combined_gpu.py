"""The combined (random-combination) check of a whole batch on the GPU (zkhip_verifier_verify_all: k_rho_scale, the one-pair Miller loop,
k_gt_product and k_g1_sum of zecale_amd/csrc/pairing.hip, and the host finish) against the host route it is pinned on and the Python
value of tests/combine_fixtures.py.  Batches repeat the eight cached statements of a key; a tampered proof has C + k D, its pairing
product is g^k, so a batch's combined value is g^(sum k_i rho_i) - compared as a VALUE: an all-valid batch has value one whatever a
reduction drops or repeats.  STRIP values form a strip of either reduction tree, WG = 16 proofs share a workgroup of the Miller loop,
CHUNK proofs a launch sequence: the batch sizes sit on both sides of each."""
import numpy as np
import pytest

from oracle import pyref as R
from tests import combine_fixtures as C
from tests import point_check_fixtures as F
from tests import verify_fixtures as V
from tests.helpers import aff_limbs

pytestmark = pytest.mark.gpu

STRIP, WG, CHUNK = 8, 16, 16384
COUNTS = (1, 2, WG + 1, STRIP - 1, STRIP, STRIP + 1, STRIP * STRIP + 1)
N = 4                                   # inputs of the key most tests use
ONE = V.EXT.one()


@pytest.fixture(scope="module")
def handles(zk):
    keys = {n: V.vk_limbs(V.statements(n)[0]) for n in (0, N, 5)}
    h = {n: zk.Verifier(keys[n]) for n in (0, N)}
    h["checked"] = zk.Verifier(keys[5], checked=True)
    h["unchecked5"] = zk.Verifier(keys[5])
    yield h
    for v in h.values():
        v.free()


def test_constants(zk):
    assert (zk.VERIFIER_STRIP, zk.VERIFIER_WORKGROUP, zk.VERIFIER_CHUNK) == (STRIP, WG, CHUNK)


def _placements(count):
    """the first position, the last, the last element of a strip and the first of the next"""
    return sorted({0, count - 1} | {p for p in (STRIP - 1, STRIP) if p < count})


def _values(zk, v, inp, prf, rhos):
    gpu, host = zk.verify_all_value("gpu", v, inp, prf, rhos), zk.verify_all_value("host", v, inp, prf, rhos)
    assert (gpu == host).all()
    return V.fq6_ints(gpu)


# ---------------------------------------------------------------- 1, 2: values and verdicts
@pytest.mark.parametrize("count", COUNTS)
def test_value_and_verdict_with_a_tampered_proof_at_every_placement(zk, handles, count):
    """Explicit, pairwise different scalars.  With the tampered proof at position p the device's value equals the host route's limb
    for limb and g^(rho_p): a tree that drops, repeats or misplaces position p gives another power.  Verdict 0 there, 1 for the
    all-valid batch with supplied and with drawn scalars."""
    v, rhos = handles[N], C.scalars(count, seed=count)
    assert len(set(rhos)) == count and 0 not in rhos
    for p in _placements(count):
        inp, prf, ks = C.batch(N, count, {p: 1})
        got = _values(zk, v, inp, prf, rhos)
        assert got == C.expected_value(N, ks, rhos) == V.EXT.pow(list(C.g(N)), rhos[p]) != ONE, (count, p)
        assert v.verify_all(inp, prf, rho=rhos) is False, (count, p)
        assert v.verify_all(inp, prf) is False, (count, p)
    inp, prf, _ = C.batch(N, count)
    assert V.fq6_ints(zk.verify_all_value("gpu", v, inp, prf, rhos)) == ONE
    assert v.verify_all(inp, prf, rho=rhos) is True
    assert v.verify_all(inp, prf) is True


def test_several_tampered_proofs_and_a_key_without_inputs(zk, handles):
    """Every position's scalar reaches the value: tamperings k_i at many positions of a three-level batch give g^(sum k_i rho_i); and the
    same on the key without inputs (no input sums, S_acc = sigma ABC_0)."""
    count = STRIP * STRIP + 1
    rhos = C.scalars(count, seed=5)
    for n in (N, 0):
        tampered = {p: 1 + p % 5 for p in range(0, count, 3)}
        inp, prf, ks = C.batch(n, count, tampered)
        assert _values(zk, handles[n], inp, prf, rhos) == C.expected_value(n, ks, rhos) != ONE
    inp, prf, _ = C.batch(0, WG + 1)
    assert handles[0].verify_all(inp, prf) is True


def test_empty_batch(zk, handles):
    v = handles[N]
    assert v.verify_all(np.zeros((0, N, 6), dtype=np.uint64), np.zeros((0, 72), dtype=np.uint64)) is True
    assert v.verify_all(np.zeros((0, N, 6), dtype=np.uint64), np.zeros((0, 72), dtype=np.uint64), rho=[]) is True


# ---------------------------------------------------------------- 3: why the scalars matter
def test_equal_scalars_let_two_tamperings_cancel(zk, handles):
    """C + D and C - D: under EQUAL supplied scalars the errors cancel, the value is one and the verdict 1 - which is why a caller's
    scalars prove nothing; under different scalars, and under drawn ones, the verdict is 0.  The value g^(rho_0 - rho_2) pins that the
    same rho_i scales A, C and the input sums of proof i."""
    v = handles[N]
    inp, prf, ks = C.batch(N, 3, {0: 1, 2: -1})
    assert _values(zk, v, inp, prf, [77, 5, 77]) == ONE
    assert v.verify_all(inp, prf, rho=[77, 5, 77]) is True
    assert _values(zk, v, inp, prf, [77, 5, 78]) == C.expected_value(N, ks, [77, 5, 78]) != ONE
    assert v.verify_all(inp, prf, rho=[77, 5, 78]) is False
    assert v.verify_all(inp, prf) is False


# ---------------------------------------------------------------- 4: the group law's edges in the sum tree
def test_group_law_edges_in_the_sum_tree(zk, handles):
    v = handles[N]
    rho = 0xF00DFACE0123456789ABCDEF02468ACE
    inp, prf, _ = C.batch(N, 2, {0: 1})
    # the same proof twice with the same scalar: the sum tree doubles; value gt^(2 rho)
    twice_in, twice_pr = np.array([inp[0], inp[0]]), np.array([prf[0], prf[0]])
    assert _values(zk, v, twice_in, twice_pr, [rho, rho]) == V.EXT.pow(list(C.g(N)), 2 * rho)
    # a proof and its copy with C negated under the same scalar: the partial sum is the point at infinity
    neg = prf[1].copy(); neg[48:] = aff_limbs(R.ec_neg(V.statements(N)[1][1][0]["c"]))
    pair_in, pair_pr = np.array([inp[1], inp[1]]), np.array([prf[1], neg])
    assert _values(zk, v, pair_in, pair_pr, [rho, rho]) != ONE
    assert _values(zk, v, np.array([inp[0], inp[1], inp[1]]), np.array([prf[0], prf[1], neg]), [3, rho, rho]) != ONE
    # all-zero C alone: S_C at infinity; all-zero A: its pair contributes 1
    for lo in (48, 0):
        zeroed = prf[1].copy(); zeroed[lo:lo + 24] = 0
        assert _values(zk, v, inp[1:2], zeroed[None], [rho]) != ONE
        assert _values(zk, v, np.array([inp[1], inp[0]]), np.array([zeroed, prf[0]]), [rho, 9]) != ONE
        assert v.verify_all(inp[1:2], zeroed[None]) is False


# ---------------------------------------------------------------- 5: the chunk boundary
def test_chunk_boundary(zk, handles):
    """CHUNK + 1 proofs, tampered only at index CHUNK (a second chunk of one proof): the value is g^(rho_CHUNK), the verdict 0; the same
    batch untampered passes."""
    v, count = handles[N], CHUNK + 1
    rhos = np.array([[r & (2 ** 64 - 1), r >> 64] for r in C.scalars(count, seed=3)], dtype=np.uint64)
    rho_last = int(rhos[CHUNK, 0]) | int(rhos[CHUNK, 1]) << 64
    inp, prf, ks = C.batch(N, count, {CHUNK: 2})
    assert V.fq6_ints(zk.verify_all_value("gpu", v, inp, prf, rhos)) == V.EXT.pow(list(C.g(N)), 2 * rho_last) != ONE
    assert v.verify_all(inp, prf) is False
    inp, prf, _ = C.batch(N, count)
    assert v.verify_all(inp, prf) is True


# ---------------------------------------------------------------- 6: the checked handle
def _checked_batch():
    """valid proofs, one tampered (nothing refuses it: the pairing rejects it), and refused ones of every class at the first, the last
    and middle positions; (inputs, proofs, ks, refusal bytes wanted)"""
    ref = F.refused_cases(5)
    refused = {0: ref["a"][0], 3: ref["b"][4], 4: ref["c"][6], 8: ref["inputs"][0], 9: ref["mixed"][4], 12: ref["a"][2], 18: ref["c"][1]}
    count = 19
    inp, prf, ks = C.batch(5, count, {6: 1})
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
    assert _values(zk, v, inp, prf, rhos) == V.EXT.pow(list(C.g(5)), rhos[6]) != ONE
    # without the tampered proof the product over the unflagged proofs IS one - and the batch still fails, for its refused proofs
    inp2, prf2 = inp.copy(), prf.copy()
    inp2[6], prf2[6] = C.batch(5, 7)[0][6], C.batch(5, 7)[1][6]
    assert _values(zk, v, inp2, prf2, rhos) == ONE
    assert v.verify_all(inp2, prf2, rho=rhos, status=True) == (False, bytes(want))
    # an all-valid batch on the checked handle
    good_in, good_pr, _ = C.batch(5, WG + 1)
    assert v.verify_all(good_in, good_pr, status=True) == (True, bytes(WG + 1))
    assert v.verify_all(good_in, good_pr) is True
    assert v.verify_all(good_in[:0], good_pr[:0], status=True) == (True, b"")


def test_status_needs_a_checked_handle_and_scalars_must_not_be_zero(zk, handles):
    inp, prf, _ = C.batch(5, 3)
    with pytest.raises(zk.ZkhipError) as e:
        handles["unchecked5"].verify_all(inp, prf, status=True)
    assert e.value.code == -4
    for v in (handles["unchecked5"], handles["checked"]):
        with pytest.raises(zk.ZkhipError) as e:
            v.verify_all(inp, prf, rho=[5, 0, 7])
        assert e.value.code == -1


def test_work_space_grows_and_is_reused_across_routes_on_one_handle(zk):
    """ONE fresh checked handle takes, in this order: verify_all with status at STRIP + 1 (the handle's first call: the combined route
    reserves the input buffer), verify_batch_checked at WG + 1, verify_all at 1, verify_batch at 2 WG + 1, verify_all with status at
    STRIP^2 + 1, verify_batch_checked at 1 - growing, shrinking, and changing the route that sizes the work space.  Every batch has a
    tampered proof in the middle and, from two proofs on, a refused one (an input >= r) at the end.  Every result equals that of the
    same call on a fresh handle of its own, and the bytes the checked calls give are the construction's."""
    key = V.vk_limbs(V.statements(5)[0])
    refused = F.refused_cases(5)["inputs"][0]
    calls = [("verify_all", STRIP + 1, True), ("verify_batch_checked", WG + 1, False), ("verify_all", 1, False), ("verify_batch", 2 * WG + 1, False),
             ("verify_all", STRIP * STRIP + 1, True), ("verify_batch_checked", 1, False)]

    def call(v, name, count, status):
        inp, prf, _ = C.batch(5, count, {count // 2: 1})
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

    shared = zk.Verifier(key, checked=True)
    try:
        got = [call(shared, *c) for c in calls]
    finally:
        shared.free()
    for c, g in zip(calls, got):
        fresh = zk.Verifier(key, checked=True)
        try:
            assert call(fresh, *c) == g, c
        finally:
            fresh.free()
    assert got[0] == (False, bytes_wanted(STRIP + 1, 0)) and got[4] == (False, bytes_wanted(STRIP * STRIP + 1, 0))
    assert got[1] == bytes_wanted(WG + 1, F.REJECT) and got[5] == [F.REJECT]
    assert got[2] is False and got[3][:2 * WG] == [j != WG for j in range(2 * WG)]


# ---------------------------------------------------------------- 7: per-proof verdicts by way of the combined check
def test_verify_batch_combined(zk, handles):
    v, count = handles[N], WG + 1
    inp, prf, ks = C.batch(N, count, {0: 1, 7: 2, count - 1: 3})
    want = v.verify_batch(inp, prf)
    assert list(want) == [k == 0 for k in ks]
    got = v.verify_batch_combined(inp, prf)
    assert got.dtype == want.dtype and list(got) == list(want)
    inp, prf, _ = C.batch(N, count)
    got = v.verify_batch_combined(inp, prf)
    assert got.dtype == np.bool_ and list(got) == [True] * count == list(v.verify_batch(inp, prf))
    # a checked handle: verify_batch_checked's codes and masks
    c = handles["checked"]
    inp, prf, _, _ = _checked_batch()
    for a, b in zip(c.verify_batch_combined(inp, prf), c.verify_batch_checked(inp, prf)):
        assert a.dtype == b.dtype and (a == b).all()
    good_in, good_pr, _ = C.batch(5, count)
    for a, b in zip(c.verify_batch_combined(good_in, good_pr), c.verify_batch_checked(good_in, good_pr)):
        assert a.dtype == b.dtype and (a == b).all() and not a.any()
