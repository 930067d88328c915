"""Opening a bucket from its first table point (ec_edw.cuh edw_open_lds_pre, the lockstep kernel's iteration 0), in the integer model
of tests/test_edwards_model.py: (X : Y : Z : T) = (ypx - ymx : ypx + ymx : 2 : t2d / d), a negated entry with its loads swapped and
t2d negated.  Followed by the mixed additions of the remaining entries it gives the point that the additions from the identity give."""
import itertools

import pytest

from tests import test_edwards_model as E
from tests.test_edwards_reduction_model import opening

q, D = E.q, E.D


def test_opening_then_additions_equals_additions_from_the_identity():
    pts = E.rand_points(31, 5)
    pres = [E.precomputed(E.chi(P)) for P in pts]
    for n in range(1, 6):
        for signs in itertools.product((False, True), repeat=n):
            ref = E.IDENTITY
            for pre, neg in zip(pres, signs):
                ref = E.madd_7m(ref, pre, neg)
            got = opening(pres[0], signs[0])
            for pre, neg in zip(pres[1:n], signs[1:]):
                got = E.madd_7m(got, pre, neg)
            assert E.e_affine(got) == E.e_affine(ref), (n, signs)


def test_opening_p_then_adding_minus_p_is_the_identity_as_an_ordinary_point():
    pre = E.precomputed(E.chi(E.rand_points(32, 1)[0]))
    other = E.precomputed(E.chi(E.rand_points(33, 1)[0]))
    for neg in (False, True):
        acc = E.madd_7m(opening(pre, neg), pre, not neg)
        assert acc[2] % q and E.e_affine(acc) == (0, 1)
        assert E.e_affine(E.madd_7m(acc, other)) == E.chi(E.rand_points(33, 1)[0])


def test_dinv_constant_is_the_generated_one():
    assert E._header_array("EDW_DINV", 27) == E.inv(D) * (1 << (29 * 27)) % q
    assert E._header_array("EDW_DINV", 27) * E._header_array("EDW_D2", 27) % q == 2 * (1 << (2 * 29 * 27)) % q


@pytest.mark.parametrize("neg", [False, True])
def test_stored_coordinates_stay_below_2p(neg):
    """the device forms X = ypx - ymx + p (fp_sub_k<1>) and Y = ypx + ymx from CANONICAL table words, without reduction: both must be
    below 2p, the bound step 0 of the addition (fp_sub<2>) asks of a stored coordinate; Z = 2 in Montgomery form likewise"""
    R = 1 << (29 * 27)
    worst = [(0, q - 1, 0), (q - 1, 0, 0), (q - 1, q - 1, 0), (0, 0, 0)]
    pres = [E.precomputed(E.chi(P)) for P in E.rand_points(34, 16)] + worst
    for ymx, ypx, _ in pres:
        assert 0 <= ymx < q and 0 <= ypx < q
        ymx_m, ypx_m = ymx * R % q, ypx * R % q            # the table's words: canonical Montgomery residues
        if neg:
            ymx_m, ypx_m = ypx_m, ymx_m
        X, Y = ypx_m - ymx_m + q, ypx_m + ymx_m
        assert 0 < X < 2 * q and 0 <= Y < 2 * q
        assert X % q == (ypx_m - ymx_m) % q
    assert 2 * (R % q) < 2 * q
