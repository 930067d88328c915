"""The adversarial MSM inputs of tests/msm_cases.py do what they claim (no GPU): the boundary scalars put the targeted signed digit
into every window of the recoding that k_digit_pass performs, the NAF worst cases are as dense as the width-(c+1) NAF allows, every
scalar is below r, and the C oracle's multi_exp equals the closed form on the degenerate structures - so that the GPU comparisons in
tests/test_msm_edges_gpu.py rest on an oracle known to be right on this input."""
import pytest

from oracle import pyref as R
from tests import msm_cases as M
from tests.helpers import aff_limbs

WINDOWS = (4, 5, 8, 9, 11, 12, 13, 16, 17, 18, 20, 21, 22)


@pytest.mark.parametrize("c", WINDOWS)
def test_window_layout_tiles_378_bits(c):
    lay = M.window_layout(c)
    assert len(lay) == -(-378 // c)
    assert lay[0][0] == 0 and lay[-1][0] + lay[-1][1] == 378
    assert all(o2 == o1 + b1 for (o1, b1), (o2, _) in zip(lay, lay[1:]))
    n_small = len(lay) * c - 378
    assert [b for _, b in lay] == [c] * (len(lay) - n_small) + [c - 1] * n_small


@pytest.mark.parametrize("c", WINDOWS)
def test_boundary_scalars_hit_their_digits(c):
    lay = M.window_layout(c)
    half = [1 << (cw - 1) for _, cw in lay]
    fam = M.boundary_scalars(c)
    for s in fam:
        assert 0 <= s < R.R_MOD
        ds = M.recode_plain(s, c)
        assert M.digits_value(ds) == s
        assert all(-h < d <= h for (_, d), h in zip(ds, half))      # the signed range of each window's width
    digits = lambda s: [d for _, d in M.recode_plain(s, c)]
    low = len(lay) - 1
    assert digits(fam[0])[:low] == half[:-1]                             # +2^(cw-1) everywhere
    assert digits(fam[1])[:low] == [-(h - 1) for h in half[:-1]]         # window value 2^(cw-1) + 1: negative, carry out
    assert digits(fam[2])[:low] == [-1] * low                            # window value 2^cw - 1 (+ carry): -1, carry out
    assert digits(fam[3])[:low] == [h - 1 for h in half[:-1]]            # the largest digit without a carry
    assert digits(fam[4]) == [-1] + [0] * (low - 1) + [1]                # one carry through every window into the top
    top_max = min(half[-1], (R.R_MOD - 1) >> lay[-1][0])
    assert digits(fam[6])[-1] == top_max and digits(fam[6])[0] == -1     # the carry lands on the top window's largest digit
    assert digits(fam[7]) == [0] * low + [top_max]
    if 378 % c:
        assert lay[-1][1] == c - 1                                       # a top window of c - 1 bits
    for s in fam[:4]:
        assert digits(s)[-1] > 0                                         # (the top digit keeps the scalar positive and below r)
    for v in M.tiny_values(c):
        assert 0 <= v < R.R_MOD


@pytest.mark.parametrize("c", (4, 5, 8, 9, 13, 16, 20, 21))
def test_naf_worst_cases(c):
    Wd = 378 // (c + 1) + 2
    for pos, ds in M.naf_dense_digits(c):
        s = sum(d << p for p, d in zip(pos, ds))
        assert 0 <= s < R.R_MOD
        assert M.recode_naf(s, c) == list(zip(pos, ds))                  # a digit at every (c + 1)-th bit, as targeted
        assert len(ds) >= 378 // (c + 1) - 1                             # within two of the most a scalar below r can have
    for s in M.naf_worst_scalars(c) + M.boundary_scalars(c) + M.tiny_values(c):
        assert 0 <= s < R.R_MOD
        nd = M.recode_naf(s, c)
        assert M.digits_value(nd) == s
        assert len(nd) <= Wd
        assert all(d % 2 == 1 and -(1 << c) < d < (1 << c) for _, d in nd)
        assert all(p2 - p1 >= c + 1 for (p1, _), (p2, _) in zip(nd, nd[1:]))
    runs = M.recode_naf((1 << 200) - 1, c)                               # an all-ones run: -1, then a carry to the run's end
    assert runs[0] == (0, -1) and runs[-1] == (200, 1) and len(runs) == 2


def test_small_multiples_are_the_multiples(oracle_lib):
    O = oracle_lib
    for g2 in (False, True):
        pts = M.small_multiples(O, g2)
        jac = lambda k: O.aff_to_jac(pts[k])
        g = pts[1]
        assert (g == aff_limbs(R.G2_GEN if g2 else R.G1_GEN)).all()
        assert (O.jac_to_affine(O.jac_dbl(jac(1))) == pts[2]).all()
        assert (O.jac_to_affine(O.jac_add(jac(2), jac(1))) == pts[3]).all()
        for k in (1, 2, 3):
            assert (O.jac_to_affine(O.jac_add(jac(k), jac(-k))) == 0).all()
            assert O.on_curve(pts[-k], g2=g2)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("structure", M.STRUCTURES)
def test_oracle_msm_equals_the_closed_form(oracle_lib, structure, g2):
    """The C oracle's multi_exp (both with_mixed settings) against (sum s_i k_i mod r) G on every structure, at a few thousand
    terms, with the scalar pool of windows 4, 9 and 16."""
    O = oracle_lib
    n = 3001
    pool = M.scalar_pool((4, 9, 16))
    ks, scal = M.make_case(structure, n, pool, seed=17, c=9)
    bases = M.bases_of(O, ks, g2)
    exp = M.closed_form(O, ks, scal, g2)
    sm = M.montgomery_limbs(scal)
    for mixed in (True, False):
        assert (O.jac_to_affine(O.msm(bases, sm, with_mixed=mixed)) == exp).all(), mixed


def test_structures_are_what_they_claim(oracle_lib):
    pool = M.scalar_pool((9,))
    ks, scal = M.make_case("cancel", 1000, pool, seed=3)
    from collections import Counter
    cnt = Counter(zip(ks, scal))
    assert all(cnt[(k, s)] == cnt[(-k, s)] for k, s in cnt)              # every (P, s) also as (-P, s): the sum is O
    assert sum(s * k for s, k in zip(scal, ks)) % R.R_MOD == 0
    ks, scal = M.make_case("runs", 1000, pool, seed=3)
    assert sum(1 for i in range(1, 1000) if (ks[i], scal[i]) == (ks[i - 1], scal[i - 1])) >= 500
    ks, scal = M.make_case("rows", 1000, pool, seed=3, c=9)
    assert set(ks) == {1} and sorted(set(scal)) == list(range(1, 257))
    ks, scal = M.make_case("signs", 1000, pool, seed=3)
    assert set(ks) == {1, -1}
