"""The bucket reduction of an Edwards launch, as a model in Python integers: psi commutes with it.  The device keeps the buckets on
the Edwards curve through the stitching and the two-level reduction (msm.hip, the k_..._edw kernels; ec_edw.cuh) and applies psi to
the one point per window that reaches the host (msm.hip edw_abi_to_jac) - psi is a homomorphism, so psi(sum (j + 1) E_j) =
sum (j + 1) psi(E_j).  An EMPTY bucket (all-zero words, None here) is skipped or copied over, never fed to a formula; the identity
(0 : Y : Y : 0) is an ordinary point."""
import os
import random
import re

import pytest

from tests import test_edwards_model as E

q, EP = E.q, E.EP
ROOT = E.ROOT


def e_add(a, b):
    """pt_add of the Edwards model: an empty operand is the neutral element (edw_add_mem, edw_add_mem_quad)"""
    if b is None:
        return a
    if a is None:
        return b
    return E.add_9m(a, b)


def e_dbl(a):
    return None if a is None else E.dbl_4m4s(a)


def weighted_sum_hilo(buckets, lo_bits):
    """sum_j (j + 1) B_j through the split j = hi R + lo of msm.hip: R sum_hi hi Row[hi] + sum_lo (lo + 1) Col[lo]; the two small
    weighted sums by running sums (k_seg), the factor R by doublings (k_hilo_combine)."""
    Rr = 1 << lo_bits
    H = len(buckets) // Rr
    rows = [None] * H
    cols = [None] * Rr
    for j, b in enumerate(buckets):
        rows[j // Rr] = e_add(rows[j // Rr], b)
        cols[j % Rr] = e_add(cols[j % Rr], b)

    def running(items):                     # sum_i (i + 1) items[i]: run and acc as in k_seg, from the top
        run = acc = None
        for it in reversed(items):
            run = e_add(run, it)
            acc = e_add(acc, run)
        return acc

    hi = running(rows[1:])                  # weights hi = 1 .. H - 1 (k_place_hilo drops row 0)
    lo = running(cols)
    for _ in range(lo_bits):
        hi = e_dbl(hi)
    return e_add(hi, lo)


def ext(P, z):
    x, y = E.chi(P)
    return x * z % q, y * z % q, z % q, x * y * z % q


def w_weighted_sum(points):
    tot = None
    for j, P in enumerate(points):
        if P is not None:
            tot = E.w_add(tot, E.w_mul(j + 1, P))
    return tot


def psi_or_none(e):
    return None if e is None else E.psi_xyzz(e)


def _case(kind, n, seed):
    """n buckets as (Weierstrass point the bucket stands for under psi, Edwards point); None = empty"""
    rng = random.Random(seed)
    pts = E.rand_points(seed, n)
    ed = [ext(P, rng.randrange(1, q)) for P in pts]
    w = [E.w_add(P, P) for P in pts]        # psi(chi(P)) = 2 P
    ident = (0, 5, 5, 0)                    # the identity as P + (-P) leaves it: Z = Y, not 1
    if kind == "random":
        pass
    elif kind == "sparse":
        for j in range(n):
            if rng.random() < 0.8:
                ed[j], w[j] = None, None
    elif kind == "all_empty":
        ed, w = [None] * n, [None] * n
    elif kind == "identity":
        for j in (0, 3, n - 1):
            ed[j], w[j] = ident, None
    elif kind == "equal_neighbours":
        ed, w = [ed[0]] * n, [w[0]] * n     # every addition of the trees is P + P
    elif kind == "p_minus_p":
        for j in range(0, n - 1, 2):
            X, Y, Z, T = ed[j]
            ed[j + 1], w[j + 1] = ((-X) % q, Y, Z, (-T) % q), E.w_neg(w[j])
    return w, ed


@pytest.mark.parametrize("kind", ["random", "sparse", "all_empty", "identity", "equal_neighbours", "p_minus_p"])
@pytest.mark.parametrize("lo_bits, hi_bits", [(2, 1), (2, 2), (3, 2)])
def test_psi_commutes_with_the_bucket_reduction(kind, lo_bits, hi_bits):
    n = 1 << (lo_bits + hi_bits)
    w, ed = _case(kind, n, 11 * lo_bits + hi_bits)
    got = weighted_sum_hilo(ed, lo_bits)
    assert psi_or_none(got) == w_weighted_sum(w)
    if got is not None:
        assert got[2] % q and (got[0] * got[1] - got[3] * got[2]) % q == 0      # a point: Z != 0, T = XY / Z


def test_an_all_zero_operand_would_poison_a_sum():
    """why empty slots are tested for and never added: the formulas turn (0, 0, 0, 0) + P into zeros"""
    P = ext(E.rand_points(1, 1)[0], 7)
    assert E.add_9m((0, 0, 0, 0), P) == (0, 0, 0, 0)
    assert E.dbl_4m4s((0, 0, 0, 0)) == (0, 0, 0, 0)


def opening(pre, neg=False):
    """stage 2 of the plan (not built: DESIGN.md section 6): a run opened from its first table point with one product,
    (X : Y : Z : T) = ((y + x) - (y - x) : (y + x) + (y - x) : 2 : (2 d x y) / d); negated: swap the loads, negate T"""
    ymx, ypx, t2d = pre
    if neg:
        ymx, ypx, t2d = ypx, ymx, -t2d
    return (ypx - ymx) % q, (ypx + ymx) % q, 2, t2d * E.inv(E.D) % q


@pytest.mark.parametrize("neg", [False, True])
def test_opening_a_run_from_its_first_table_point(neg):
    for P in E.rand_points(21, 8):
        pre = E.precomputed(E.chi(P))
        o = opening(pre, neg)
        assert E.e_affine(o) == E.e_affine(E.madd_7m(E.IDENTITY, pre, neg))


def _header_array64(name, n):
    txt = open(os.path.join(ROOT, "zecale_amd", "csrc", "bw6_params.h")).read()
    m = re.search(r"%s\[%d\] = \{([^}]*)\}" % (name, n), txt)
    assert m, name
    vals = [int(v.strip().rstrip("ul"), 16) for v in m.group(1).split(",") if v.strip()]
    return sum(v << (64 * i) for i, v in enumerate(vals))


@pytest.mark.parametrize("name, key", [("EDW_C1_64", "c1"), ("EDW_C2_64", "c2")])
def test_host_psi_constants_are_the_generated_ones(name, key):
    assert _header_array64(name, 12) == EP[key] * (1 << 768) % q
