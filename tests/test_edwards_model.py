"""The Edwards model of the G1 bucket accumulation (zecale_amd/csrc/ec_edw.cuh), checked in pure Python:
the 2-isogenous twisted Edwards curve of tools/gen_params.py, the maps chi (G1 -> Edwards) and psi (back), and the formulas the
device uses - in the order and with the constants the device uses them."""
import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_params as GP  # noqa: E402

q, r = GP.Q, GP.R
EP = GP.edwards_params()
D = EP["d"]
G = GP.G1


def inv(a):
    return pow(a % q, q - 2, q)


def w_add(P, Q_):
    """G1 (y^2 = x^3 - 1), affine; None = infinity"""
    if P is None:
        return Q_
    if Q_ is None:
        return P
    (x1, y1), (x2, y2) = P, Q_
    if x1 == x2:
        if (y1 + y2) % q == 0:
            return None
        lam = 3 * x1 * x1 * inv(2 * y1) % q
    else:
        lam = (y2 - y1) * inv(x2 - x1) % q
    x3 = (lam * lam - x1 - x2) % q
    return x3, (lam * (x1 - x3) - y1) % q


def w_mul(k, P):
    acc = None
    while k:
        if k & 1:
            acc = w_add(acc, P)
        P = w_add(P, P)
        k >>= 1
    return acc


def w_neg(P):
    return None if P is None else (P[0], (-P[1]) % q)


def e_on_curve(P):
    """-x^2 + y^2 = 1 + d x^2 y^2"""
    x, y = P
    return (-x * x + y * y - 1 - D * x * x * y * y) % q == 0


def e_add_affine(P, Q_):
    (x1, y1), (x2, y2) = P, Q_
    k = D * x1 * x2 * y1 * y2 % q
    return (x1 * y2 + y1 * x2) * inv(1 + k) % q, (y1 * y2 + x1 * x2) * inv(1 - k) % q


def e_affine(E):
    """extended (X : Y : Z : T) -> affine, checking T = XY/Z"""
    X, Y, Z, T = E
    assert Z % q and (X * Y - T * Z) % q == 0
    zi = inv(Z)
    return X * zi % q, Y * zi % q


IDENTITY = (0, 1, 1, 0)


def chi(P):
    """as k_table_edw computes it: X = x - 1, x_e = t s y / (3 - X^2), y_e = (y^2 - s X^2) / (y^2 + s X^2)"""
    x, y = P
    X = (x - 1) % q
    XX = X * X % q
    sXX = EP["s"] * XX % q
    D1, D2, N2 = (3 - XX) % q, (y * y + sXX) % q, (y * y - sXX) % q
    i = inv(D1 * D2)
    return EP["t"] * EP["s"] % q * y % q * D2 % q * i % q, N2 * D1 % q * i % q


def precomputed(Pe, neg=False):
    x, y = Pe
    if neg:
        x = -x
    return (y - x) % q, (y + x) % q, 2 * D * x * y % q


def madd_7m(acc, pre, neg=False):
    """edw_madd_lds_regy: a negated point swaps the loads of y - x / y + x and trades F for G"""
    X1, Y1, Z1, T1 = acc
    ymx, ypx, t2d = pre
    A = (Y1 - X1) * (ypx if neg else ymx) % q
    B = (Y1 + X1) * (ymx if neg else ypx) % q
    C = T1 * t2d % q
    E, H = B - A, B + A
    F, Gv = 2 * Z1 - C, 2 * Z1 + C
    if neg:
        F, Gv = Gv, F
    return E * F % q, Gv * H % q, F * Gv % q, E * H % q


def add_9m(a, b):
    """full addition (add-2008-hwcd-3, k = 2d)"""
    X1, Y1, Z1, T1 = a
    X2, Y2, Z2, T2 = b
    A = (Y1 - X1) * (Y2 - X2) % q
    B = (Y1 + X1) * (Y2 + X2) % q
    C = T1 * T2 % q * (2 * D) % q
    Dz = Z1 * 2 * Z2 % q
    E, F, Gv, H = B - A, Dz - C, Dz + C, B + A
    return E * F % q, Gv * H % q, F * Gv % q, E * H % q


def dbl_4m4s(a):
    """doubling for a = -1 (dbl-2008-hwcd)"""
    X1, Y1, Z1, _ = a
    A, B, C = X1 * X1 % q, Y1 * Y1 % q, 2 * Z1 * Z1 % q
    E = ((X1 + Y1) * (X1 + Y1) - A - B) % q
    Gv = (B - A) % q
    F, H = Gv - C, -A - B
    return E * F % q, Gv * H % q, F * Gv % q, E * H % q


def psi_xyzz(E):
    """edw_to_xyzz_mem: W = Z^2 - Y^2, lambda = X W, ZZ = lambda^2, ZZZ = lambda^3, X' = (X^2 + c1 Z^2) W^2,
    Y' = c2 Y Z^2 ZZ.  Returns the affine G1 point (None for ZZ = 0)."""
    X, Y, Z, _ = E
    XX, Z2, YY = X * X % q, Z * Z % q, Y * Y % q
    W = (Z2 - YY) % q
    lam = X * W % q
    Xp = (XX + EP["c1"] * Z2) * (W * W) % q
    ZZ = lam * lam % q
    ZZZ = ZZ * lam % q
    Yp = Y * Z2 % q * ZZ % q * EP["c2"] % q
    if ZZ == 0:
        return None
    return Xp * inv(ZZ) % q, Yp * inv(ZZZ) % q


def rand_points(seed, n):
    rng = random.Random(seed)
    step = w_mul(rng.getrandbits(64) | 1, G)
    P = w_mul(rng.getrandbits(64) | 1, G)
    out = []
    for _ in range(n):
        out.append(P)
        P = w_add(P, step if rng.random() < 0.5 else w_add(step, G))
    return out


def test_curve_parameters():
    s, t, A = EP["s"], EP["t"], EP["A"]
    assert s * s % q == q - 3
    assert A == -6 * inv(s) % q
    a_e, d_e = (A + 2) * inv(s) % q, (A - 2) * inv(s) % q
    assert t * t % q == -a_e % q                     # -a_E is a square: the model scales to a = -1
    assert D == -d_e * inv(a_e) % q
    assert pow(D, (q - 1) // 2, q) == 1              # d is a square: the formulas are safe on odd order only
    assert EP["half_r"] * 2 % r == 1
    assert (G[1] ** 2 - G[0] ** 3 + 1) % q == 0


def test_chi_lands_on_the_curve_and_is_a_homomorphism():
    pts = rand_points(1, 12)
    for P in pts:
        assert e_on_curve(chi(P))
    for P, Q_ in zip(pts, pts[1:]):
        assert chi(w_add(P, Q_)) == e_add_affine(chi(P), chi(Q_))
        assert chi(w_neg(P)) == ((-chi(P)[0]) % q, chi(P)[1])


def test_psi_of_chi_is_doubling():
    for P in rand_points(2, 12):
        x, y = chi(P)
        assert psi_xyzz((x, y, 1, x * y % q)) == w_add(P, P)
    assert psi_xyzz(IDENTITY) is None               # the identity maps to XYZZ's infinity (ZZ = 0)


def test_mixed_addition_7m_against_the_affine_law():
    pts = rand_points(3, 200)
    rng = random.Random(4)
    acc, tot = IDENTITY, None
    for P in pts:
        neg = rng.random() < 0.5
        acc = madd_7m(acc, precomputed(chi(P)), neg)
        tot = w_add(tot, w_neg(P) if neg else P)
        assert e_affine(acc) == chi(tot)
    P = pts[7]
    pe = chi(P)
    one = (pe[0], pe[1], 1, pe[0] * pe[1] % q)
    two = madd_7m(one, precomputed(pe))               # P + P through the same formula, Z3 != 0
    assert two[2] % q and e_affine(two) == chi(w_add(P, P))
    zero = madd_7m(one, precomputed(pe), neg=True)    # P + (-P)
    assert zero[2] % q and e_affine(zero) == (0, 1)
    assert e_affine(madd_7m(IDENTITY, precomputed(pe))) == pe
    assert madd_7m(one, precomputed(pe), neg=True) == madd_7m(one, precomputed(pe, neg=True))


def test_full_addition_and_doubling_against_the_affine_law():
    pts = rand_points(5, 40)
    ext = [(x * 3 % q, y * 3 % q, 3, x * y * 3 % q) for x, y in map(chi, pts)]      # Z = 3: projective
    for (a, P), (b, Q_) in zip(zip(ext, pts), zip(ext[1:], pts[1:])):
        assert e_affine(add_9m(a, b)) == chi(w_add(P, Q_))
        assert e_affine(dbl_4m4s(a)) == chi(w_add(P, P))
        assert e_affine(add_9m(a, a)) == chi(w_add(P, P))
        neg = ((-a[0]) % q, a[1], a[2], (-a[3]) % q)
        assert e_affine(add_9m(a, neg)) == (0, 1)
        assert e_affine(add_9m(a, IDENTITY)) == chi(P)
    assert e_affine(dbl_4m4s(IDENTITY)) == (0, 1)


def test_msm_through_the_edwards_model_equals_the_msm():
    """sum k_i P_i = psi(sum k_i chi([1/2] P_i)): the table holds chi of the halved points (k_half_bases), the digits are the
    scalars' own, psi maps the buckets back"""
    rng = random.Random(6)
    pts = rand_points(7, 6)
    ks = [rng.randrange(r) for _ in pts] + [r - 1, 1]
    pts = pts + [pts[0], pts[1]]
    want = None
    for k, P in zip(ks, pts):
        want = w_add(want, w_mul(k, P))
    acc = IDENTITY
    for k, P in zip(ks, pts):
        H = w_mul(EP["half_r"], P)
        assert w_add(H, H) == P                                         # k_half_bases' check: 2 H = P iff r P = O
        run = IDENTITY
        for bit in bin(k)[2:]:
            run = dbl_4m4s(run)
            if bit == "1":
                run = madd_7m(run, precomputed(chi(H)))
        acc = add_9m(acc, run)
    assert psi_xyzz(acc) == want


def test_halving_check_rejects_points_outside_g1():
    """A point of the curve with a component of order 2 (T = (1, 0)) passes the curve equation but not 2 [1/2 mod r] P = P."""
    P = w_add(rand_points(8, 1)[0], (1, 0))
    assert (P[1] ** 2 - P[0] ** 3 + 1) % q == 0
    H = w_mul(EP["half_r"], P)
    assert w_add(H, H) != P


def _header_array(name, n):
    txt = open(os.path.join(ROOT, "zecale_amd", "csrc", "bw6_params.h")).read()
    m = re.search(r"%s\[%d\] = \{([^}]*)\}" % (name, n), txt)
    assert m, name
    vals = [int(v.strip().rstrip("u"), 16) for v in m.group(1).split(",") if v.strip()]
    return sum(v << (29 * i) for i, v in enumerate(vals))


@pytest.mark.parametrize("name, value", [("EDW_D2", 2 * D), ("EDW_S", EP["s"]), ("EDW_TS", EP["t"] * EP["s"]),
                                         ("EDW_C1", EP["c1"]), ("EDW_C2", EP["c2"]), ("EDW_THREE", 3)])
def test_header_constants_are_the_generated_ones(name, value):
    assert _header_array(name, 27) == value * (1 << (29 * 27)) % q


def test_header_half_constant():
    assert _header_array("HALF_RAW", 14) == EP["half_r"] == (r + 1) // 2
    assert EP["half_r"].bit_length() == 376                         # k_half_bases starts from bit 375
