"""Nested (BLS12-377) proof points and inputs a checked nested verifier must refuse, and the status byte pyref alone gives a proof
made of them: the shared fixtures of tests/test_nested_point_check_model.py (CPU) and tests/test_nested_verify_checked_gpu.py.  Built on
the trapdoor statements of tests/nested_verify_fixtures.py, modelled on tests/point_check_fixtures.py.

An element is an Elem: the limbs that go to the library, and the code Python integers give it (0 fine, 2 encoding, 3 off its curve,
4 not of order r).  Points whose encoding is fine get their code from pyref's curve equations and from [r] P by double-and-add:
R.ec_mul does not reduce its scalar and serves G1; R.bls_g2_mul reduces its scalar mod r (bls_g2_mul(r, P) is infinity for EVERY P), so
G2 has its own double-and-add over R.bls_g2_add here.  Limbs that are not fully reduced are made by integer addition on the Montgomery
limbs and are code 2 by construction.  q = 1 (mod 4): square roots by Tonelli-Shanks (15 is a non-residue), Fq2 roots through the norm.
The nested format has no point at infinity: the all-zero point is off its curve."""
import functools
import random
from collections import namedtuple

import numpy as np

from oracle import pyref as R
from tests import nested_verify_fixtures as N

ACCEPT, REJECT, ENCODING, OFF_CURVE, NOT_ORDER_R = range(5)
MASK = dict(a=0x10, b=0x20, c=0x40, inputs=0x80)

Elem = namedtuple("Elem", "name limbs code")

Q, RM = R.BLS_Q, R.BLS_R
assert Q % 4 == 1 and pow(R.FR_GENERATOR, (Q - 1) // 2, Q) == Q - 1


def fq_sqrt(a):
    """Tonelli-Shanks in Fq; None for a non-residue"""
    a %= Q
    if a == 0:
        return 0
    if pow(a, (Q - 1) // 2, Q) != 1:
        return None
    s, t = 0, Q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    c, x, b, m = pow(R.FR_GENERATOR, t, Q), pow(a, (t + 1) // 2, Q), pow(a, t, Q), s
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2, i = b2 * b2 % Q, i + 1
        e = pow(c, 1 << (m - i - 1), Q)
        x, c = x * e % Q, e * e % Q
        b, m = b * c % Q, i
    assert x * x % Q == a
    return x


def fq2_sqrt(a):
    """a root of a = (a0, a1) in Fq[u]/(u^2 + 5) through the norm a0^2 + 5 a1^2; None when there is none"""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        s = fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fq_sqrt(a0 * R.inv_mod(-5 % Q, Q))               # (s u)^2 = -5 s^2
        return None if s is None else (0, s)
    n = fq_sqrt(a0 * a0 + 5 * a1 * a1)
    if n is None:
        return None
    half = R.inv_mod(2, Q)
    for cand in ((a0 + n) * half % Q, (a0 - n) * half % Q):  # x0^2 = (a0 +- n) / 2, x1 = a1 / (2 x0)
        x0 = fq_sqrt(cand)
        if x0:
            x = (x0, a1 * R.inv_mod(2 * x0, Q) % Q)
            if R.fq2_mul(x, x) == (a0, a1):
                return x
    return None


G2_B = R.fq2_inv((0, 1))                                       # 1 / u


def g2_mul_raw(k, P):
    """[k] P on the twist by double-and-add over R.bls_g2_add, the scalar NOT reduced"""
    acc = None
    while k:
        if k & 1:
            acc = R.bls_g2_add(acc, P)
        P = R.bls_g2_add(P, P)
        k >>= 1
    return acc


def pyref_code(P, g2):
    """the checks in their order, for a point whose encoding is fine"""
    if g2:
        if not R.bls_g2_on_curve(P):
            return OFF_CURVE
        return ACCEPT if g2_mul_raw(RM, P) is None else NOT_ORDER_R
    if not R.on_curve(P, R.BLS_G1_B, Q):
        return OFF_CURVE
    return ACCEPT if R.ec_mul(RM, P, Q) is None else NOT_ORDER_R


def _limbs(P, g2):
    return np.array(N.g2_limbs(P) if g2 else N.g1_limbs(P), dtype=np.uint64)


def point_elem(name, P, g2):
    return Elem(name, _limbs(P, g2), pyref_code(P, g2))


def _plus_modulus(limbs):
    """six limbs as one integer, plus q: the same residue, not fully reduced"""
    v = R.limbs_to_int(limbs) + Q
    assert v < 1 << 384
    return np.array(R.int_to_limbs(v, 6), dtype=np.uint64)


Q_LIMBS = np.array(R.int_to_limbs(Q, 6), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def g1_cofactor_points():
    """(the curve point with x = 3, [r] of it): the smallest x >= 3 with a root is 3 itself"""
    y = fq_sqrt(3 ** 3 + 1)
    assert y is not None
    generic = (3, y)
    cof = R.ec_mul(RM, generic, Q)
    assert cof is not None
    return generic, cof


@functools.lru_cache(maxsize=None)
def g2_cofactor_points():
    """(the twist point with x = (2, 0), [r] of it)"""
    x = (2, 0)
    y = fq2_sqrt(R.fq2_add(R.fq2_mul(R.fq2_mul(x, x), x), G2_B))
    assert y is not None
    generic = (x, y)
    cof = g2_mul_raw(RM, generic)
    assert cof is not None
    return generic, cof


@functools.lru_cache(maxsize=None)
def bad_points(g2):
    """the refused points of one group in the issue's order: those not of order r, those off the curve, two encodings"""
    if not g2:
        gen = R.BLS_G1_GEN
        generic, cof = g1_cofactor_points()
        out = [point_elem("g1 (-1, 0) of order 2", (Q - 1, 0), False),
               point_elem("g1 (0, 1) of order 3", (0, 1), False),
               point_elem("g1 (2, 3) of order 6", (2, 3), False),
               point_elem("g1 generator + (-1, 0)", R.ec_add(gen, (Q - 1, 0), Q), False),
               point_elem("g1 the curve point with x = 3", generic, False),
               point_elem("g1 cofactor point", cof, False),
               point_elem("g1 y + 1", (gen[0], (gen[1] + 1) % Q), False),
               Elem("g1 all zero", np.zeros(12, dtype=np.uint64), pyref_code((0, 0), False))]
        assert [e.code for e in out] == [NOT_ORDER_R] * 6 + [OFF_CURVE] * 2
        assert R.ec_mul(2, (Q - 1, 0), Q) is None and R.ec_mul(3, (0, 1), Q) is None and R.ec_mul(6, (2, 3), Q) is None
        assert R.ec_mul(3, (2, 3), Q) is not None and R.ec_mul(2, (2, 3), Q) is not None
        good = _limbs(N.g1mul(77), False)
        plus_q = good.copy(); plus_q[:6] = _plus_modulus(good[:6])
        is_q = good.copy(); is_q[6:] = Q_LIMBS
        return tuple(out + [Elem("g1 x + q", plus_q, ENCODING), Elem("g1 a coordinate equal to q", is_q, ENCODING)])
    gen = R.BLS_G2_GEN
    generic, cof = g2_cofactor_points()
    g1 = R.BLS_G1_GEN
    out = [point_elem("g2 the twist point with x = (2, 0)", generic, True),
           point_elem("g2 cofactor point", cof, True),
           point_elem("g2 generator + cofactor point", R.bls_g2_add(gen, cof), True),
           point_elem("g2 y.c1 + 1", (gen[0], (gen[1][0], (gen[1][1] + 1) % Q)), True),
           Elem("g2 all zero", np.zeros(24, dtype=np.uint64), pyref_code(((0, 0), (0, 0)), True)),
           point_elem("g2 the G1 generator embedded", ((g1[0], 0), (g1[1], 0)), True)]
    assert [e.code for e in out] == [NOT_ORDER_R] * 3 + [OFF_CURVE] * 3
    good = _limbs(N.g2mul(77), True)
    plus_q = good.copy(); plus_q[6:12] = _plus_modulus(good[6:12])
    is_q = good.copy(); is_q[12:18] = Q_LIMBS
    return tuple(out + [Elem("g2 x.c1 + q", plus_q, ENCODING), Elem("g2 y.c0 equal to q", is_q, ENCODING)])


def first_bad(g2, code):
    return next(e for e in bad_points(g2) if e.code == code)


@functools.lru_cache(maxsize=None)
def good_points(g2, n=8, seed=31):
    """the generator and n pseudo-random multiples of it"""
    rng = random.Random(seed + g2)
    mul = N.g2mul if g2 else N.g1mul
    pts = [R.BLS_G2_GEN if g2 else R.BLS_G1_GEN] + [mul(rng.randrange(1, RM)) for _ in range(n)]
    out = tuple(point_elem("good %d" % i, P, g2) for i, P in enumerate(pts))
    assert all(e.code == ACCEPT for e in out)
    return out


def fr2_y_zero_case():
    """The Y = 0 doubling of the Fr2 body, reached at body level (the twist's cofactor has no prime factor below 2000, so no twist point
    of small order exists to reach it through the public route): the "point" ((7, 11), (0, 0)) - the formulas never use b.  Returns
    (24 limbs, whether the Python affine law ends at infinity): 2 (x, 0) = O and r is odd, so [r] (x, 0) = (x, 0): not infinity."""
    P = ((7, 11), (0, 0))
    end = g2_mul_raw(RM, P)
    assert end == P
    return _limbs(P, True), end is None


def input_elems(x):
    """inputs in the place of one of value x: refused (x + q on the limbs, the value r, 2^253 - 1) and fine (r - 1, 0)"""
    val = lambda v: np.array(N.fl(v), dtype=np.uint64)
    assert (1 << 253) - 1 < Q and RM < (1 << 253)
    return ([Elem("input x + q on the limbs", _plus_modulus(val(x % RM)), ENCODING), Elem("input equal to r", val(RM), ENCODING),
             Elem("input 2^253 - 1", val((1 << 253) - 1), ENCODING)],
            [Elem("input r - 1", val(RM - 1), ACCEPT), Elem("input 0", val(0), ACCEPT)])


def bad_inputs(x):
    return input_elems(x)[0]


def status_byte(codes):
    """codes: {"a": .., "b": .., "c": .., "inputs": ..} of one proof -> its refusal byte, 0 when nothing is refused: the first of 2, 3, 4
    that any element has, and the mask of the elements that have exactly that code"""
    for code in (ENCODING, OFF_CURVE, NOT_ORDER_R):
        mask = sum(MASK[k] for k, c in codes.items() if c == code)
        if mask:
            return code | mask
    return 0


Case = namedtuple("Case", "label inputs proof want")       # limbs for the library, and the status byte pyref and the construction give

SLOT = dict(a=(0, 12), b=(12, 36), c=(36, 48))


def make_case(n_inputs, j, replace=None, bump=False, label=""):
    """Statement j of the n_inputs key with elements replaced: replace maps "a" / "b" / "c" to an Elem and "inputs" to an Elem that
    takes the place of the last input.  bump: the first input (without inputs: C := A) is changed, so that a proof nothing refuses is
    rejected by the pairing.  want: the refusal byte from the Elems' codes; else 0 for an untouched statement and 1 for a bumped one -
    what the trapdoor construction makes them (tests/test_nested_pairing_model.py pins it on pyref's pairing)."""
    replace = replace or {}
    vk, proofs = N.statements(n_inputs)
    proof, xs = proofs[j % len(proofs)]
    pl, inp = N.proof_limbs(proof), N.input_limbs(xs)
    codes = dict(a=0, b=0, c=0, inputs=0)
    if bump:
        if n_inputs:
            inp[0] = N.fl((xs[0] + 1 + j) % RM)
        else:
            pl[36:48] = pl[0:12]
    for slot, e in replace.items():
        codes[slot] = e.code
        if slot == "inputs":
            inp[n_inputs - 1] = e.limbs
        else:
            lo, hi = SLOT[slot]
            pl[lo:hi] = e.limbs
    refusal = status_byte(codes)
    return Case(label or ", ".join("%s: %s" % (s, e.name) for s, e in replace.items()) or ("bumped" if bump else "valid"),
                inp, pl, refusal if refusal else (REJECT if bump else ACCEPT))


@functools.lru_cache(maxsize=None)
def refused_cases(n_inputs):
    """{group: [Case]}: every fixture once in each slot it fits - A and C for the G1 ones, B for the G2 ones, the last input for the
    refused inputs (keys with inputs only) - and, under "mixed", proofs with two failure classes at once (precedence and mask), with
    several elements of one class, and a refused proof that is also a wrong statement."""
    g1, g2 = bad_points(False), bad_points(True)
    o1, c1, e1 = first_bad(False, NOT_ORDER_R), first_bad(False, OFF_CURVE), first_bad(False, ENCODING)
    o2, c2, e2 = first_bad(True, NOT_ORDER_R), first_bad(True, OFF_CURVE), first_bad(True, ENCODING)
    out = dict(a=[make_case(n_inputs, i, {"a": e}) for i, e in enumerate(g1)],
               b=[make_case(n_inputs, i + 3, {"b": e}) for i, e in enumerate(g2)],
               c=[make_case(n_inputs, i + 5, {"c": e}) for i, e in enumerate(g1)])
    mixed = [make_case(n_inputs, 1, {"a": o1, "b": c2}),                           # order + curve -> curve, B alone
             make_case(n_inputs, 2, {"a": c1, "c": e1}),                           # curve + encoding -> encoding, C alone
             make_case(n_inputs, 3, {"a": g1[2], "c": g1[5]}),                     # two of one class -> both in the mask
             make_case(n_inputs, 4, {"a": g1[9], "b": o2, "c": g1[7]}),            # all three classes -> encoding, A alone
             make_case(n_inputs, 6, {"b": g2[1], "c": g1[1]}, bump=True)]          # refused AND a wrong statement: the checks decide
    if n_inputs:
        xs = N.statements(n_inputs)[1][2][1]
        bi = bad_inputs(xs[n_inputs - 1])
        out["inputs"] = [make_case(n_inputs, 2, {"inputs": e}) for e in bi]
        mixed += [make_case(n_inputs, 2, {"inputs": bi[0], "b": c2}),              # a refused input + curve -> the input alone
                  make_case(n_inputs, 2, {"inputs": bi[1], "a": e1, "b": e2}),     # three encodings -> A, B and the input
                  make_case(n_inputs, 7, {"inputs": bi[2], "c": o1})]              # a refused input + order -> the input alone
    out["mixed"] = mixed
    for cases in out.values():
        assert all(c.want >= ENCODING for c in cases)
    return out


def fine_input_cases(n_inputs):
    """the inputs r - 1 and 0 in the place of the last input: nothing is refused, the statement is wrong, the pairing rejects"""
    return [make_case(n_inputs, 2, {"inputs": e}, bump=True, label=e.name) for e in input_elems(0)[1]]


def bad_keys(n_inputs=1):
    """[(element name, code, vk limbs)]: delta off its curve, an ABC_i not of order r (the generator + (-1, 0): on its curve and with
    a doubling chain that is not degenerate, so the unchecked constructor takes it), alpha not reduced"""
    vk = N.vk_limbs(N.statements(n_inputs)[0])
    g1, g2 = bad_points(False), bad_points(True)
    k1 = vk.copy(); k1[36:60] = first_bad(True, OFF_CURVE).limbs
    k2 = vk.copy(); k2[60 + 12 * n_inputs:72 + 12 * n_inputs] = g1[3].limbs
    k3 = vk.copy(); k3[0:12] = first_bad(False, ENCODING).limbs
    return [("delta", OFF_CURVE, k1), ("ABC[%d]" % n_inputs, NOT_ORDER_R, k2), ("alpha", ENCODING, k3)]
