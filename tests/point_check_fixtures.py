"""Proof points and inputs a checked verifier must refuse, and the status byte pyref alone gives a proof made of them: the shared
fixtures of tests/test_point_check_model.py (CPU) and tests/test_verify_checked_gpu.py.  Built on the trapdoor statements of
tests/verify_fixtures.py.  q = 3 (mod 4), so a square root is a^((q + 1) / 4).

An element is an Elem: the limbs that go to the library, and the code pyref gives it (0 fine, 2 encoding, 3 off its curve,
4 not of order r).  Points whose encoding is fine get their code from pyref's on_curve and ec_mul(r, P); limbs that are not fully
reduced are made by integer addition on the Montgomery limbs and are code 2 by construction (the value is >= the modulus)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import pyref as R
from tests import verify_fixtures as V
from tests.helpers import aff_limbs, fq_limbs, fr_limbs

ACCEPT, REJECT, ENCODING, OFF_CURVE, NOT_ORDER_R = range(5)
MASK = dict(a=0x10, b=0x20, c=0x40, inputs=0x80)

Elem = namedtuple("Elem", "name limbs code")

Q, RM = R.Q_MOD, R.R_MOD
assert Q % 4 == 3


def _sqrt(a):
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


def _first_point(b, x0):
    x = x0
    while _sqrt(x ** 3 + b) is None:
        x += 1
    return (x, _sqrt(x ** 3 + b))


def pyref_code(P, g2):
    """the checks in their order, for a point whose encoding is fine (None is the point at infinity)"""
    if P is None:
        return ACCEPT
    if not R.on_curve(P, R.G2_B if g2 else R.G1_B):
        return OFF_CURVE
    return ACCEPT if R.ec_mul(RM, P) is None else NOT_ORDER_R


def point_elem(name, P, g2):
    return Elem(name, aff_limbs(P), pyref_code(P, g2))


def _plus_modulus(limbs, mod):
    """the limbs as one integer, plus the modulus: the same residue, not fully reduced"""
    v = R.limbs_to_int(limbs) + mod
    assert v < 1 << (64 * len(limbs))
    return np.array(R.int_to_limbs(v, len(limbs)), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def bad_points(g2):
    """the refused points of one group, in the issue's order: four not of order r, two off the curve, two encodings"""
    gen, other_gen = (R.G2_GEN, R.G1_GEN) if g2 else (R.G1_GEN, R.G2_GEN)
    small = (0, 2) if g2 else (1, 0)                        # order 3 on y^2 = x^3 + 4, order 2 on y^2 = x^3 - 1
    generic = _first_point(R.G2_B if g2 else R.G1_B, 1 if g2 else 2)
    assert generic[0] == (1 if g2 else 2)
    cof = R.ec_mul(RM, generic)                             # in the cofactor subgroup, no component of order r
    assert cof is not None
    tag = "g2" if g2 else "g1"
    out = [point_elem(tag + " small order", small, g2),
           point_elem(tag + " generator + small order", R.ec_add(gen, small), g2),
           point_elem(tag + " generic curve point", generic, g2),
           point_elem(tag + " cofactor point", cof, g2),
           point_elem(tag + " y + 1", (gen[0], (gen[1] + 1) % Q), g2),
           point_elem(tag + " the other group's generator", other_gen, g2)]
    assert [e.code for e in out] == [NOT_ORDER_R] * 4 + [OFF_CURVE] * 2
    good = aff_limbs(V.g2mul(77) if g2 else V.g1mul(77))
    plus_q = good.copy(); plus_q[:12] = _plus_modulus(good[:12], Q)
    is_q = good.copy(); is_q[12:] = np.array(R.int_to_limbs(Q, 12), dtype=np.uint64)
    out += [Elem(tag + " x + q", plus_q, ENCODING), Elem(tag + " a coordinate equal to q", is_q, ENCODING)]
    return tuple(out)


def good_points(g2, n=8, seed=31):
    """both kinds of points a check must pass: the generator, infinity, n pseudo-random multiples of the generator"""
    import random
    rng = random.Random(seed + g2)
    mul = V.g2mul if g2 else V.g1mul
    pts = [R.G2_GEN if g2 else R.G1_GEN, None] + [mul(rng.randrange(1, RM)) for _ in range(n)]
    return [point_elem("good %d" % i, P, g2) for i, P in enumerate(pts)]


def bad_inputs(x):
    """an input of value x, not fully reduced: x + r on the Montgomery limbs, and r itself"""
    return [Elem("input x + r", _plus_modulus(fr_limbs(x % RM), RM), ENCODING),
            Elem("input equal to r", np.array(R.int_to_limbs(RM, 6), dtype=np.uint64), ENCODING)]


def status_byte(codes):
    """codes: {"a": .., "b": .., "c": .., "inputs": ..} of one proof -> its refusal byte, 0 when nothing is refused: the first of 2, 3, 4
    that any element has, and the mask of the elements that have exactly that code"""
    for code in (ENCODING, OFF_CURVE, NOT_ORDER_R):
        mask = sum(MASK[k] for k, c in codes.items() if c == code)
        if mask:
            return code | mask
    return 0


Case = namedtuple("Case", "label inputs proof want")       # limbs for the library, and the status byte pyref and the construction give


def make_case(n_inputs, j, replace=None, bump=False, label=""):
    """Statement j of the n_inputs key with elements replaced: replace maps "a" / "b" / "c" to an Elem and "inputs" to an Elem that
    takes the place of the last input.  bump: the first input (without inputs: C := A) is changed, so that a proof nothing refuses is
    rejected by the pairing.  want: the refusal byte from the Elems' pyref codes; else 0 for an untouched statement and 1 for a bumped
    one - what the trapdoor construction makes them, and tests/test_pairing_model.py pins on pyref's pairing."""
    replace = replace or {}
    vk, proofs = V.statements(n_inputs)
    proof, xs = proofs[j % len(proofs)]
    pl, inp = V.proof_limbs(proof), V.input_limbs(xs)
    codes = dict(a=0, b=0, c=0, inputs=0)
    if bump:
        if n_inputs:
            inp[0] = fr_limbs((xs[0] + 1 + j) % RM)
        else:
            pl[48:] = pl[:24]
    for slot, e in replace.items():
        codes[slot] = e.code
        if slot == "inputs":
            inp[n_inputs - 1] = e.limbs
        else:
            lo = dict(a=0, b=24, c=48)[slot]
            pl[lo:lo + 24] = e.limbs
    refusal = status_byte(codes)
    return Case(label or ", ".join("%s: %s" % (s, e.name) for s, e in replace.items()) or ("bumped" if bump else "valid"),
                inp, pl, refusal if refusal else (REJECT if bump else ACCEPT))


@functools.lru_cache(maxsize=None)
def refused_cases(n_inputs):
    """{group: [Case]}: every fixture once in each slot it fits - A and C for the G1 ones, B for the G2 ones, the last input for the
    encodings of an input (keys with inputs only) - and, under "mixed", proofs with two failure classes at once (precedence and mask)
    and with several elements of one class."""
    g1, g2 = bad_points(False), bad_points(True)
    out = dict(a=[make_case(n_inputs, i, {"a": e}) for i, e in enumerate(g1)],
               b=[make_case(n_inputs, i + 3, {"b": e}) for i, e in enumerate(g2)],
               c=[make_case(n_inputs, i + 5, {"c": e}) for i, e in enumerate(g1)])
    mixed = [make_case(n_inputs, 1, {"a": g1[0], "b": g2[4]}),                   # order + curve -> curve, B alone
             make_case(n_inputs, 2, {"a": g1[5], "c": g1[6]}),                   # curve + encoding -> encoding, C alone
             make_case(n_inputs, 3, {"a": g1[2], "c": g1[3]}),                   # two of one class -> both in the mask
             make_case(n_inputs, 4, {"a": g1[7], "b": g2[1], "c": g1[4]}),       # all three classes -> encoding, A alone
             make_case(n_inputs, 6, {"b": g2[3], "c": g1[1]}, bump=True)]        # refused AND a wrong statement: the checks decide
    if n_inputs:
        xs = V.statements(n_inputs)[1][2][1]
        bi = bad_inputs(xs[n_inputs - 1])
        out["inputs"] = [make_case(n_inputs, 2, {"inputs": e}) for e in bi]
        mixed += [make_case(n_inputs, 2, {"inputs": bi[0], "b": g2[5]}),          # encoding of an input + curve -> the input alone
                  make_case(n_inputs, 2, {"inputs": bi[1], "a": g1[6], "b": g2[7]}),   # three encodings -> A, B and the input
                  make_case(n_inputs, 7, {"inputs": bi[0], "c": g1[0]})]                  # encoding of an input + order -> the input alone
    out["mixed"] = mixed
    for cases in out.values():
        assert all(c.want >= ENCODING for c in cases)
    return out


def bad_keys(n_inputs=1):
    """[(element name, vk limbs)]: delta off its curve, an ABC_i of order 2, alpha not reduced"""
    vk = V.vk_limbs(V.statements(n_inputs)[0])
    g1, g2 = bad_points(False), bad_points(True)
    k1 = dict(vk, delta=g2[4].limbs)
    abc = vk["ABC"].copy(); abc[n_inputs] = g1[0].limbs
    k2 = dict(vk, ABC=abc)
    k3 = dict(vk, alpha=g1[6].limbs)
    return [("delta", OFF_CURVE, k1), ("ABC[%d]" % n_inputs, NOT_ORDER_R, k2), ("alpha", ENCODING, k3)]
