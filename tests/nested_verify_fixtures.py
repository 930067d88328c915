"""Nested (BLS12-377) Groth16 statements and Fq12 operands in Python big integers: the shared fixtures of
tests/test_nested_pairing_model.py (CPU) and tests/test_nested_verify_gpu.py.  Statements come from pyref's trapdoor construction
(bls12_377_groth16_statement_from_trapdoor), from the reference's own fixtures (tests/golden/dummy_app) and from
tests/golden/nested_k{3,9}.json; the degenerate statement is built here with chosen exponents."""
import functools
import random

import numpy as np

from oracle import pyref as R
from tests.helpers import golden, h2i, pt_from_json

Q = R.BLS_Q
EXT = R.ExtField(Q, 12, -5)
LINE_IDX = (0, 1, 3, 7, 9)
# w^q = FROB_C1 w in Fq12 = Fq[w]/(w^12 + 5): the Frobenius scalings of the device are its powers (tower.hpp Fq12Consts)
FROB_C1 = pow(-5 % Q, (Q - 1) // 12, Q)


def fl(x):
    return R.int_to_limbs(R.to_mont(x % Q, Q, 6), 6)


def fint(a):
    return R.from_mont(R.limbs_to_int(a), Q, 6)


def g1_limbs(p):
    return fl(p[0]) + fl(p[1])


def g2_limbs(p):
    return fl(p[0][0]) + fl(p[0][1]) + fl(p[1][0]) + fl(p[1][1])


def vk_limbs(nvk):
    return np.array(g1_limbs(nvk["alpha"]) + g2_limbs(nvk["beta"]) + g2_limbs(nvk["delta"]) + sum((g1_limbs(p) for p in nvk["ABC"]), []),
                    dtype=np.uint64)


def proof_limbs(pr):
    return np.array(g1_limbs(pr["a"]) + g2_limbs(pr["b"]) + g1_limbs(pr["c"]), dtype=np.uint64)


def input_limbs(xs):
    return np.array([fl(x) for x in xs], dtype=np.uint64).reshape(-1, 6)


def frob_limbs():
    return np.array([fl(pow(FROB_C1, i, Q)) for i in range(12)], dtype=np.uint64)


def fq12_limbs(a):
    return np.array([fl(x) for x in a], dtype=np.uint64)


def fq12_ints(limbs):
    return [fint(row) for row in np.asarray(limbs).reshape(12, 6)]


def fq12_cases(seed=11):
    """(a, b) operand pairs of the Fq12 bodies - verify_fixtures.fq6_cases at degree 12: random, zero, one, every coefficient at
    q - 1 (the lazy bounds' worst case), a sparse line, line x line."""
    rng = random.Random(seed)
    rnd = lambda: [rng.randrange(Q) for _ in range(12)]
    top = [Q - 1] * 12
    sparse = lambda f: [f() if i in LINE_IDX else 0 for i in range(12)]
    line = sparse(lambda: rng.randrange(Q))
    return [(rnd(), rnd()), (rnd(), rnd()), ([0] * 12, rnd()), (rnd(), [0] * 12), (EXT.one(), rnd()), (rnd(), EXT.one()),
            (top, top), (top, rnd()), (rnd(), line), (top, sparse(lambda: Q - 1)), (line, line)]


def fq12_expected(op, a, b):
    if op == "mul":
        return EXT.mul(a, b)
    if op == "sqr":
        return EXT.mul(a, a)
    return EXT.mul(a, [b[i] if i in LINE_IDX else 0 for i in range(12)])


g1mul = lambda k: R.ec_mul(k % R.BLS_R, R.BLS_G1_GEN, Q)
g2mul = lambda k: R.bls_g2_mul(k % R.BLS_R, R.BLS_G2_GEN)
g1neg = lambda P: R.ec_neg(P, Q)


@functools.lru_cache(maxsize=None)
def statements(n_inputs, n_proofs=10, seed=377):
    """(vk, [(proof, inputs)]) from pyref's trapdoor construction.  Cached: every test of a session shares them."""
    return R.bls12_377_groth16_statement_from_trapdoor(random.Random(seed + n_inputs), n_inputs, n_proofs)


def _g2_json(p):
    return ((h2i(p[0][1]), h2i(p[0][0])), (h2i(p[1][1]), h2i(p[1][0])))      # JSON order is [c1, c0]


@functools.lru_cache(maxsize=None)
def dummy_app():
    """The reference's nested fixtures: vk.json and extproof1..6.json (one input each, 7 .. 12)."""
    vk = golden("dummy_app/vk.json")
    nvk = dict(alpha=pt_from_json(vk["alpha"]), beta=_g2_json(vk["beta"]), delta=_g2_json(vk["delta"]), ABC=[pt_from_json(p) for p in vk["ABC"]])
    proofs = []
    for i in range(1, 7):
        j = golden(f"dummy_app/extproof{i}.json")["extended_proof"]
        proofs.append((dict(a=pt_from_json(j["proof"]["a"]), b=_g2_json(j["proof"]["b"]), c=pt_from_json(j["proof"]["c"])),
                       [h2i(x) for x in j["inputs"]]))
    return nvk, proofs


@functools.lru_cache(maxsize=None)
def golden_statement(k):
    """tests/golden/nested_k{k}.json: a key with k inputs and three valid proofs."""
    j = golden(f"nested_k{k}.json")
    vk = j["vk"]
    nvk = dict(alpha=pt_from_json(vk["alpha"]), beta=_g2_json(vk["beta"]), delta=_g2_json(vk["delta"]), ABC=[pt_from_json(p) for p in vk["ABC"]])
    proofs = [(dict(a=pt_from_json(e["proof"]["a"]), b=_g2_json(e["proof"]["b"]), c=pt_from_json(e["proof"]["c"])), [h2i(x) for x in e["inputs"]])
              for e in j["proofs"]]
    return nvk, proofs


@functools.lru_cache(maxsize=None)
def degenerate_statement(x=4, negated=False, seed=0xDE6E):
    """A VALID one-input statement (by the group law) under a key on which the host's affine accumulator can meet a degenerate step:
    ABC_0 = c_0 G with c_0 = 4 c_1, or -4 c_1 when `negated`.  While bits 0 and 1 of the input are clear, at step 2 the accumulator
    still is ABC_0 = +-4 ABC_1: the chain point 2^2 ABC_1 or its negative.
      x = 4:           bit 2 is set, the step adds the chain point to itself (or to its negative): the statement of the plan;
      x = 8:           bit 2 is CLEAR, but the host forms the sum and its denominator's inverse at every bit before it selects.  With
                       `negated` its product check fails (verdict 0 although the group law says valid); without, numerator and
                       denominator are both zero and it happens to go through;
      x = 3, 5, 6:     bit 0 or 1 moves the accumulator away first: ordinary statements of the same key.
    Otherwise the trapdoor construction of pyref; one key per value of `negated`, whatever x.  Returns (vk, proof, inputs)."""
    rng = random.Random(seed)
    a, b, d, c1 = (rng.randrange(1, R.BLS_R) for _ in range(4))
    c0 = (-4 if negated else 4) * c1 % R.BLS_R
    vk = dict(alpha=g1mul(a), beta=g2mul(b), delta=g2mul(d), ABC=[g1mul(c0), g1mul(c1)])
    rho, sigma = rng.randrange(1, R.BLS_R), rng.randrange(1, R.BLS_R)
    c = (rho * sigma - a * b - c0 - x * c1) * R.inv_mod(d, R.BLS_R) % R.BLS_R
    return vk, dict(a=g1mul(rho), b=g2mul(sigma), c=g1mul(c)), [x]


def doubling_chain(P, bits=253):
    """[2^j P for j < bits], affine"""
    out = []
    for _ in range(bits):
        out.append(P)
        P = R.ec_add(P, P, Q)
    return out


def accumulator(vk, xs):
    acc = vk["ABC"][0]
    for x, P in zip(xs, vk["ABC"][1:]):
        acc = R.ec_add(acc, R.ec_mul(x % (1 << 253), P, Q), Q)
    return acc


def verification_pairs(vk, proof, xs):
    """the four pairs whose product is one for a valid statement"""
    return [(proof["a"], proof["b"]), (accumulator(vk, xs), R.bls_g2_neg(R.BLS_G2_GEN)), (vk["alpha"], R.bls_g2_neg(vk["beta"])),
            (proof["c"], R.bls_g2_neg(vk["delta"]))]


def pair_limbs(pairs):
    """[(P, Q)] -> (1 x n x 12, 1 x n x 24) limb arrays"""
    return (np.array([[g1_limbs(P) for P, _ in pairs]], dtype=np.uint64), np.array([[g2_limbs(Qq) for _, Qq in pairs]], dtype=np.uint64))
