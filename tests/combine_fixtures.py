"""Batches for the combined (random-combination) check and their expected GT value in Python big integers: the shared fixtures of
tests/test_pairing_combine_model.py (CPU) and tests/test_verify_combined_gpu.py.  Built on the eight trapdoor statements per key of
tests/verify_fixtures.py, repeated, so Python never computes more than a handful of Miller loops.

A proof is TAMPERED by C := C + k D for a fixed D in G1.  The valid part of its pairing product is one, so its product is
gt = t(k D, -delta) = g^k with g = t(D, -delta): one Python pairing per key gives the value of every tampering, and a batch with
scalars rho_i and tamperings k_i (0 = untouched) has the combined value g^(sum k_i rho_i mod r)."""
import functools

import numpy as np

from oracle import pyref as R
from tests import verify_fixtures as V

D = R.ec_mul(5, R.G1_GEN)
MASK128 = (1 << 128) - 1


def tamper(proof, k):
    """the proof with C + k D in place of C (k may be negative)"""
    return dict(proof, c=R.ec_add(proof["c"], R.ec_mul(k % R.R_MOD, D)))


@functools.lru_cache(maxsize=None)
def g(n_inputs):
    """t(D, -delta) under the n_inputs key: the pairing product of a proof tampered with k = 1"""
    vk = V.statements(n_inputs)[0]
    return tuple(V.gt_value([(D, R.ec_neg(vk["delta"]))]))


def expected_value(n_inputs, ks, rhos):
    """the combined value of a batch with tamperings ks under scalars rhos"""
    return V.EXT.pow(list(g(n_inputs)), sum(k * r for k, r in zip(ks, rhos)) % R.R_MOD)


def scalars(count, seed=1):
    """count explicit, pairwise different, non-zero 128-bit scalars (an odd multiplier is a bijection of Z / 2^128) with high words set"""
    mult = 0x9E3779B97F4A7C15F39CC0605CEDC835
    return [((i + seed) * mult) & MASK128 for i in range(count)]


@functools.lru_cache(maxsize=None)
def _limbs(n_inputs, j, k):
    proof, xs = V.statements(n_inputs)[1][j]
    return V.input_limbs(xs), V.proof_limbs(tamper(proof, k) if k else proof)


def batch(n_inputs, count, tampered=None):
    """count statements cycling through the key's eight; tampered: {position: k}.  Returns (inputs count x n x 6, proofs count x 72, ks)."""
    tampered = tampered or {}
    n = len(V.statements(n_inputs)[1])
    base_in = np.array([_limbs(n_inputs, j, 0)[0] for j in range(n)]).reshape(n, n_inputs, 6)
    base_pr = np.array([_limbs(n_inputs, j, 0)[1] for j in range(n)])
    idx = np.arange(count) % n
    inputs, proofs = base_in[idx], base_pr[idx]
    ks = [0] * count
    for pos, k in tampered.items():
        proofs[pos] = _limbs(n_inputs, pos % n, k)[1]
        ks[pos] = k
    return np.ascontiguousarray(inputs), np.ascontiguousarray(proofs), ks


def four_pairs(vk, proof, xs):
    """the four pairs of the Groth16 equation for one proof, Python points"""
    acc = vk["ABC"][0]
    for x, P in zip(xs, vk["ABC"][1:]):
        acc = R.ec_add(acc, R.ec_mul(x, P))
    return [(proof["a"], proof["b"]), (acc, R.ec_neg(R.G2_GEN)), (vk["alpha"], R.ec_neg(vk["beta"])), (proof["c"], R.ec_neg(vk["delta"]))]
