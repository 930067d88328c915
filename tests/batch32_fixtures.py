"""Batches of up to 32 nested proofs for the tests and for tools/batch32_witness_ab.py: the reference's fixtures (one input per proof)
or the trapdoor-built statements of tests/golden/nested_k{k}.json, cycled."""
import numpy as np

from tests.helpers import fr_limbs
from tests.test_aggregator_host import nested_proof_limbs, nested_vk_limbs
from tests.test_oracle_pins import load_nested_fixtures, load_nested_statement


def big_batch(n, k, bumped=()):
    """n nested proofs with k inputs each under one key - the reference's fixtures (k = 1) or the trapdoor-built statements of
    tests/golden/nested_k{k}.json, cycled - with input 0 of the proofs in `bumped` raised by one.  -> (vk, proofs, inputs as limbs,
    inputs as integers)"""
    nvk, proofs = load_nested_fixtures() if k == 1 else load_nested_statement(k)
    chosen = [proofs[i % len(proofs)] for i in range(n)]
    xs = [list(inp[:k]) for _, inp in chosen]
    for p in bumped:
        xs[p][0] += 1
    return (nested_vk_limbs(nvk), np.concatenate([nested_proof_limbs(p) for p, _ in chosen]),
            np.array([fr_limbs(x) for row in xs for x in row]), [x for row in xs for x in row])


def bumped_proofs(n):
    return (0, n // 2 + 1, n - 1)


def bits_without(n, bumped):
    return ((1 << n) - 1) & ~sum(1 << p for p in bumped)
