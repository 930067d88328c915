"""BW6-761 Groth16 statements with known toxic waste, and the pairing's reduced value in Python big integers: the shared fixtures of
tests/test_pairing_model.py (CPU) and tests/test_verify_gpu.py.  The construction is pyref.bls12_377_groth16_statement_from_trapdoor's,
over BW6-761: key alpha = a G1, beta = b G2, delta = d G2, ABC_i = c_i G1; proof A = rho G1, B = sigma G2,
C = ((rho sigma - a b - c_0 - sum x_i c_i) / d) G1, which makes e(A, B) = e(alpha, beta) e(acc, g2) e(C, delta) hold."""
import functools
import random

import numpy as np

from oracle import pyref as R
from tests.helpers import aff_limbs, fq_int, fq_limbs, fr_limbs

EXT = R.ExtField(R.Q_MOD, 6, -4)
FINAL_EXP = (R.Q_MOD ** 6 - 1) // R.R_MOD

g1mul = lambda k: R.ec_mul(k % R.R_MOD, R.G1_GEN)
g2mul = lambda k: R.ec_mul(k % R.R_MOD, R.G2_GEN)


def statement(seed, n_inputs, n_proofs, edge_inputs=True):
    """(vk, [(proof, inputs)]) as Python points / ints.  With edge_inputs the first proof's inputs start with 0 and r - 1."""
    rng = random.Random(seed)
    a, b, d = (rng.randrange(1, R.R_MOD) for _ in range(3))
    cs = [rng.randrange(1, R.R_MOD) for _ in range(n_inputs + 1)]
    vk = dict(alpha=g1mul(a), beta=g2mul(b), delta=g2mul(d), ABC=[g1mul(c) for c in cs])
    dinv = R.inv_mod(d, R.R_MOD)
    out = []
    for j in range(n_proofs):
        xs = [rng.randrange(R.R_MOD) for _ in range(n_inputs)]
        if edge_inputs and j == 0:
            xs[:2] = [0, R.R_MOD - 1][:n_inputs]
        rho, sigma = rng.randrange(1, R.R_MOD), rng.randrange(1, R.R_MOD)
        c = (rho * sigma - a * b - cs[0] - sum(x * ci for x, ci in zip(xs, cs[1:]))) * dinv % R.R_MOD
        out.append((dict(a=g1mul(rho), b=g2mul(sigma), c=g1mul(c)), xs))
    return vk, out


@functools.lru_cache(maxsize=None)
def statements(n_inputs, n_proofs=8, seed=2024):
    """Cached: the statements every test of a session shares (Python scalar multiplications cost ~10 ms each)."""
    return statement(seed + n_inputs, n_inputs, n_proofs)


def vk_limbs(vk):
    return dict(alpha=aff_limbs(vk["alpha"]), beta=aff_limbs(vk["beta"]), delta=aff_limbs(vk["delta"]),
                ABC=np.array([aff_limbs(P) for P in vk["ABC"]]).reshape(-1, 24))


def proof_limbs(proof):
    return np.concatenate([aff_limbs(proof["a"]), aff_limbs(proof["b"]), aff_limbs(proof["c"])])


def input_limbs(xs):
    return np.array([fr_limbs(x % R.R_MOD) for x in xs], dtype=np.uint64).reshape(-1, 6)


def fq6_limbs(a):
    """six Python ints -> 6 x 12 ABI limbs"""
    return np.array([fq_limbs(x % R.Q_MOD) for x in a], dtype=np.uint64)


def fq6_ints(limbs):
    return [fq_int(row) for row in np.asarray(limbs).reshape(6, 12)]


@functools.lru_cache(maxsize=None)
def _miller(P, Q):
    m4inv = R.inv_mod(-4 % R.Q_MOD, R.Q_MOD)
    Qx, Qy = [0] * 6, [0] * 6
    Qx[4] = Q[0] * m4inv % R.Q_MOD
    Qy[3] = Q[1] * m4inv % R.Q_MOD
    return tuple(R._tate_miller(P, Qx, Qy, EXT, R.R_MOD, R.Q_MOD))


def gt_value(pairs):
    """prod t(P, Q) over the pairs, reduced: pyref's Miller loop and exponentiation with the VALUE returned (pyref's own
    bw6_pairing_product_is_one only says whether it is one).  Infinity (None) on either side contributes 1."""
    f = EXT.one()
    for P, Q in pairs:
        if P is None or Q is None:
            continue
        f = EXT.mul(f, list(_miller(P, Q)))
    return EXT.pow(f, FINAL_EXP)


def fq6_cases(seed=7):
    """(a, b) operand pairs of the Fq6 bodies: random, zero, one, every coefficient at q - 1, a sparse line."""
    rng = random.Random(seed)
    q = R.Q_MOD
    rnd = lambda: [rng.randrange(q) for _ in range(6)]
    top = [q - 1] * 6
    line = [rng.randrange(q), 0, 0, rng.randrange(q), rng.randrange(q), 0]
    return [(rnd(), rnd()), (rnd(), rnd()), ([0] * 6, rnd()), (rnd(), [0] * 6), (EXT.one(), rnd()), (rnd(), EXT.one()),
            (top, top), (top, rnd()), (rnd(), line), (top, [q - 1, 0, 0, q - 1, q - 1, 0]), (line, line)]


def fq6_expected(op, a, b):
    if op == "mul":
        return EXT.mul(a, b)
    if op == "sqr":
        return EXT.mul(a, a)
    return EXT.mul(a, [b[0], 0, 0, b[3], b[4], 0])
