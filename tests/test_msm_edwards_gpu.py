"""Single MSMs over one-level-per-window tables accumulate on G1's 2-isogenous Edwards curve by default (ec_edw.cuh, DESIGN.md
section 4).  The same bases and scalars through a table built under each model (zkhip_set_table_model) give the same affine limbs
over the kinds of input the MSM tests use; G2 sets, sets with a point outside the order-r subgroup, every-bit-position tables and
forced batched-affine levels stay XYZZ; and a 2^20 Edwards MSM of random G1 points meets its closed form."""
import numpy as np
import pytest

from oracle import pyref as R
from tests import msm_cases as M
from tests.helpers import aff_limbs, random_fr_canonical, random_fr_uniform

pytestmark = pytest.mark.gpu

POOL = M.scalar_pool((4, 9, 16))


def _table(zk, bases, c, model, naf=False):
    zk.set_table_model(model)
    try:
        return zk.Bases.upload(bases).precompute(c, table_naf=naf)
    finally:
        zk.set_table_model(-1)


def _both_models(zk, bases, scal, c, montgomery):
    out = []
    for model in (0, 1):
        b = _table(zk, bases, c, model)
        try:
            assert b.table_model == model
            out.append(zk.jac_to_affine(b.msm(scal, montgomery=montgomery)))
        finally:
            b.free()
    return out


def _random_g1(zk, seed, n):
    return zk.fixed_base_mul(aff_limbs(R.G1_GEN), random_fr_canonical(seed, n), montgomery=False)


KINDS = ("random", "zero", "single", "duplicates", "p_minus_p", "r_minus_1", "infinity", "witness_like")


@pytest.mark.parametrize("c", [4, 9, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_models_agree(zk, oracle_lib, kind, c):
    n = 3000
    bases = _random_g1(zk, 31 + c, n)
    scal = random_fr_uniform(41 + c, n)
    montgomery = True
    if kind == "zero":
        scal[:] = 0
    elif kind == "single":
        bases, scal = bases[:1], scal[:1]
    elif kind == "duplicates":
        bases = np.repeat(bases[: n // 4], 4, axis=0)
    elif kind == "p_minus_p":
        half = n // 2
        for i in range(half):
            bases[half + i, :12] = bases[i, :12]
            bases[half + i, 12:] = oracle_lib.f_op("sub", 0, np.zeros(12, dtype=np.uint64), bases[i, 12:])
        scal[half:2 * half] = scal[:half]
    elif kind == "r_minus_1":
        scal, montgomery = M.canonical_limbs([R.R_MOD - 1] * n), False
    elif kind == "infinity":
        bases[::3] = 0
    elif kind == "witness_like":
        rng = np.random.default_rng(c)
        sel = rng.random(n)
        scal[sel < 0.5] = 0
        scal[(sel >= 0.5) & (sel < 0.85)] = M.canonical_limbs([1])[0]
        montgomery = False
    xyzz, edw = _both_models(zk, bases, scal, c, montgomery)
    assert (xyzz == edw).all(), (kind, c)
    if kind in ("zero", "p_minus_p"):
        assert (edw == 0).all()


@pytest.mark.parametrize("n", (3, 257, 5000))
def test_models_agree_on_the_structures(zk, oracle_lib, n):
    """cancellation, runs of one point (P + P), rows and random signs over {O, +-G, +-2G, +-3G}: both models against the closed form"""
    for j, st in enumerate(M.STRUCTURES):
        ks, scal = M.make_case(st, n, POOL, seed=j * 13 + n, c=9)
        bases = M.bases_of(oracle_lib, ks)
        exp = M.closed_form(oracle_lib, ks, scal)
        for montgomery, limbs in ((False, M.canonical_limbs(scal)), (True, M.montgomery_limbs(scal))):
            xyzz, edw = _both_models(zk, bases, limbs, 9, montgomery)
            assert (xyzz == exp).all() and (edw == exp).all(), (st, n, montgomery)


def test_selection_keeps_xyzz_where_it_must(zk, oracle_lib):
    ks, scal = M.make_case("signs", 1025, POOL, seed=5, c=9)
    exp_g2 = M.closed_form(oracle_lib, ks, scal, g2=True)
    b = _table(zk, M.bases_of(oracle_lib, ks, g2=True), 9, 1)
    try:
        assert b.table_model == 0                                   # a G2 set: not on G1's curve
        assert (zk.jac_to_affine(b.msm(M.canonical_limbs(scal), montgomery=False)) == exp_g2).all()
    finally:
        b.free()
    bases = M.bases_of(oracle_lib, ks)
    b = _table(zk, bases, 9, 1, naf=True)
    try:
        assert b.table_model == 0                                   # every bit position: NAF digits stay XYZZ
    finally:
        b.free()
    # on G1's curve but not of order r: G + (1, 0) (a component of order 2) - the halving check keeps such a set on XYZZ
    odd = np.stack([M.small_multiples(oracle_lib)[1], aff_limbs((1, 0))] * 3)
    odd_scal = M.montgomery_limbs([3, 5, 7, 8, 11, 2])
    b = _table(zk, odd, 9, 1)
    try:
        assert b.table_model == 0
        assert (zk.jac_to_affine(b.msm(odd_scal)) == oracle_lib.jac_to_affine(oracle_lib.msm(odd, odd_scal))).all()
    finally:
        b.free()
    zk.set_affine_levels(1)
    try:
        b = _table(zk, bases, 9, 1)
        try:
            assert b.table_model == 0                               # forced batched-affine levels: k_affine_level, XYZZ
            assert (zk.jac_to_affine(b.msm(M.canonical_limbs(scal), montgomery=False)) == M.closed_form(oracle_lib, ks, scal)).all()
        finally:
            b.free()
    finally:
        zk.set_affine_levels(-1)


def test_2_20_random_points_closed_form(zk, oracle_lib):
    """The headline shape on the Edwards model: 2^20 random multiples k_i G with their default table, uniform scalars through the
    stream (and a sub-range), against (sum s_i k_i) G."""
    n = 1 << 20
    ks = random_fr_canonical(77, n)
    bases = zk.fixed_base_mul(aff_limbs(R.G1_GEN), ks, montgomery=False)
    scal = random_fr_uniform(78, n)
    to_int = lambda a: [int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192 | int(x[4]) << 256 | int(x[5]) << 320
                        for x in a.tolist()]
    ki, si = to_int(ks), to_int(scal)
    g = aff_limbs(R.G1_GEN)
    exp = lambda lo, ln: oracle_lib.jac_to_affine(oracle_lib.scalar_mul(
        g, M.montgomery_limbs([sum(s * k for s, k in zip(si[:ln], ki[lo:lo + ln])) % R.R_MOD])[0]))
    b = zk.Bases.upload(bases).precompute()
    dev = zk.DeviceBuffer(scal)
    stream = zk.MsmStream(b, depth=2)
    try:
        assert b.table_model == 1
        tickets = [stream.submit(dev.ptr, n, montgomery=False), stream.submit(dev.ptr, n - 4321, offset=4321, montgomery=False)]
        assert (zk.jac_to_affine(stream.collect(tickets[0])) == exp(0, n)).all()
        assert (zk.jac_to_affine(stream.collect(tickets[1])) == exp(4321, n - 4321)).all()
    finally:
        stream.free(); dev.free(); b.free()
