"""An Edwards launch keeps its points on the Edwards curve from the slots to the host: the stitching, the bucket reduction and the
two combine kernels add and double extended points (ec_edw.cuh, the k_..._edw kernels of msm.hip) and psi is applied once, on the
host (edw_abi_to_jac).  Every case runs the same bases and scalars through a table built under each point model
(zkhip_set_table_model) and compares the affine limbs exactly - with each other and with the closed form (sum s_i k_i) G: the bases
are known multiples k_i G."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import msm_cases as M
from tests.helpers import aff_limbs, fr_limbs, random_fr_canonical, random_fr_uniform

pytestmark = pytest.mark.gpu

BIG = 1 << 18
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _rebase_device_clock(zk):
    """The library reports accumulation intervals as FLOAT milliseconds since an origin on the device's clock; this module keeps
    the device busy for minutes (c = 4 at 2^18 terms is 25 M entries in 8 buckets), so it re-bases the origin when it is done, as
    the API asks of long-running callers (zkhip_reset_time_base): later readers get their microseconds back."""
    yield
    _cache.clear()
    zk.reset_time_base()


def _to_ints(a):
    return [int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192 | int(x[4]) << 256 | int(x[5]) << 320 for x in a.tolist()]


def _known_points(zk, n):
    """(k_i, k_i G) for n random k_i: one set of BIG points per session, prefixes for the smaller cases"""
    if "pts" not in _cache:
        ks = random_fr_canonical(901, BIG)
        _cache["pts"] = (_to_ints(ks), zk.fixed_base_mul(aff_limbs(R.G1_GEN), ks, montgomery=False))
    ks, bases = _cache["pts"]
    return ks[:n], bases[:n].copy()


def _expected(oracle, ks, scal):
    return oracle.jac_to_affine(oracle.scalar_mul(aff_limbs(R.G1_GEN), fr_limbs(sum(s * k for s, k in zip(scal, ks)) % R.R_MOD)))


def _table(zk, bases, c, model):
    zk.set_table_model(model)
    try:
        return zk.Bases.upload(bases).precompute(c)
    finally:
        zk.set_table_model(-1)


def _both_models(zk, bases, limbs, c):
    out = []
    for model in (0, 1):
        b = _table(zk, bases, c, model)
        try:
            assert b.table_model == model
            out.append(zk.jac_to_affine(b.msm(limbs, montgomery=False)))
        finally:
            b.free()
    return out


def _check(zk, oracle, ks, bases, scal, c, what):
    xyzz, edw = _both_models(zk, bases, M.canonical_limbs(scal), c)
    exp = _expected(oracle, ks, scal)
    assert (edw == xyzz).all(), what
    assert (edw == exp).all(), what
    return edw


@pytest.mark.parametrize("n", [200, BIG])
@pytest.mark.parametrize("c", [4, 9, 16, 20])
def test_uniform_scalars(zk, oracle_lib, c, n):
    """n = 200: almost every slot is empty at the wide windows (the empty-operand paths of every level); n = 2^18: every tree level,
    the one-lane kernels on the CU (k_sum_lds_edw, k_fixup_edw) and the quad kernels both in use"""
    ks, bases = _known_points(zk, n)
    scal = _to_ints(random_fr_uniform(100 + c, n))
    _check(zk, oracle_lib, ks, bases, scal, c, (c, n))


@pytest.mark.parametrize("c", [9, 20])
def test_all_scalars_equal(zk, oracle_lib, c):
    """one bucket per window holds everything: the long stitching list (k_fixup_fold_edw's workgroup folds), every other slot empty"""
    n = 1 << 17
    ks, bases = _known_points(zk, n)
    s = _to_ints(random_fr_uniform(7, 1))[0]
    _check(zk, oracle_lib, ks, bases, [s] * n, c, c)


def test_witness_like(zk, oracle_lib):
    """35 % zeros, 35 % ones, 30 % uniform: one hot bucket in the lowest window beside uniformly filled ones"""
    n = BIG
    ks, bases = _known_points(zk, n)
    scal = _to_ints(random_fr_uniform(8, n))
    sel = np.random.default_rng(8).random(n)
    scal = [0 if u < 0.35 else 1 if u < 0.7 else s for u, s in zip(sel, scal)]
    _check(zk, oracle_lib, ks, bases, scal, 20, "witness_like")


@pytest.mark.parametrize("c", [9, 16])
def test_every_base_the_same_point(zk, oracle_lib, c):
    """every bucket is a multiple of G: equal operands (P + P through the unified addition) at every level of every tree"""
    n = 1 << 16
    bases = np.tile(aff_limbs(R.G1_GEN), (n, 1))
    if c == 9:
        scal = [(i % (1 << (c - 1))) + 1 for i in range(n)]                   # every bucket of the lowest window the SAME point
    else:
        scal = _to_ints(random_fr_uniform(9, n))
    _check(zk, oracle_lib, [1] * n, bases, scal, c, c)


@pytest.mark.parametrize("c", [9, 16])
def test_p_and_minus_p(zk, oracle_lib, c):
    """(P, s) and (-P, s): every bucket is the identity (0 : Y : Y : 0) - an ordinary point that enters the trees - and the sum is
    infinity; with a few unpaired terms behind them the identities are added to real points"""
    half = 1 << 15
    ks, bases = _known_points(zk, half)
    neg = bases.copy()
    for i in range(half):
        neg[i, 12:] = oracle_lib.f_op("sub", 0, np.zeros(12, dtype=np.uint64), bases[i, 12:])
    scal = _to_ints(random_fr_uniform(10 + c, half))
    out = _check(zk, oracle_lib, ks + [-k for k in ks], np.concatenate([bases, neg]), scal + scal, c, c)
    assert (out == 0).all()
    extra = 37
    out = _check(zk, oracle_lib, ks + [-k for k in ks] + ks[:extra], np.concatenate([bases, neg, bases[:extra]]),
                 scal + scal + scal[100:100 + extra], c, c)
    assert (out != 0).any()


@pytest.mark.parametrize("edge", ["lowest", "highest"])
@pytest.mark.parametrize("c", [9, 16])
def test_one_bucket_index_per_window(zk, oracle_lib, c, edge):
    """digits 0 or 1 (only the lowest bucket index of a window is filled: weight 1, the last item of every running sum) and digits 0
    or 2^(cw-1) (only the highest: the first item, the full weight)"""
    n = 1 << 14
    ks, bases = _known_points(zk, n)
    lay = M.window_layout(c)
    rng = random.Random(c)
    scal = []
    for _ in range(n):
        ds = [(1 if edge == "lowest" else 1 << (cw - 1)) if rng.random() < 0.5 else 0 for _, cw in lay]
        scal.append(M._from_digits(c, ds[:-1], ds[-1]))
    assert all(0 <= s < R.R_MOD for s in scal)
    _check(zk, oracle_lib, ks, bases, scal, c, (c, edge))


def test_stream_and_plain_entry_alternate_the_models(zk, oracle_lib):
    """An Edwards set (G1) and an XYZZ set (G2: never Edwards) of the same size and window share the contexts of the plain entry
    point, and a stream of depth 3 keeps several Edwards launches in flight: the finish must apply psi to the Edwards launches only"""
    n, c = 4096, 9
    ks, scal = M.make_case("signs", n, M.scalar_pool((9,)), seed=3, c=c)
    limbs = M.canonical_limbs(scal)
    exp1, exp2 = M.closed_form(oracle_lib, ks, scal), M.closed_form(oracle_lib, ks, scal, g2=True)
    b1 = _table(zk, M.bases_of(oracle_lib, ks), c, 1)
    b2 = _table(zk, M.bases_of(oracle_lib, ks, g2=True), c, 1)
    dev = zk.DeviceBuffer(limbs)
    stream = zk.MsmStream(b1, depth=3)
    try:
        assert b1.table_model == 1 and b2.table_model == 0
        for _ in range(3):
            assert (zk.jac_to_affine(b1.msm(limbs, montgomery=False)) == exp1).all()
            assert (zk.jac_to_affine(b2.msm(limbs, montgomery=False)) == exp2).all()
        sub = 1000
        exp_sub = M.closed_form(oracle_lib, ks[sub:], scal[:n - sub])
        for _ in range(2):
            tickets = [stream.submit(dev.ptr, n, montgomery=False), stream.submit(dev.ptr, n - sub, offset=sub, montgomery=False),
                       stream.submit(dev.ptr, n, montgomery=False)]
            for t, e in zip(tickets, (exp1, exp_sub, exp1)):
                assert (zk.jac_to_affine(stream.collect(t)) == e).all()
        assert (zk.jac_to_affine(b2.msm(limbs, montgomery=False)) == exp2).all()
    finally:
        stream.free(); dev.free(); b1.free(); b2.free()
