"""The merged Edwards launch (msm.hip k_accumulate_edw_multi): up to four G1 MSMs over one-level-per-window tables through ONE launch
sequence that adds on G1's 2-isogenous twisted Edwards curve, a bucket window per job - through the test hook
zkhip_internal_msm_multi, since the launch is otherwise reached by whole proofs only.  Every job's result must equal the C oracle's
multi_exp of that job and the hook's XYZZ launch (model 0) of the same jobs; an Edwards launch reports the sliced route (0), an XYZZ
launch "not an Edwards launch" (-1).  The base sets differ per job but have EQUAL length: a lane that read another job's table would
give a wrong point, not a wild address."""
import numpy as np
import pytest

from oracle import pyref as R
from tests import msm_cases as M
from tests.helpers import aff_limbs, random_fr_canonical, random_fr_uniform

pytestmark = pytest.mark.gpu

N_SET = 5000
WINDOWS = (4, 9, 13)
# every K in 1 .. 4 at every window, every length of {0, 1, 2, 3, 63, 64, 65, 300, 5000} at least once per window
LENGTHS = ((5000,), (63, 64), (1, 0, 65), (2, 3, 300, 5000))
_cache = {}


def _points(zk):
    """four different sets of N_SET random multiples of the G1 generator (made once)"""
    if "pts" not in _cache:
        g1 = aff_limbs(R.G1_GEN)
        _cache["pts"] = [zk.fixed_base_mul(g1, random_fr_canonical(900 + k, N_SET), montgomery=False) for k in range(4)]
    return _cache["pts"]


def _sets(zk, c):
    """their tables at window c, Edwards forms included (the library's default for G1 sets); kept for the module"""
    if ("sets", c) not in _cache:
        _cache["sets", c] = [zk.Bases.upload(p).precompute(c, table_naf=False) for p in _points(zk)]
        assert all(b.table_model == 1 and b.table_window == c for b in _cache["sets", c])
    return _cache["sets", c]


def _expect(O, bases, scal_mont):
    return O.jac_to_affine(O.msm(bases, scal_mont)) if len(scal_mont) else np.zeros(24, dtype=np.uint64)


def _both(zk, sets, scalars, montgomery=True):
    """[K x 24 affine limbs] of the Edwards and of the XYZZ launch, with the routes they report checked"""
    out = []
    for model, want_path in ((1, 0), (0, -1)):
        jac, path = zk.msm_multi(sets, scalars, model, montgomery=montgomery)
        assert path == want_path, (model, path)
        out.append(np.array([zk.jac_to_affine(j) for j in jac]))
    return out


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda l: "n" + "_".join(map(str, l)))
def test_every_job_equals_the_oracle_and_the_xyzz_launch(zk, oracle_lib, lengths, c):
    pts, sets = _points(zk), _sets(zk, c)
    K = len(lengths)
    # uniform scalars, read as Montgomery limbs by the library and by the oracle alike
    scal = [random_fr_uniform(17 * c + 5 * k + n, n) if n else np.zeros((0, 6), dtype=np.uint64) for k, n in enumerate(lengths)]
    exp = np.array([_expect(oracle_lib, pts[k][:n], scal[k]) for k, n in enumerate(lengths)])
    edw, xyzz = _both(zk, sets[:K], scal)
    for k in range(K):
        assert (edw[k] == exp[k]).all(), ("edwards", c, lengths, k)
        assert (xyzz[k] == exp[k]).all(), ("xyzz", c, lengths, k)
    assert all(exp[k].any() for k, n in enumerate(lengths) if n)            # (no expected value is trivially infinity)


def test_a_slice_spans_buckets_of_several_jobs(zk, oracle_lib):
    """3 terms per job at c = 9: 42 digits x 3 = 126 entries per job over 256 buckets, about 500 in the launch.  A slice holds at least
    16 entries and 126 is no multiple of 16: slices run across the boundaries between the jobs' bucket windows."""
    pts, sets = _points(zk), _sets(zk, 9)
    scal = [random_fr_uniform(400 + k, 3) for k in range(4)]
    exp = np.array([_expect(oracle_lib, pts[k][:3], scal[k]) for k in range(4)])
    edw, xyzz = _both(zk, sets, scal)
    assert (edw == exp).all() and (xyzz == exp).all()
    entries = zk.last_accumulate_entries()
    assert 4 * 100 <= entries <= 4 * 126, entries


def test_a_heavy_bucket_next_to_a_job_boundary(zk, oracle_lib):
    """Job 1: 5,000 scalars equal to 1 at c = 9 - every entry in the FIRST bucket of job 1's window, right behind job 0's last bucket;
    the bucket is cut into many F pieces (the long stitching list).  Jobs 0 and 2 are uniform."""
    pts, sets = _points(zk), _sets(zk, 9)
    ones = M.montgomery_limbs([1] * N_SET)
    scal = [random_fr_uniform(500, 300), ones, random_fr_uniform(502, 300)]
    exp = np.array([_expect(oracle_lib, pts[k][:len(scal[k])], scal[k]) for k in range(3)])
    edw, xyzz = _both(zk, sets[:3], scal)
    assert (edw == exp).all() and (xyzz == exp).all()


def test_scalar_and_point_edges(zk, oracle_lib):
    """Scalars 0, 1, r - 1, r - 2 (negated digits, the sign bit of an entry); P and -P in one bucket; one P five times in one bucket
    (the unified addition doubles); bases at infinity inside a set; an empty job between two that are not."""
    O = oracle_lib
    pts = _points(zk)
    neg = lambda p: np.concatenate([p[:12], O.f_op("sub", 0, np.zeros(12, dtype=np.uint64), p[12:])])
    P, Q = pts[1][0], pts[1][1]
    b0 = pts[0][:64].copy()
    s0 = M.montgomery_limbs([0, 1, R.R_MOD - 1, R.R_MOD - 2] * 16)
    b1 = np.stack([P, neg(P)] + [P] * 5 + [Q])
    s1 = M.montgomery_limbs([5, 5] + [3] * 5 + [7])
    b3 = pts[3][:300].copy()
    b3[::3] = 0                                                             # a third of the set is the point at infinity
    s3 = random_fr_uniform(77, 300)
    bases = [b0, b1, pts[2][:8].copy(), b3]
    scal = [s0, s1, np.zeros((0, 6), dtype=np.uint64), s3]
    sets = [zk.Bases.upload(b).precompute(9, table_naf=False) for b in bases]
    try:
        assert all(b.table_model == 1 for b in sets)
        exp = np.array([_expect(O, bases[k][:len(scal[k])], scal[k]) for k in range(4)])
        edw, xyzz = _both(zk, sets, scal)
        assert (edw == exp).all() and (xyzz == exp).all()
        assert (exp[1] == O.jac_to_affine(O.msm(np.stack([P, Q]), M.montgomery_limbs([15, 7])))).all()      # P - P cancels, 5 x 3 P stays
        assert (exp[2] == 0).all() and exp[0].any() and exp[3].any()
        # job 1 alone with every scalar 0: an Edwards launch whose windows all stay empty is the point at infinity
        edw, xyzz = _both(zk, sets[:2], [M.montgomery_limbs([0] * 64), M.montgomery_limbs([0] * 8)])
        assert (edw == 0).all() and (xyzz == 0).all()
    finally:
        for b in sets:
            b.free()


def test_a_g2_set_is_refused_before_anything_is_enqueued(zk, oracle_lib):
    ks, scal = M.make_case("signs", 257, M.scalar_pool((9,)), seed=3, c=9)
    g2 = zk.Bases.upload(M.bases_of(oracle_lib, ks, g2=True)).precompute(9, table_naf=False)
    g1 = _sets(zk, 9)[0]
    s1 = random_fr_uniform(601, 257)
    jobs = ([g1, g2], [s1, M.montgomery_limbs(scal)])
    try:
        assert g2.table_model == 0
        with pytest.raises(zk.ZkhipError) as e:
            zk.msm_multi(*jobs, 1, montgomery=True)
        assert e.value.code == -4                                           # ZKHIP_ERR_STATE
        jac, path = zk.msm_multi(*jobs, 0, montgomery=True)                                  # the next call on the same sets, XYZZ: correct
        assert path == -1
        assert (zk.jac_to_affine(jac[0]) == _expect(oracle_lib, _points(zk)[0][:257], s1)).all()
        assert (zk.jac_to_affine(jac[1]) == M.closed_form(oracle_lib, ks, scal, g2=True)).all()
        jac, path = zk.msm_multi([g1], [s1], 1, montgomery=True)                             # and an Edwards launch still works afterwards
        assert path == 0 and (zk.jac_to_affine(jac[0]) == _expect(oracle_lib, _points(zk)[0][:257], s1)).all()
    finally:
        g2.free()
