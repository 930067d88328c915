"""The tail of the bucket reduction by bit planes (msm.hip k_plane_sum, k_plane_combine, enqueue_tail), alone
through its test hook, and whole MSMs over window tables against the oracle.

The hook takes 2W groups of N affine points, the W hi groups first, item i of a group with weight i + 1, and returns per window
2^lo_bits sum (i+1) hi[i] + sum (i+1) lo[i] and, with total, the plain sum of the lo group (what a NAF plan's finish needs).  Every
item is a known multiple k_i G (zkhip.fixed_base_mul; k_i = 0: the point at infinity), so the expected values are scalar
multiplications of G by the oracle.  An Edwards run maps the items through chi and the results back through psi,
psi(chi(P)) = 2 P: it returns twice the sums.  Results are compared as affine points (the projective representative is free)."""
import numpy as np
import pytest

from oracle import pyref as R
from tests.helpers import aff_limbs, fr_ints, fr_limbs, random_fr_canonical, random_fr_uniform

pytestmark = pytest.mark.gpu

W_MAX, N_MAX = 5, 1024
# (N, lo_bits, H): the sizes of the plan at c = 3 (N = 2: one level of fan-in 2), c = 5 (R = 4, H = 2), c = 13 (R = H = 64: three
# levels of fan-in 4) and c = 20 (R = 1024, H = 512: five levels; the bench's window).  The hi group holds Row[1 .. H-1]: H - 1 items.
SHAPES = [(2, 1, 2), (4, 2, 2), (64, 6, 64), (1024, 10, 512)]


@pytest.fixture(scope="module")
def pool(zk):
    """2 W_MAX N_MAX known multiples of G, made once: (k_i as ints, affine limbs [n][24])"""
    n = 2 * W_MAX * N_MAX
    lim = random_fr_canonical(77, n)
    ks = [sum(int(lim[i, j]) << (64 * j) for j in range(6)) for i in range(n)]
    pts = zk.fixed_base_mul(aff_limbs(R.G1_GEN), lim, montgomery=False)
    return ks, pts


def points_of(zk, ks):
    """affine limbs of k G for a short list of ints (0: all-zero limbs)"""
    lim = np.array([[(k >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(6)] for k in ks], dtype=np.uint64).reshape(-1, 6)
    pts = zk.fixed_base_mul(aff_limbs(R.G1_GEN), lim, montgomery=False)
    pts[[i for i, k in enumerate(ks) if k % R.R_MOD == 0]] = 0
    return pts


def expected(oracle_lib, e):
    return oracle_lib.jac_to_affine(oracle_lib.scalar_mul(aff_limbs(R.G1_GEN), fr_limbs(e % R.R_MOD)))


def check(zk, oracle_lib, ks, pts, W, N, lo_bits, edw, total):
    """ks: [2W][N] ints, pts: [2W][N][24]"""
    got = zk.msm_tail(pts, W, lo_bits, edw=edw, total=total)
    assert got.shape == (W * (2 if total else 1), 36)
    m = 2 if edw else 1
    for w in range(W):
        e = (sum((i + 1) * k for i, k in enumerate(ks[w])) << lo_bits) + sum((i + 1) * k for i, k in enumerate(ks[W + w]))
        assert (zk.jac_to_affine(got[w]) == expected(oracle_lib, m * e)).all(), ("window", w, W, N, lo_bits, edw, total)
        if total:
            assert (zk.jac_to_affine(got[W + w]) == expected(oracle_lib, m * sum(ks[W + w]))).all(), ("total", w, W, N, lo_bits, edw)


@pytest.mark.parametrize("edw", (False, True), ids=("xyzz", "edw"))
@pytest.mark.parametrize("W", (1, 5))
@pytest.mark.parametrize("N,lo_bits,H", SHAPES)
def test_tail_of_random_items(zk, oracle_lib, pool, N, lo_bits, H, W, edw):
    ks_all, pts_all = pool
    ks = [list(ks_all[g * N:(g + 1) * N]) for g in range(2 * W)]
    pts = pts_all[:2 * W * N].reshape(2 * W, N, 24).copy()
    for g in range(W):                        # the hi groups as k_place_hilo leaves them: H - 1 rows, infinity beyond
        ks[g][H - 1:] = [0] * (N - H + 1)
        pts[g, H - 1:] = 0
    for total in (False, True):
        check(zk, oracle_lib, ks, pts, W, N, lo_bits, edw, total)


def edge_cases(N, k, k2):
    """name -> [hi group, lo group] of N scalars"""
    r = R.R_MOD
    z = [0] * N
    one = lambda i: [k if j == i else 0 for j in range(N)]
    pairs = [(k if j % 4 < 2 else k2) if j % 2 == 0 else r - (k if j % 4 < 2 else k2) for j in range(N)]      # P, -P, Q, -Q, ...
    return {
        "all_infinity": [z, z],
        "first_item_only": [z, one(0)],
        "last_item_only": [z, one(N - 1)],
        "first_and_last_of_hi": [[k if j in (0, N - 2) else 0 for j in range(N)], z],
        "all_equal": [[k] * (N - 1) + [0], [k] * N],                 # every addition of the planes' trees is a doubling
        "p_and_minus_p_adjacent": [pairs[:N - 2] + [0, 0], pairs],
        "one_live_pair_cancels": [z, [k, r - k] + [0] * (N - 2)],    # the total and plane sums that hold both are the identity
    }


@pytest.mark.parametrize("edw", (False, True), ids=("xyzz", "edw"))
@pytest.mark.parametrize("N,lo_bits", [(2, 1), (4, 2), (64, 6)])
@pytest.mark.parametrize("name", sorted(edge_cases(4, 1, 2)))
def test_tail_edge_cases(zk, oracle_lib, pool, name, N, lo_bits, edw):
    k, k2 = pool[0][0], pool[0][1]
    ks = edge_cases(N, k, k2)[name]
    vals = sorted({v for g in ks for v in g})
    by_val = dict(zip(vals, points_of(zk, vals)))
    pts = np.array([[by_val[v] for v in g] for g in ks], dtype=np.uint64)
    check(zk, oracle_lib, ks, pts, 1, N, lo_bits, edw, total=True)
    if name == "all_infinity":
        assert all((zk.jac_to_affine(p) == 0).all() for p in zk.msm_tail(pts, 1, lo_bits, edw=edw, total=True))


def test_tail_hook_refuses_bad_shapes(zk):
    pts = np.zeros((2, 3, 24), dtype=np.uint64)
    with pytest.raises(zk.ZkhipError):
        zk.msm_tail(pts, 1, 2)                # N = 3: not a power of two
    with pytest.raises(zk.ZkhipError):
        zk.msm_tail(np.zeros((12, 4, 24), dtype=np.uint64), 6, 2)


# ---------------------------------------------------------------- whole MSMs over window tables
@pytest.fixture(scope="module")
def msm_inputs(zk, oracle_lib):
    """n -> (bases, {scalar family: (canonical limbs, expected affine point)}); the oracle's MSM once per (n, family)"""
    out = {}
    for n in (257, 4096):
        bases = zk.fixed_base_mul(aff_limbs(R.G1_GEN), random_fr_canonical(1000 + n, n), montgomery=False)
        fam = {"uniform": random_fr_uniform(2000 + n, n), "ones": np.tile(np.array([1, 0, 0, 0, 0, 0], dtype=np.uint64), (n, 1))}
        exp = {}
        for name, s in fam.items():
            mont = np.array([fr_limbs(x) for x in [sum(int(s[i, j]) << (64 * j) for j in range(6)) for i in range(n)]]).reshape(n, 6)
            exp[name] = (s, oracle_lib.jac_to_affine(oracle_lib.msm(bases, mont)))
        # run LAST on each base set (sorted order): every bucket is empty, and an empty slot keeps the coordinates of the launch before
        # it - only its ZZ / Z words are cleared.  The result is the point at infinity, all-zero limbs.
        exp["zeros"] = (np.zeros((n, 6), dtype=np.uint64), np.zeros(24, dtype=np.uint64))
        out[n] = (bases, exp)
    return out


# the table kinds that reach the tail: XYZZ and Edwards points over a one-level-per-window table, XYZZ over a NAF table (total)
KINDS = {"xyzz": (0, False), "edw": (1, False), "naf": (0, True)}


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("c", (4, 9, 12))
@pytest.mark.parametrize("n", (257, 4096))
def test_whole_msm_over_tables_matches_the_oracle(zk, msm_inputs, n, c, kind):
    """scalars uniform below r, every scalar 1 (the whole MSM in bucket 0: one finite item at index 0 of the lo group), and, last on
    the same context, every scalar 0 (no bucket written: the tail reads slots that are empty by their ZZ / Z words alone)"""
    model, naf = KINDS[kind]
    bases, fams = msm_inputs[n]
    zk.set_table_model(model)
    try:
        b = zk.Bases.upload(bases).precompute(c, table_naf=naf)
    finally:
        zk.set_table_model(-1)
    try:
        assert b.table_window == c and b.table_model == model
        for name, (s, exp) in sorted(fams.items()):
            got = zk.jac_to_affine(b.msm(s, montgomery=False))
            assert (got == exp).all(), (n, c, kind, name)
    finally:
        b.free()
