"""The lockstep route of the Edwards accumulation (msm.hip k_bucket_order, k_accumulate_edw_lock): one bucket per
lane over the buckets ordered by population, taken when the device finds no bucket above ZK_LOCK_CAP entries and enough non-empty
buckets, the sliced route (k_accumulate_edw + stitching) otherwise.

Every case is a small table-backed set of known multiples of G (tests/msm_cases.py) with scalars chosen digit by digit, so the
bucket populations are known here (recode_plain mirrors the device recoding; a one-level-per-window table puts every digit of
every window into ONE bucket window of 2^(c-1) buckets, bucket = |digit| - 1).  The affine result is compared exactly with the closed
form (sum s_i k_i) G under both settings of the switch, and the route the device took is read back with the test hook.  The number of
non-empty buckets a launch needs is lowered to 1 for these small sets (zkhip_internal_set_lockstep); one test keeps the chip's figure."""
import os
import random
import re

import pytest

from tests import msm_cases as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = int(re.search(r"#define ZK_LOCK_CAP (\d+)u", open(os.path.join(ROOT, "zecale_amd", "csrc", "msm.hip")).read()).group(1))


def counts_of(ks, scal, c):
    """(entries per bucket, negated entries per bucket) of the launch: what k_bucket_sort's histogram will say"""
    nb = 1 << (c - 1)
    cnt, neg = [0] * nb, [0] * nb
    for k, s in zip(ks, scal):
        if k == 0:
            continue                                  # a base at infinity produces no entry
        for _, d in M.recode_plain(s, c):
            if d:
                cnt[abs(d) - 1] += 1
                neg[abs(d) - 1] += d < 0
    return cnt, neg


def from_counts(c, want, seed, ks_pool=(1, -1, 2, -2, 3, -3)):
    """terms whose only non-zero digit is the lowest window's: scalar b + 1 -> one entry in bucket b; want[b] of them"""
    rng = random.Random(seed)
    terms = [(rng.choice(ks_pool), b + 1) for b, w in enumerate(want) for _ in range(w)]
    rng.shuffle(terms)
    return [k for k, _ in terms], [s for _, s in terms]


def case_equal():          # every bucket the same count; nb = 32: no multiple of 64
    return 6, *from_counts(6, [8] * 32, 1)


def case_mixed_cap():      # count 1 next to count CAP inside wave 0; 65 non-empty buckets: wave 1 has a single live lane; empties
    want = [0] * 128
    for b in (3, 64, 127):
        want[b] = CAP
    for b in range(5, 5 + 62):
        if want[b] == 0:
            want[b] = 1
    want[100] = 1
    assert sum(1 for w in want if w) == 65 and max(want) == CAP
    return 8, *from_counts(8, want, 2)


def case_cap_plus_one():   # the same histogram with one entry more in one bucket
    c, ks, scal = case_mixed_cap()
    return c, ks + [2], scal + [4]


def case_tiny():           # nb = 8, five non-empty buckets, mixed counts
    return 4, *from_counts(4, [45, 0, 105, 15, 0, 30, 0, 75], 3)


def case_negated():        # bucket 5 holds negated entries only (window value 2^c - 6: digit -6 and a carry: digit +1 one window up)
    c = 7
    ks, scal = from_counts(c, [2, 4, 0, 3, 1, 0, 6] + [5] * 50 + [0] * 7, 4)
    ks += [1, -2, 3, 1, 2]
    scal += [(1 << c) - 6] * 5
    cnt, neg = counts_of(ks, scal, c)
    assert cnt[5] == 5 and neg[5] == 5
    return c, ks, scal


def case_identity_bucket():   # bucket 8 holds P and -P and nothing else: the identity, an ordinary point; bucket 2 the same twice over
    c = 6
    ks, scal = from_counts(c, [1, 2, 0, 3] + [0] * 12 + [16] * 16, 5)
    ks += [2, -2, 1, 3, -1, -3]
    scal += [9, 9, 3, 3, 3, 3]
    return c, ks, scal


def case_all_cancel():     # every bucket sums to the identity: the MSM is the point at infinity
    ks, scal = M.make_case("cancel", 600, list(range(1, 33)), seed=6)
    return 6, ks, scal


def case_uniform():        # full-width random scalars, 48 digits each, over 128 finite bases (and as many at infinity): about 48 entries a bucket
    rng = random.Random(7)
    n = 256
    return 8, [rng.choice((1, -1, 2, -2, 3, -3)) if i % 2 else 0 for i in range(n)], [rng.randrange(M.R.R_MOD) for _ in range(n)]


def case_witness_like():   # 35 % zeros, 35 % ones, 30 % uniform: "scalar == 1" alone fills bucket 0 far above the cap
    rng = random.Random(8)
    n = 2048
    scal = []
    for _ in range(n):
        u = rng.random()
        scal.append(0 if u < 0.35 else 1 if u < 0.7 else rng.randrange(M.R.R_MOD))
    return 8, [rng.choice((1, -1, 2, -2, 3, -3)) for _ in range(n)], scal


# name -> (maker, route expected with the switch on)
CASES = {
    "equal": (case_equal, 1), "mixed_cap": (case_mixed_cap, 1), "cap_plus_one": (case_cap_plus_one, 0), "tiny": (case_tiny, 1),
    "negated": (case_negated, 1), "identity_bucket": (case_identity_bucket, 1), "all_cancel": (case_all_cancel, 1),
    "uniform": (case_uniform, 1), "witness_like": (case_witness_like, 0),
}


def _table(zk, bases, c):
    zk.set_table_model(1)
    try:
        b = zk.Bases.upload(bases).precompute(c)
    finally:
        zk.set_table_model(-1)
    assert b.table_model == 1
    return b


def _run(zk, b, scal, mode, min_buckets=1):
    zk.set_lockstep(mode, min_buckets)
    try:
        out = zk.jac_to_affine(b.msm(M.canonical_limbs(scal), montgomery=False))
        return out, zk.last_acc_path()
    finally:
        zk.set_lockstep(-1, -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_routes_agree_with_the_closed_form(zk, oracle_lib, name):
    maker, want_path = CASES[name]
    c, ks, scal = maker()
    assert 256 <= len(ks) <= 4096
    cnt, _ = counts_of(ks, scal, c)
    assert (max(cnt) <= CAP) == bool(want_path), "the case no longer has the histogram it was built for"
    if name == "mixed_cap":
        assert max(cnt) == CAP
    if name == "cap_plus_one":
        assert max(cnt) == CAP + 1
    exp = M.closed_form(oracle_lib, ks, scal)
    b = _table(zk, M.bases_of(oracle_lib, ks), c)
    try:
        on, path_on = _run(zk, b, scal, 1)
        off, path_off = _run(zk, b, scal, 0)
    finally:
        b.free()
    print(name, "c", c, "n", len(ks), "max count", max(cnt), "non-empty", sum(1 for x in cnt if x), "route", path_on, path_off)
    assert path_on == want_path and path_off == 0
    assert (on == exp).all() and (off == exp).all()
    if name == "all_cancel":
        assert (on == 0).all()


def test_one_context_alternates_routes(zk, oracle_lib):
    """Five launches on one base set and one context, eligible and ineligible in turn: the flag word, the bucket slots and the
    stitching lists of a launch carry nothing into the next."""
    c = 8
    seq = ["mixed_cap", "cap_plus_one", "uniform", "witness_like", "mixed_cap"]
    made = {}
    for name in set(seq):
        cc, ks, scal = CASES[name][0]()
        assert cc == c
        made[name] = (ks, scal)
    # one base set that serves every vector: each case's multiples in a range of its own, the other ranges get scalar 0
    order = sorted(made)
    start, all_ks = {}, []
    for name in order:
        start[name] = len(all_ks)
        all_ks += made[name][0]
    b = _table(zk, M.bases_of(oracle_lib, all_ks), c)
    try:
        for name in seq:
            ks, scal = made[name]
            full = [0] * len(all_ks)
            full[start[name]:start[name] + len(scal)] = scal
            got, path = _run(zk, b, full, 1)
            assert path == CASES[name][1], name
            assert (got == M.closed_form(oracle_lib, ks, scal)).all(), name
    finally:
        b.free()


def test_small_launch_stays_sliced_under_the_chips_own_threshold(zk, oracle_lib):
    """With the chip's figure for the non-empty buckets (two waves for every SIMD) a launch of 32 buckets is not eligible."""
    c, ks, scal = case_equal()
    b = _table(zk, M.bases_of(oracle_lib, ks), c)
    try:
        got, path = _run(zk, b, scal, 1, min_buckets=-1)
    finally:
        b.free()
    assert path == 0
    assert (got == M.closed_form(oracle_lib, ks, scal)).all()
