"""The lockstep kernel's opening and its gathers ahead (msm.hip k_accumulate_edw_lock; ec_edw.cuh edw_open_lds_pre, edw_madd_lds_pre,
edw_pre_issue): a bucket is SET to its first table point (one product) instead of adding it to the identity, and
every addition finds its point in registers, gathered under the addition before it.

Built like tests/test_msm_lockstep_gpu.py: small table-backed sets of known multiples of G (tests/msm_cases.py), scalars chosen digit
by digit, the non-empty buckets a launch needs lowered to 1, the affine result compared exactly with the closed form under both
settings of the switch and the route read back.  Here the histograms are given bucket by bucket WITH the signs of the entries:

  '+' in bucket b   a term with scalar b + 1: one entry, digit b + 1 of window 0
  '-' in bucket b   a term with scalar (2^c - (b + 1)) + (w - 1) 2^c: window 0 holds 2^c - (b + 1) > 2^(c-1), which recodes to the
                    digit -(b + 1) - a NEGATED entry of bucket b - and carries into window 1, digit w: a '+' entry of bucket w - 1
                    (the level-1 table point of the same base).  The '+' slot it fills is taken from the histogram, so the counts
                    stay what the case says.  (b + 1 < 2^(c-1): the top bucket takes no negated entry.)

The order of the entries INSIDE a bucket is the device sort's; where a case is about an order (sign patterns, "negated first") the
terms are supplied in both orders in different buckets."""
import os
import random
import re

import pytest

from tests import msm_cases as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = int(re.search(r"#define ZK_LOCK_CAP (\d+)u", open(os.path.join(ROOT, "zecale_amd", "csrc", "msm.hip")).read()).group(1))
KS = (1, -1, 2, -2, 3, -3)


def histogram(ks, scal, c):
    """(entries per bucket, negated entries per bucket) of the launch, by the mirror of the device recoding"""
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


def terms_of(c, want, seed, fixed=()):
    """want[b] = the signs of bucket b's entries, e.g. "+-+"; `fixed` = [(k, scalar)] terms that come FIRST and whose entries the
    caller has already taken out of `want`.  Returns (ks, scalars) and checks the histogram against the mirror of the recoding."""
    rng = random.Random(seed)
    nb = 1 << (c - 1)
    assert len(want) == nb
    plus = [b for b, w in enumerate(want) for ch in w if ch == "+"]
    minus = [b for b, w in enumerate(want) for ch in w if ch == "-"]
    rng.shuffle(plus)
    assert len(plus) >= len(minus), "every negated entry needs a '+' slot for its carry"
    terms = list(fixed)
    for b in minus:
        assert b + 1 < 1 << (c - 1)
        w = plus.pop() + 1
        terms.append((rng.choice(KS), (1 << c) - (b + 1) + ((w - 1) << c)))
    tail = [(rng.choice(KS), b + 1) for b in plus]
    rng.shuffle(tail)
    terms += tail
    ks, scal = [k for k, _ in terms], [s for _, s in terms]
    return ks, scal


def check_histogram(ks, scal, c, want, extra=None):
    cnt, neg = histogram(ks, scal, c)
    exp_cnt = [len(w) for w in want]
    exp_neg = [w.count("-") for w in want]
    for b, (dc, dn) in (extra or {}).items():
        exp_cnt[b] += dc
        exp_neg[b] += dn
    assert cnt == exp_cnt and neg == exp_neg, "the case no longer has the histogram it was built for"
    return cnt, neg


def case_singles():            # every non-empty bucket holds exactly one entry, a third of them negated: opening, then the close
    c = 7
    want = [""] * 64
    for b in range(0, 60):
        if b % 5 != 4:
            want[b] = "-" if b % 3 == 1 else "+"
    ks, scal = terms_of(c, want, 11)
    cnt, neg = check_histogram(ks, scal, c, want)
    assert max(cnt) == 1 and sum(neg) >= 10
    return c, ks, scal


def case_pairs():              # buckets of exactly two entries, every sign pattern: ONE addition, from a prefetched point
    c = 8
    want = [""] * 128
    for i, b in enumerate(range(3, 3 + 96)):
        want[b] = ("++", "+-", "-+", "--")[i % 4]
    want[0] = want[1] = "++"
    ks, scal = terms_of(c, want, 12)
    cnt, neg = check_histogram(ks, scal, c, want)
    assert set(cnt) == {0, 2} and {n for n, k in zip(neg, cnt) if k} == {0, 1, 2}
    return c, ks, scal


def _one_beside_cap(last_is_one):
    """65 non-empty buckets of 128: three of CAP entries and 62 of one - wave 0 holds the three beside 61 lanes that sit out 127
    iterations while their neighbours prefetch, wave 1 has a single live lane (count 1) and 63 lanes of empty buckets"""
    c = 8
    want = [""] * 128
    big = (3, 64, 126) if last_is_one else (3, 64, 127)
    for b in big:
        want[b] = "".join("-" if (i % 7 == 2 and b + 1 < 128) else "+" for i in range(CAP))
    ones = [b for b in range(5, 5 + 62) if not want[b]] + [100]
    for i, b in enumerate(ones):
        want[b] = "-" if i % 4 == 1 else "+"
    if last_is_one:
        want[127] = "+"        # the LAST bucket of the entry array holds one entry: entries[off + 1] would be past the array's end
        want[ones[0]] = ""
    ks, scal = terms_of(c, want, 13 + last_is_one)
    cnt, _ = check_histogram(ks, scal, c, want)
    assert sum(1 for x in cnt if x) == 65 and max(cnt) == CAP and sorted(set(cnt)) == [0, 1, CAP]
    assert cnt[127] == (1 if last_is_one else CAP)
    return c, ks, scal


def case_one_beside_cap():
    return _one_beside_cap(False)


def case_one_last():
    return _one_beside_cap(True)


def case_open_then_cancel():   # a bucket that opens at P and adds -P: the identity as an ordinary point, then one more addition onto it
    c = 6
    want = [""] * 32
    # buckets 4 and 9: -(2G), +(2G), +(3G), the first two terms in either order; buckets 6 and 11 the same without the third entry
    fixed, extra = [], {}
    for b, order, third in ((4, "-+", True), (9, "+-", True), (6, "-+", False), (11, "+-", False)):
        for ch in order:
            if ch == "-":
                fixed.append((2, (1 << c) - (b + 1) + (20 << c)))    # carries into window 1, digit 21: bucket 20
                extra[20] = (extra.get(20, (0, 0))[0] + 1, 0)
            else:
                fixed.append((2, b + 1))
        if third:
            fixed.append((3, b + 1))
        extra[b] = (3 if third else 2, 1)
    for b in range(12, 20):
        want[b] = "+-+"
    for b in range(22, 30):
        want[b] = "++"
    ks, scal = terms_of(c, want, 15, fixed=fixed)
    check_histogram(ks, scal, c, want, extra)
    return c, ks, scal


def case_small_nb():           # nb = 16: a single wave of 16 lanes with buckets, five of them empty, 48 lanes beyond nb
    c = 5
    want = ["+-+", "", "+", "--+", "", "+++++", "-", "", "++", "+-", "", "-+-+", "+", "", "+++", "+"]
    ks, scal = terms_of(c, want, 16)
    check_histogram(ks, scal, c, want)
    return c, ks, scal


def case_all_cancel():         # the all-cancel case of tests/test_msm_lockstep_gpu.py: every bucket sums to the identity
    ks, scal = M.make_case("cancel", 600, list(range(1, 33)), seed=6)
    return 6, ks, scal


CASES = {"singles": case_singles, "pairs": case_pairs, "one_beside_cap": case_one_beside_cap, "one_last": case_one_last,
         "open_then_cancel": case_open_then_cancel, "small_nb": case_small_nb, "all_cancel": case_all_cancel}


def _table(zk, bases, c):
    zk.set_table_model(1)
    try:
        b = zk.Bases.upload(bases).precompute(c)
    finally:
        zk.set_table_model(-1)
    assert b.table_model == 1
    return b


def _run(zk, b, scal, mode):
    zk.set_lockstep(mode, 1)
    try:
        out = zk.jac_to_affine(b.msm(M.canonical_limbs(scal), montgomery=False))
        return out, zk.last_acc_path()
    finally:
        zk.set_lockstep(-1, -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_opening_and_prefetch_agree_with_the_closed_form(zk, oracle_lib, name):
    c, ks, scal = CASES[name]()
    pad = max(0, 256 - len(ks))            # (the size of the neighbouring file's sets; a zero scalar produces no entry)
    ks, scal = ks + [1] * pad, scal + [0] * pad
    assert 4 <= c <= 8 and 256 <= len(ks) <= 1500
    cnt, neg = histogram(ks, scal, c)
    assert max(cnt) <= CAP
    exp = M.closed_form(oracle_lib, ks, scal)
    b = _table(zk, M.bases_of(oracle_lib, ks), c)
    try:
        on, path_on = _run(zk, b, scal, 1)
        off, path_off = _run(zk, b, scal, 0)
    finally:
        b.free()
    print(name, "c", c, "n", len(ks), "max count", max(cnt), "non-empty", sum(1 for x in cnt if x), "negated", sum(neg),
          "route", path_on, path_off)
    assert path_on == 1 and path_off == 0
    assert (on == exp).all() and (off == exp).all()
    if name == "all_cancel":
        assert (on == 0).all()
