"""The layout helpers of the device-layout transform tests (tests/ntt_layout.py) against their definitions; needs no GPU."""
import random

import numpy as np

from oracle import pyref as R
from tests.ntt_layout import abi_ints, from_packed, from_transposed, layout_logk, packed_raw, to_packed, to_transposed
from tests.helpers import fr_array


def test_layout_logk():
    assert [layout_logk(n) for n in (0, 1, 11, 12, 13, 14, 15, 18, 19, 20, 21, 22)] == [0, 0, 0, 6, 7, 7, 8, 9, 10, 10, 11, 11]


def test_transposed_order_is_identity_below_2_12():
    for log_d in (0, 1, 5, 11):
        a = np.arange(1 << log_d, dtype=np.uint64)
        assert (to_transposed(a, log_d) == a).all() and (from_transposed(a, log_d) == a).all()


def test_transposed_order_places_and_inverts():
    for log_d in (12, 13):
        d = 1 << log_d
        K = 1 << layout_logk(log_d)
        N2 = d // K
        assert (K, N2) == ((64, 64) if log_d == 12 else (128, 64))
        a = np.arange(d, dtype=np.uint64)
        t = to_transposed(a, log_d)
        for k1, k2 in ((0, 0), (1, 0), (0, 1), (K - 1, 0), (0, N2 - 1), (K - 1, N2 - 1), (5, 3), (K - 2, N2 // 2)):
            assert t[k1 * N2 + k2] == k1 + K * k2
        assert sorted(t.tolist()) == a.tolist()
        assert (from_transposed(t, log_d) == a).all()
        assert (to_transposed(from_transposed(a, log_d), log_d) == a).all()
        if log_d == 13:
            assert (t != from_transposed(a, log_d)).any()            # unequal factors: the two permutations differ
        rows = np.stack([a, a + np.uint64(d)], axis=1)                # trailing axes travel with their element
        assert (to_transposed(rows, log_d)[:, 1] == t + np.uint64(d)).all()


def test_packed_words_round_trip_and_carry_multiples_of_r():
    rng = random.Random(5)
    xs = [0, 1, R.R_MOD - 1, pow(2, -406, R.R_MOD)] + [rng.randrange(R.R_MOD) for _ in range(60)]
    for m in range(8):
        w = to_packed(xs, m)
        assert w.dtype == np.uint32 and w.shape == (len(xs), 12)
        assert from_packed(w) == xs
        raws = packed_raw(w)
        assert all(m * R.R_MOD <= raw < (m + 1) * R.R_MOD for raw in raws)
        assert (to_packed(from_packed(w), m) == w).all()
    ms = [i % 8 for i in range(len(xs))]
    assert from_packed(to_packed(xs, ms)) == xs
    assert [raw // R.R_MOD for raw in packed_raw(to_packed(xs, ms))] == ms
    assert packed_raw(to_packed([pow(2, -406, R.R_MOD)]))[0] == 1            # the device form of 2^-406 is the word 1


def test_abi_ints():
    xs = [0, 1, 2, R.R_MOD - 1, 12345678901234567890123]
    assert abi_ints(fr_array(xs)) == xs
