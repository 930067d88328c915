"""A phase-2 contribution's lane body without a GPU: zecale_amd/csrc/phase2.cuh common_scalar_mul (the code k_common_scalar_mul runs on
every lane) and the host's recoding of the common scalar, compiled for the HOST by g++, against pyref's big integers.  CPU only."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import verify_fixtures as V
from tests.helpers import aff_limbs

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")
RM = R.R_MOD


def build_shim():
    so = os.path.join(HERE, "libphase2_host_shim.so")
    src = os.path.join(HERE, "phase2_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("phase2.cuh", "sha256.hpp", "pairing.cuh", "ec.cuh", "fp29.cuh", "fp_inv.cuh", "bw6_params.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.phase2_recode.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.phase2_lane.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.phase2_decompose.argtypes = [ctypes.c_void_p] * 4
    lib.phase2_recode_glv.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.phase2_lambda.argtypes = [ctypes.c_void_p]
    lib.phase2_lane_glv.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.sha256_shim.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sha256_pieces_shim.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def shim():
    return build_shim()


def scalars():
    """[(label, k)]: the values of s^-1 the chain must get right"""
    zero_run = (1 << 376) | (1 << 300) | 5                       # 75 and 297 zero digits in a row
    assert zero_run < RM and 3 << 374 < RM
    return [("one", 1), ("r - 1", RM - 1), ("two", 2), ("(r + 1) / 2", (RM + 1) // 2), ("1 / 3", pow(3, -1, RM)),
            ("the recoding carries out of the top digit", 3 << 374), ("a long run of zero digits", zero_run),
            ("ones throughout", (1 << 376) - 1), ("random", random.Random(41).randrange(1, RM))]


def recode(shim, k):
    digits = np.zeros(shim.phase2_digit_buffer(), dtype=np.int8)
    words = np.array(R.int_to_limbs(k, 6), dtype=np.uint64)
    n = shim.phase2_recode(words.ctypes.data, digits.ctypes.data)
    return [int(d) for d in digits[:n]], digits


def test_recoding_reproduces_the_scalar_in_non_adjacent_form(shim):
    """sum d_i 2^i = k with digits in {-1, 0, 1}, no two neighbours both non-zero, the top digit 1, at most one digit more than the
    binary form, nothing behind the last digit; the all-ones value of 384 bits carries into the working copy's seventh word"""
    for label, k in scalars() + [("zero", 0), ("2^384 - 1", (1 << 384) - 1), ("r", RM)]:
        d, buf = recode(shim, k)
        assert sum(x << i for i, x in enumerate(d)) == k, label
        assert all(x in (-1, 0, 1) for x in d), label
        assert all(not (a and b) for a, b in zip(d, d[1:])), label
        assert len(d) <= k.bit_length() + 1 and (not d or d[-1] == 1), label
        assert not buf[len(d):].any(), label
    assert len(recode(shim, 3 << 374)[0]) == (3 << 374).bit_length() + 1       # the case that is one digit longer
    assert len(recode(shim, (1 << 384) - 1)[0]) == 385


def lane(shim, P, k):
    p = np.ascontiguousarray(aff_limbs(P), dtype=np.uint64)
    words = np.array(R.int_to_limbs(k, 6), dtype=np.uint64)
    o = np.full(24, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    shim.phase2_lane(p.ctypes.data, words.ctypes.data, o.ctypes.data)
    return o


def test_lane_body_equals_pyref_on_every_scalar_and_point(shim):
    """k P, limb for limb (affine Montgomery limbs are canonical): the generator, small multiples, a random multiple and the point at
    infinity, which stays there.  For a scalar below r no partial sum of the chain is +-P when P is added, so the addition's same-x
    branch is reached by k = r alone (the last assertion); r - 1 ends in a doubling."""
    pts = [("g1", R.G1_GEN)] + [("%d g1" % m, V.g1mul(m)) for m in (2, 3, 5)] + [("random multiple", V.g1mul(random.Random(7).randrange(1, RM)))]
    for sl, k in scalars():
        for pl, P in pts:
            assert (lane(shim, P, k) == aff_limbs(R.ec_mul(k, P))).all(), (sl, pl)
        assert not lane(shim, None, k).any(), sl
    assert (lane(shim, R.G1_GEN, RM - 1) == aff_limbs((R.G1_GEN[0], R.Q_MOD - R.G1_GEN[1]))).all()      # (r - 1) P = -P
    assert not lane(shim, R.G1_GEN, RM).any() and not lane(shim, R.G1_GEN, 0).any()                      # r P = 0 P = O


def test_lane_body_on_g2(shim):
    """the formulas never use the curve's b: the same body multiplies a point of G2 (delta_g2 is host work, but nothing forbids it)"""
    k = random.Random(43).randrange(1, RM)
    assert (lane(shim, R.G2_GEN, k) == aff_limbs(R.ec_mul(k, R.G2_GEN))).all()


# ---- the endomorphism form: k = k1 + k2 lambda, phi(x, y) = (omega x, y)

def lam(shim):
    out = np.zeros(6, dtype=np.uint64)
    shim.phase2_lambda(out.ctypes.data)
    return R.limbs_to_int(out)


def decompose(shim, k):
    words = np.array(R.int_to_limbs(k, 6), dtype=np.uint64)
    k1, k2, neg = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.int32)
    ok = shim.phase2_decompose(words.ctypes.data, k1.ctypes.data, k2.ctypes.data, neg.ctypes.data)
    sign = lambda n: -1 if n else 1
    return ok, sign(neg[0]) * R.limbs_to_int(k1), sign(neg[1]) * R.limbs_to_int(k2)


def glv_scalars(shim):
    l = lam(shim)
    return scalars() + [("k2 = 0: a scalar below the bound", 5), ("k2 = 0: 2^188", 1 << 188), ("k1 = 0: lambda", l), ("k1 = 0: 7 lambda", 7 * l % RM),
                        ("-lambda", RM - l), ("lambda^2 = -1 - lambda", l * l % RM)]


def test_the_committed_constants_are_the_endomorphism_of_g1(shim):
    """lambda is a primitive cube root of unity mod r, omega one mod q, and phi(G1_GEN) = (omega x, y) = lambda G1_GEN in pyref - the
    pair, not one of the three other combinations; omega is read back through the lane body: lambda P has P's ordinate"""
    l = lam(shim)
    assert (l * l + l + 1) % RM == 0 and l != 1
    from tools.gen_params import glv_params
    assert glv_params()["lam"] == l      # the committed header is the generator's output
    lp = R.ec_mul(l, R.G1_GEN)
    assert lp[1] == R.G1_GEN[1] and lp[0] != R.G1_GEN[0] and pow(lp[0] * pow(R.G1_GEN[0], -1, R.Q_MOD), 3, R.Q_MOD) == 1
    assert (lane_glv(shim, R.G1_GEN, l) == aff_limbs(lp)).all()


def test_decomposition_reproduces_the_scalar_within_its_bound(shim):
    """k1 + k2 lambda = k (mod r) with |k1|, |k2| < 2^GLV_BITS, on the named scalars and a few hundred random ones; a scalar below the
    bound keeps k2 = 0, a small multiple of lambda k1 = 0"""
    l, bound = lam(shim), 1 << shim.phase2_glv_bits()
    assert shim.phase2_glv_bits() <= 191 and shim.phase2_glv_digits() >= shim.phase2_glv_bits() + 1
    rng = random.Random(5)
    for label, k in glv_scalars(shim) + [("zero", 0)] + [("random %d" % i, rng.randrange(RM)) for i in range(300)]:
        ok, k1, k2 = decompose(shim, k)
        assert ok == 1, label
        assert (k1 + k2 * l - k) % RM == 0, label
        assert abs(k1) < bound and abs(k2) < bound, label
    assert decompose(shim, 5) == (1, 5, 0) and decompose(shim, 1 << 188) == (1, 1 << 188, 0)
    assert decompose(shim, l) == (1, 0, 1) and decompose(shim, 7 * l % RM) == (1, 0, 7)
    assert decompose(shim, RM - l) == (1, 0, -1)


def test_endomorphism_digits_reproduce_both_halves(shim):
    for label, k in glv_scalars(shim):
        digits = np.zeros(shim.phase2_digit_buffer(), dtype=np.int8)
        words = np.array(R.int_to_limbs(k, 6), dtype=np.uint64)
        n = shim.phase2_recode_glv(words.ctypes.data, digits.ctypes.data)
        half = shim.phase2_glv_digits()
        d1, d2 = [int(d) for d in digits[:half]], [int(d) for d in digits[half:]]
        _, k1, k2 = decompose(shim, k)
        assert sum(x << i for i, x in enumerate(d1)) == k1 and sum(x << i for i, x in enumerate(d2)) == k2, label
        assert 0 <= n <= half and not any(d1[n:]) and not any(d2[n:]), label
        for d in (d1, d2):
            assert all(not (a and b) for a, b in zip(d, d[1:])), label


def lane_glv(shim, P, k):
    p = np.ascontiguousarray(aff_limbs(P), dtype=np.uint64)
    words = np.array(R.int_to_limbs(k, 6), dtype=np.uint64)
    o = np.full(24, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert shim.phase2_lane_glv(p.ctypes.data, words.ctypes.data, o.ctypes.data) >= 0
    return o


def test_endomorphism_lane_body_is_limb_identical_to_the_baseline(shim):
    """the same scalars and points through both lane bodies, and pyref on the decomposition's own cases"""
    pts = [("g1", R.G1_GEN)] + [("%d g1" % m, V.g1mul(m)) for m in (2, 3, 5)] + [("random multiple", V.g1mul(random.Random(7).randrange(1, RM)))]
    for sl, k in glv_scalars(shim):
        for pl, P in pts:
            assert (lane_glv(shim, P, k) == lane(shim, P, k)).all(), (sl, pl)
        assert not lane_glv(shim, None, k).any(), sl
    for sl, k in glv_scalars(shim)[len(scalars()):]:
        assert (lane_glv(shim, R.G1_GEN, k) == aff_limbs(R.ec_mul(k, R.G1_GEN))).all(), sl
    assert not lane_glv(shim, R.G1_GEN, 0).any()
