"""What the tests of the transform passes in device layout (tests/test_ntt_layout_gpu.py) know about that layout, in numpy and
Python integers only: the transposed order of vectors of 2^12 elements and more, and the packed device words of an element."""
import numpy as np

from oracle import pyref as R

DEV_BITS = 406                      # device Montgomery radix 2^(29 * 14)
_TO_DEV = pow(2, DEV_BITS, R.R_MOD)
_FROM_DEV = pow(_TO_DEV, -1, R.R_MOD)
_FROM_ABI = pow(pow(2, 384, R.R_MOD), -1, R.R_MOD)


def layout_logk(log_d):
    """log2 K of the transposed order (ntt_layout_logk): 0 = the vector is in natural order on both sides of a transform."""
    return 0 if log_d <= 11 else (log_d + 1) // 2


def to_transposed(a, log_d):
    """natural -> transposed order along the first axis: element k1 + K k2 goes to location k1 N2 + k2 (a copy; the identity
    below 2^12)."""
    a = np.asarray(a)
    assert a.shape[0] == 1 << log_d
    lk = layout_logk(log_d)
    if lk == 0:
        return a.copy()
    K, N2 = 1 << lk, 1 << (log_d - lk)
    return np.ascontiguousarray(a.reshape((N2, K) + a.shape[1:]).swapaxes(0, 1)).reshape(a.shape)       # [k2, k1] -> [k1, k2]


def from_transposed(t, log_d):
    """transposed -> natural order: the element at location k1 N2 + k2 goes to index k1 + K k2."""
    t = np.asarray(t)
    assert t.shape[0] == 1 << log_d
    lk = layout_logk(log_d)
    if lk == 0:
        return t.copy()
    K, N2 = 1 << lk, 1 << (log_d - lk)
    return np.ascontiguousarray(t.reshape((K, N2) + t.shape[1:]).swapaxes(0, 1)).reshape(t.shape)       # [k1, k2] -> [k2, k1]


def to_packed(ints, extra_r=0):
    """Canonical integers x in [0, r) -> uint32 [n, 12], the packed device words of x 2^406 mod r + m r.  extra_r: one m for all or
    one per element; the total must stay below 2^384."""
    ints = list(ints)
    ms = [extra_r] * len(ints) if isinstance(extra_r, int) else [int(m) for m in extra_r]
    assert len(ms) == len(ints)
    out = np.zeros((len(ints), 12), dtype=np.uint32)
    for i, (x, m) in enumerate(zip(ints, ms)):
        assert 0 <= x < R.R_MOD and m >= 0
        raw = x * _TO_DEV % R.R_MOD + m * R.R_MOD
        assert raw < 1 << 384
        out[i] = [(raw >> (32 * k)) & 0xFFFFFFFF for k in range(12)]
    return out


def packed_raw(words):
    """uint32 [n, 12] -> the stored integers (below 2^384), as they are."""
    w = np.asarray(words, dtype=np.uint32).reshape(-1, 12)
    return [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in w]


def from_packed(words):
    """uint32 [n, 12] -> the canonical integers the words stand for: stored value / 2^406 mod r."""
    return [raw * _FROM_DEV % R.R_MOD for raw in packed_raw(words)]


def abi_ints(arr):
    """uint64 [n, 6] ABI limbs -> canonical integers (tests.helpers.fr_ints with the radix inverted once)."""
    return [R.limbs_to_int(row) * _FROM_ABI % R.R_MOD for row in np.asarray(arr).reshape(-1, 6)]
