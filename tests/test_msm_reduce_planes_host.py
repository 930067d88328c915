"""The plane arithmetic of the bucket reduction's tail (zecale_amd/csrc/msm_plan.hpp: tail_weight_planes, tail_fan_in,
tail_level_outputs, cap_tail - what enqueue_tail in msm.hip sizes its launches and buffers by), compiled by g++ and checked on the
CPU.  The launch loop of enqueue_tail and the indexing of k_plane_sum / k_plane_combine are walked here on integer stand-ins for the
points: selecting by weight bit, summing level by level and recombining with doublings gives sum (i+1) x_i.  No GPU, no libzkhip."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
U64, INT = ctypes.c_uint64, ctypes.c_int
SIGNATURES = {
    "lo_bits": (INT, [INT]), "hi_bits": (INT, [INT]), "fan_in_const": (INT, []), "weight_planes": (INT, [U64]), "planes": (INT, [U64, INT]),
    "fan_in": (INT, [U64]), "levels": (INT, [U64]), "level_outputs": (U64, [INT, INT, U64, INT]), "cap_tail": (U64, [INT, U64, INT]),
    "cap_hilo": (U64, [INT, INT]),
}
MAX_LAUNCHES = 8        # behind the row and column trees: k_place_hilo, the levels, k_plane_combine


class Tail:
    def __init__(self, lib):
        for name, (res, args) in SIGNATURES.items():
            f = getattr(lib, "t_" + name)
            f.restype, f.argtypes = res, args
            setattr(self, name, f)


@pytest.fixture(scope="module")
def T():
    so = os.path.join(HERE, "libmsm_reduce_planes_host_shim.so")
    src = os.path.join(HERE, "msm_reduce_planes_host_shim.cpp")
    hdr = os.path.join(HERE, "..", "zecale_amd", "csrc", "msm_plan.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    return Tail(ctypes.CDLL(so))


NS = [1 << k for k in range(1, 12)]      # 2 .. 2048


@pytest.mark.parametrize("N", NS)
def test_plane_counts(T, N):
    """weights 1 .. N need floor(log2 N) + 1 bits; a NAF plan adds the all-ones plane"""
    assert T.weight_planes(N) == N.bit_length() == len(bin(N)) - 2
    assert (1 << T.weight_planes(N)) > N >= (1 << (T.weight_planes(N) - 1))
    assert T.planes(N, 0) == T.weight_planes(N) and T.planes(N, 1) == T.weight_planes(N) + 1
    assert 2 * T.weight_planes(N) <= 64       # k_plane_combine: a quad per (plane, hi / lo) inside one workgroup of 256 lanes


@pytest.mark.parametrize("W", (1, 5))
@pytest.mark.parametrize("c", range(4, 23))
def test_levels_fit_the_planned_buffers(T, c, W):
    """enqueue_tail's loop for the plan at window c: fan-ins divide what is left, every level's outputs fit the buffer it writes
    (level l -> planes[l & 1]), the launches stay within the budget, and the item array is the plan's hilo buffer."""
    N, G = 1 << max(T.lo_bits(c), T.hi_bits(c)), 2 * W
    assert N == 1 << T.lo_bits(c) and 4 <= N <= 2048
    assert G * N <= T.cap_hilo(W, c)
    for total in (0, 1):
        P = T.planes(N, total)
        left, level = N, 0
        while left > 1:
            L = T.fan_in(left)
            assert 2 <= L <= T.fan_in_const() and left % L == 0
            n_out = T.level_outputs(P, G, N, level)
            assert n_out == P * G * (left // L)
            assert n_out <= T.cap_tail(W, N, level & 1), (c, W, total, level)
            assert n_out * 4 < 1 << 31        # lanes of the launch: 32-bit thread indices in k_plane_sum
            left //= L
            level += 1
        assert level == T.levels(N)
        assert T.level_outputs(P, G, N, level - 1) == P * G            # one point per (plane, group) reaches k_plane_combine
        assert 1 + level + 1 <= MAX_LAUNCHES, (c, level)


def walk_tail(T, items, G, N, lo_bits, total):
    """enqueue_tail with integers for points: the launches' index arithmetic as k_plane_sum / k_plane_combine state it.
    items: [G * N]; returns ([W results], [W totals] or None)"""
    W, wp, P = G // 2, T.weight_planes(N), T.planes(N, total)
    cur, left, level = items, N, 0
    while left > 1:
        L = T.fan_in(left)
        per_plane, per_out = G * left, G * left // L
        n_out = T.level_outputs(P, G, N, level)
        assert n_out == P * per_out
        out = [0] * n_out
        for t in range(n_out):
            p, r = divmod(t, per_out)
            for u in range(L):
                i = r * L + u
                if level == 0:
                    if not (total and p == wp) and not ((i % left) + 1) >> p & 1:
                        continue
                    out[t] += cur[i]
                else:
                    out[t] += cur[p * per_plane + i]
        cur, left, level = out, left // L, level + 1
    assert len(cur) == P * G
    res = []
    for w in range(W):
        slot = lambda k: (k % wp) * G + (w if k < wp else W + w)
        acc = {k: cur[slot(k)] << ((k % wp) + (lo_bits if k < wp else 0)) for k in range(2 * wp)}
        d = 1
        while d < 2 * wp:
            for s in range(0, 2 * wp, 2 * d):
                if s + d < 2 * wp:
                    acc[s] += acc[s + d]
            d *= 2
        res.append(acc[0])
    return res, ([cur[wp * G + W + w] for w in range(W)] if total else None)


@pytest.mark.parametrize("N", NS)
def test_select_and_recombine_is_the_weighted_sum(T, N):
    rng = random.Random(N)
    for W, lo_bits, total in ((1, N.bit_length() - 1, 0), (1, 3, 1), (5, N.bit_length() - 1, 1)):
        G = 2 * W
        for fill in ("random", "ones", "single_first", "single_last"):
            if fill == "random":
                items = [rng.randrange(1 << 64) for _ in range(G * N)]
            elif fill == "ones":
                items = [1] * (G * N)
            else:
                items = [0] * (G * N)
                for g in range(G):
                    items[g * N + (0 if fill == "single_first" else N - 1)] = 1 + g
            got, tot = walk_tail(T, items, G, N, lo_bits, total)
            for w in range(W):
                hi = sum((i + 1) * items[w * N + i] for i in range(N))
                lo = sum((i + 1) * items[(W + w) * N + i] for i in range(N))
                assert got[w] == (hi << lo_bits) + lo, (N, W, fill)
                if total:
                    assert tot[w] == sum(items[(W + w) * N:(W + w + 1) * N])
