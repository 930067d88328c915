"""The MSM plan's arithmetic (zecale_amd/csrc/msm_plan.hpp: what msm_plan_init and msm_launch_multi size their buffers and launches
by) compiled by g++ and checked on the CPU: against an independent restatement of the rules as msm.hip stated them inline before
the header existed, and against the bounds that keep the driver inside its allocations.  No GPU, no libzkhip."""
import ctypes
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
U64, U32, INT = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
SIGNATURES = {      # name: (result, arguments)
    "machine_fill": (U64, []), "total_terms": (U64, [INT, U64, U64]), "digits": (INT, [INT, INT]),
    "window_layout": (None, [INT, ctypes.c_void_p, ctypes.c_void_p]),
    "sort_plan": (INT, [INT, INT, INT, U64, U64, U64, U32, ctypes.c_void_p]), "ceil_div": (U64, [U64, U64]), "hist_m": (U64, [U64, U32, U64]),
    "slice_rule": (U64, [U64, U64]), "slice_plan": (INT, [U64, U64, U64, U64, ctypes.c_void_p]), "slice_run": (U64, [U64, U64, U64, U64, U32]),
    "level_bound": (U64, [U64, U64]), "aff_m_cap": (U64, [U32]), "aff_lanes": (U32, [U32, INT, U64]), "aff_outputs_per_lane": (U32, [U64, U32]),
    "aff_scratch_bytes": (U64, []), "lock_min_live": (U32, [INT]),
    "lo_bits": (INT, [INT]), "hi_bits": (INT, [INT]),
    "tree_fan_in": (INT, [INT, U64, U32, U64]), "group_fan_in": (INT, [INT, U64, U64]),
    "cap_entries": (U64, [INT, U64]), "cap_block_tot": (U64, [U64, U64, U64]), "cap_fix_list": (U64, [U32]), "cap_fix_short": (U64, [U32]),
    "cap_segS": (U64, [U64]), "cap_segR": (U64, [U64, INT]), "cap_sumR": (U64, [U64, INT, INT]), "cap_Rlevels": (U64, [INT]), "cap_hilo": (U64, [INT, INT]),
}


class Plan:
    """msm_plan.hpp through tests/msm_plan_host_shim.cpp"""

    def __init__(self, lib):
        for name, (res, args) in SIGNATURES.items():
            f = getattr(lib, "p_" + name)
            f.restype, f.argtypes = res, args
            setattr(self, name, f)

    def sort(self, c, merged, Wd, nb, max_n, want_parts, tile_knob):
        out = (U64 * 5)()
        if not self.sort_plan(c, merged, Wd, nb, max_n, want_parts, tile_knob, out):
            return None
        return dict(zip(("LB", "NP", "bins", "tile", "hist_len"), out))

    def slices(self, m_max, nb, target, slot_words):
        out = (U64 * 3)()
        if not self.slice_plan(m_max, nb, target, slot_words, out):
            return None
        return dict(zip(("S", "T", "slot_stride"), out))


@pytest.fixture(scope="module")
def P():
    so = os.path.join(HERE, "libmsm_plan_host_shim.so")
    src = os.path.join(HERE, "msm_plan_host_shim.cpp")
    hdr = os.path.join(HERE, "..", "zecale_amd", "csrc", "msm_plan.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    return Plan(ctypes.CDLL(so))


# ---- the grid ---------------------------------------------------------------------------------------------------------------
CS = (4, 5, 8, 11, 13, 16, 18, 22)           # (22: merged plans only; a plain plan stops at 18)
MAX_NS = (1, 255, 256, 1000, (1 << 14) + 1, 1 << 20, 1 << 22)
KNOBS = ((1024, 1024), (64, 256), (8192, 16384))      # ZKHIP_SORT_PARTS, ZKHIP_SORT_TILE: the defaults and both ends of their ranges
TARGET = 80                                   # ZKHIP_SLICE_TARGET's default
SLOT_WORDS, LOCK_KEYS, W_NEXT = 112, 130, 8   # ec_mem.cuh (448-byte slots), ZK_LOCK_KEYS, ZK_W_NEXT
AFF_LEVELS = (0, 1, 3)


def shapes():
    """(c, merged, K, max_n, total_terms as given): the shapes msm_plan_init's own argument checks let through"""
    for c, merged, K, max_n in itertools.product(CS, (0, 1, 2), (1, 5), MAX_NS):
        if (not merged and K != 1) or c > (22 if merged else 18):
            continue
        for given in (0, max(1, K * max_n * 3 // 5), max(1, max_n // 2)):
            yield c, merged, K, max_n, given


# ---- the rules restated, as msm_plan_init and msm_launch_multi stated them inline ------------------------------------------
def ref_total_terms(K, max_n, total_terms):
    if total_terms == 0 or total_terms > K * max_n:
        total_terms = K * max_n
    if total_terms < max_n and K == 1:
        total_terms = max_n
    return total_terms


def ref_digits(c, merged):
    return 378 // (c + 1) + 2 if merged == 2 else (378 + c - 1) // c


def ref_sort(c, merged, Wd, nb, max_n, want_parts, tile_knob):
    B = 1 << (c - 1)
    LB = min(c - 1, 10)
    while LB > 6 and (nb >> LB) < want_parts and (B >> (LB - 1)) * (1 if merged else Wd) <= 4096:
        LB -= 1
    NP = B >> LB
    bins = NP if merged else NP * Wd
    if bins * 8 > 60 * 1024:
        return None
    tile = tile_knob & ~255
    while (max_n + tile - 1) // tile > 1024:
        tile *= 2
    nbx = (max_n + tile - 1) // tile
    return dict(LB=LB, NP=NP, bins=bins, tile=tile, hist_len=(nb >> LB) * (nbx or 1) + 1)


def ref_slice_base(m):
    lanes = 131072
    fills = max(1, (m + lanes * TARGET - 1) // (lanes * TARGET))
    return max(16, (m + lanes * fills - 1) // (lanes * fills))


def ref_slice_plan(m_max, nb):
    S = ref_slice_base(m_max)
    max_slots = ((1 << 32) - 1) // (SLOT_WORDS * 4)
    if nb + 64 >= max_slots:
        return None
    while nb + 2 * ((m_max + S - 1) // S) >= max_slots:
        S += (S + 7) // 8
    T = (m_max + S - 1) // S
    if (nb + 2 * T) * SLOT_WORDS * 4 >= 1 << 32:
        return None
    return dict(S=S, T=T, slot_stride=nb + 2 * T)


def ref_slice_run(m, one_stream, mult, live_buckets, T):
    S = ref_slice_base(m)
    if one_stream:
        S *= mult
    avg = m // (live_buckets or 1)
    if S < (avg + 1) // 2:
        S = (avg + 1) // 2
    while (m + S - 1) // S > T:
        S += 1
    return S, (m + S - 1) // S


def ref_level_bound(m, nb):
    return (m + min(m, nb)) // 2


def accepted(P, c, merged, K, max_n, given, knobs=KNOBS[0], levels=0):
    """The plan msm_plan_init makes from the header's figures, or None where it returns ZKHIP_ERR_ARG."""
    total = P.total_terms(K, max_n, given)
    Wd = P.digits(c, merged)
    W = K if merged else Wd
    nb = (1 << (c - 1)) * W
    if Wd * max_n >= 1 << 31 or Wd * total >= 1 << 32 or Wd * total * W_NEXT >= 1 << 32:      # (msm_plan_init's own checks)
        return None
    sort = P.sort(c, merged, Wd, nb, max_n, *knobs)
    if sort is None:
        return None
    m_acc = Wd * total
    for _ in range(levels):
        m_acc = P.level_bound(m_acc, nb)
    sl = P.slices(m_acc, nb, TARGET, SLOT_WORDS)
    if sl is None:
        return None
    return dict(c=c, merged=merged, K=K, max_n=max_n, total=total, Wd=Wd, W=W, nb=nb, m_acc=m_acc, **sort, **sl)


# ---- restatement checks ------------------------------------------------------------------------------------------------------
def test_machine_fill_is_the_one_constant(P):
    assert P.machine_fill() == 131072
    assert P.lock_min_live(256) == 131072 and P.lock_min_live(0) == 131072 and P.lock_min_live(64) == 64 * 2 * 4 * 64


def test_total_terms_and_digits_as_before(P):
    for c, merged, K, max_n, given in shapes():
        assert P.total_terms(K, max_n, given) == ref_total_terms(K, max_n, given)
        assert P.digits(c, merged) == ref_digits(c, merged)
    assert P.total_terms(5, 1000, 10 ** 9) == 5000 and P.total_terms(1, 1000, 10) == 1000 and P.total_terms(5, 1000, 10) == 10


def test_sort_geometry_as_before(P):
    n = 0
    for (c, merged, K, max_n, given), knobs in itertools.product(shapes(), KNOBS):
        Wd = ref_digits(c, merged)
        nb = (1 << (c - 1)) * (K if merged else Wd)
        assert P.sort(c, merged, Wd, nb, max_n, *knobs) == ref_sort(c, merged, Wd, nb, max_n, *knobs), (c, merged, K, max_n, knobs)
        n += 1
    assert n > 1000
    # the refusal: more (part, window) counters than k_digit_pass<1> has LDS for - a geometry no knob setting of msm_plan_init reaches
    assert P.sort(20, 0, 64, 64 << 19, 1000, 64, 1024) is None and ref_sort(20, 0, 64, 64 << 19, 1000, 64, 1024) is None


def test_plan_slices_as_before_and_refused_alike(P):
    seen = {"accepted": 0, "refused": 0, "grown": 0}
    for (c, merged, K, max_n, given), levels in itertools.product(shapes(), AFF_LEVELS):
        total = ref_total_terms(K, max_n, given)
        Wd = ref_digits(c, merged)
        nb = (1 << (c - 1)) * (K if merged else Wd)
        if Wd * max_n >= 1 << 31 or Wd * total >= 1 << 32 or Wd * total * W_NEXT >= 1 << 32:
            continue
        m = Wd * total
        for _ in range(levels):
            assert P.level_bound(m, nb) == ref_level_bound(m, nb)
            m = ref_level_bound(m, nb)
        exp = ref_slice_plan(m, nb)
        got = P.slices(m, nb, TARGET, SLOT_WORDS)
        assert got == exp, (c, merged, K, max_n, given, levels)
        got_plan = accepted(P, c, merged, K, max_n, given, levels=levels)
        assert (got_plan is None) == (exp is None)
        seen["accepted" if exp else "refused"] += 1
        if exp and exp["S"] > ref_slice_base(m):
            seen["grown"] += 1
    assert seen["accepted"] > 500 and seen["refused"] > 0 and seen["grown"] > 0, seen      # every branch of the rule was walked


def launch_ms(m_max):
    return sorted({m for m in (1, 15, 16, m_max // 3, m_max - 1, m_max) if 1 <= m <= m_max})


def test_launch_slices_as_before_and_inside_the_plan(P):
    n = 0
    for (c, merged, K, max_n, given), levels in itertools.product(shapes(), AFF_LEVELS):
        pl = accepted(P, c, merged, K, max_n, given, levels=levels)
        if pl is None:
            continue
        B = 1 << (c - 1)
        for m, one_stream, mult, n_jobs in itertools.product(launch_ms(pl["m_acc"]), (0, 1), (1, 2, 16), sorted({1, K})):
            live = B * n_jobs if merged else pl["nb"]
            S = P.slice_run(m, TARGET, mult if one_stream else 1, live, pl["T"])
            T_run = (m + S - 1) // S
            assert (S, T_run) == ref_slice_run(m, one_stream, mult, live, pl["T"]), (pl, m, one_stream, mult, n_jobs)
            assert 1 <= T_run <= pl["T"] and S < 1 << 32
            # the two stitching lists: a bucket on either list spans at least two (five) of the launch's T_run slices
            assert P.cap_fix_short(pl["T"]) >= T_run // 2 and P.cap_fix_list(pl["T"]) >= T_run // 5
            n += 1
    assert n > 10000


def test_affine_level_launches_as_before(P):
    for aff_m, m_out in itertools.product((4, 64, 512), (1, 1000, 131072 * 32 - 1, 131072 * 32, 131072 * 64 * 3 // 2, 10 ** 7, 10 ** 8, 3 * 10 ** 9)):
        exp, fill = aff_m, 131072
        rounds = (m_out + fill * aff_m // 2) // (fill * aff_m)
        if rounds >= 1:
            mm = (m_out + fill * rounds - 1) // (fill * rounds)
            exp = min(mm, aff_m * 3 // 2)
        assert P.aff_outputs_per_lane(m_out, aff_m) == exp
        assert P.aff_m_cap(aff_m) == aff_m * 3 // 2 and exp <= P.aff_m_cap(aff_m)
        lanes = 1 << 18
        while lanes * (aff_m * 3 // 2) * 108 >= 1 << 32:
            lanes >>= 1
        assert P.aff_lanes(aff_m, 0, m_out) == lanes
        need = (m_out + aff_m - 1) // aff_m
        assert P.aff_lanes(aff_m, 2, m_out) == ((need + 255) & ~255 if need < lanes else lanes)
        # one buffer descriptor: the scratch of a launch stays below 4 GiB
        assert P.aff_lanes(aff_m, 2, m_out) * P.aff_m_cap(aff_m) * P.aff_scratch_bytes() < 1 << 32


# ---- invariant checks: the comments beside the hipMalloc lines, as assertions ----------------------------------------------
@pytest.mark.parametrize("c", CS)
def test_windows_tile_the_scalar(P, c):
    W = (378 + c - 1) // c
    off, bits = (ctypes.c_uint16 * 96)(), (ctypes.c_uint8 * 96)()
    P.window_layout(c, off, bits)
    assert W <= 96 and off[0] == 0
    assert all(off[w + 1] == off[w] + bits[w] for w in range(W - 1)) and off[W - 1] + bits[W - 1] == 378
    assert all(bits[w] in (c, c - 1) for w in range(W)) and all(bits[w] >= bits[w + 1] for w in range(W - 1))
    assert all(bits[w] == 0 and off[w] == 0 for w in range(W, 96))      # nothing written past the last window


def test_plan_buffers_hold_every_launch(P):
    n = 0
    for (c, merged, K, max_n, given), knobs in itertools.product(shapes(), KNOBS):
        pl = accepted(P, c, merged, K, max_n, given, knobs=knobs)
        if pl is None:
            continue
        nb, LB, tile = pl["nb"], pl["LB"], pl["tile"]
        # the sort's histogram: hist_m(n) <= hist_len for every n <= max_n.  A launch of n_max terms has nbx = ceil_div(n_max, tile)
        # blocks: every count from 1 to the plan's own is walked, and ceil_div is checked to land inside that range
        nbx_max = P.ceil_div(max_n, tile)
        assert 1 <= nbx_max <= 1024
        assert all(P.hist_m(nb, LB, nbx) <= pl["hist_len"] for nbx in range(1, nbx_max + 1)), pl
        for nn in sorted({1, tile - 1, tile, tile + 1, max_n // 2, max_n - 1, max_n}):
            if 1 <= nn <= max_n:
                assert P.ceil_div(nn, tile) == -(-nn // tile) and 1 <= P.ceil_div(nn, tile) <= nbx_max
        assert LB <= 10 and pl["bins"] * 8 <= 60 * 1024 and pl["NP"] << LB == 1 << (c - 1) and tile % 256 == 0
        # the slot array behind ONE buffer descriptor; the entry list's positions and the slice weights in 32 bits
        assert pl["slot_stride"] == nb + 2 * pl["T"] and (nb + 2 * pl["T"]) * 448 < 1 << 32
        assert pl["T"] == (pl["m_acc"] + pl["S"] - 1) // pl["S"] and pl["S"] >= 16
        assert P.cap_entries(pl["Wd"], pl["total"]) == pl["Wd"] * pl["total"] + 1 < 1 << 32
        # block_tot: the block totals of the launch's four scans, and words [0..2] after them
        cap = P.cap_block_tot(nb, pl["hist_len"], LOCK_KEYS)
        for scan_m in (pl["hist_len"], nb, nb + 1, LOCK_KEYS * ((nb + 1023) // 1024)):
            assert (scan_m + 1023) // 1024 <= cap
        assert cap >= 3
        n += 1
    assert n > 1000


def reduction_walk_shapes():
    return sorted({(c, K if merged else ref_digits(c, merged)) for c, merged, K, _, _ in shapes()})


@pytest.mark.parametrize("L", (4, 8, 16, 32))
@pytest.mark.parametrize("quad_below", (1, 65536, 1 << 30))
def test_reduction_launches_fit_their_buffers(P, L, quad_below):
    """stage_reduce's loops walked on the CPU: every launch's output count against the capacity of the buffer it writes."""
    for c, W in reduction_walk_shapes():
        nb, G = (1 << (c - 1)) * W, 2 * W
        Rr, Hh = 1 << P.lo_bits(c), 1 << P.hi_bits(c)
        Nn = max(Rr, Hh)
        assert (P.lo_bits(c), P.hi_bits(c)) == (c // 2, c - 1 - c // 2)
        assert P.lo_bits(c) >= 2 and P.hi_bits(c) >= 1          # both trees have a level: no `left == 1` case
        for left, cap in ((Rr, P.cap_segS(nb)), (Hh, P.cap_segS(nb))):      # row tree -> segS, column tree -> colS (same capacity)
            n_in, rows = nb, nb // left
            while left > 1:
                fan = P.tree_fan_in(L, n_in, left, quad_below)
                assert fan >= 2 and left % fan == 0 and n_in % fan == 0
                n_in //= fan
                left //= fan
                assert n_in <= cap, (c, W, L, quad_below)
            assert n_in == rows                                              # one item per row / column is left
        assert G * Nn <= P.cap_hilo(W, c)                                    # k_place_hilo
        n_cur, level, r_off = G * Nn, 0, 0
        while n_cur > G:
            fan = P.group_fan_in(L, n_cur, G)
            assert fan >= 2 and n_cur % fan == 0
            n_out = n_cur // fan
            assert n_out <= P.cap_segS(nb)                                   # k_seg: S
            assert r_off + n_out <= P.cap_segR(nb, W), (c, W, L)             # k_seg: this level's R array, back to back in segR
            assert (level + 1) * G <= P.cap_Rlevels(W) and level < 32        # Rlevels[level], LevelShifts
            rn = n_out
            while rn > G:                                                    # the R-sum tree
                fs = P.group_fan_in(L, rn, G)
                assert fs >= 2 and rn % fs == 0
                rn //= fs
                if rn != G:
                    assert rn <= P.cap_sumR(nb, W, L), (c, W, L)
            assert rn == G
            r_off += n_out
            n_cur, level = n_out, level + 1
        assert n_cur == G and G <= P.cap_sumR(nb, W, L)                      # k_window_combine's accumulators
