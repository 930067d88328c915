"""Adversarial MSM inputs with closed-form results (test-side helpers, no GPU needed to build them).

Bases come from the tiny set {O, +-G, +-2G, +-3G} of G1 or G2, made by the C oracle's scalar multiplication and a negation
y -> q - y, then tiled: every base is a known multiple k_i G, so the MSM is (sum s_i k_i mod r) G - one scalar multiplication
at any length.  The structures put the same x coordinate into the additions of every bucket, run, piece and row of the bucket
method (P + P, P + (-P), cancel-then-reopen), whatever order the bucket sort leaves inside a bucket.

The scalar families aim at the signed-digit recoding of zecale_amd/csrc/msm.hip: window_layout (W = ceil(378 / c) windows, the top
W c - 378 of them c - 1 bits wide) and the carry recoding of k_digit_pass (a window value above 2^(cw-1) becomes negative and carries
into the next window), and the width-(c+1) non-adjacent form of the NAF tables (merged == 2).  recode_plain / recode_naf mirror
those loops in Python; tests/test_msm_cases.py checks that the families really produce the digits they are meant to."""
import random

import numpy as np

from oracle import pyref as R
from tests.helpers import aff_limbs, aff_point, fr_limbs

BITS = 378          # the span of bits the windows tile (r < 2^377)
SMALL_KS = (0, 1, -1, 2, -2, 3, -3)


# ---------------------------------------------------------------- mirrors of the device recoding
def window_layout(c):
    """[(offset, bits)] of the W = ceil(378 / c) windows: the top W c - 378 windows get c - 1 bits (msm.hip window_layout)."""
    W = (BITS + c - 1) // c
    n_small = W * c - BITS
    out, bit = [], 0
    for w in range(W):
        cw = c - 1 if w >= W - n_small else c
        out.append((bit, cw))
        bit += cw
    return out


def recode_plain(s, c):
    """Signed digits of s, one per window (k_digit_pass, plain and one-level-per-window tables): d = window value + carry; above
    2^(cw-1) it becomes d - 2^cw and carries 1.  Returns [(offset, digit)] for every window, zero digits included."""
    out, carry = [], 0
    for off, cw in window_layout(c):
        d = ((s >> off) & ((1 << cw) - 1)) + carry
        if d > 1 << (cw - 1):
            d, carry = d - (1 << cw), 1
        else:
            carry = 0
        out.append((off, d))
    assert carry == 0, "a carry out of the top window"         # cannot happen below r (bit 377 is zero)
    return out


def recode_naf(s, c):
    """Width-(c+1) NAF of s as k_digit_pass<NAF> computes it: skip the bits that produce zeros, take c + 1 bits plus the carry (odd),
    above 2^c it becomes negative and carries; at most Wd = 378 // (c + 1) + 2 digits.  Returns [(bit position, odd digit)]."""
    wbits, W = c + 1, BITS // (c + 1) + 2
    pos, carry, out = 0, 0, []
    while pos < 379 and len(out) < W:
        v32 = (s >> pos) & 0xFFFFFFFF if pos < 384 else 0
        run = (~v32 & 0xFFFFFFFF) if carry else v32
        if run & 1 == 0:
            pos += ((run & -run).bit_length() - 1) if run else 32
            continue
        win = (v32 & ((1 << wbits) - 1)) + carry
        if win > 1 << (wbits - 1):
            d, carry = win - (1 << wbits), 1
        else:
            d, carry = win, 0
        out.append((pos, d))
        pos += wbits
    return out


def digits_value(digits):
    return sum(d << pos for pos, d in digits)


# ---------------------------------------------------------------- scalar families
def tiny_values(c):
    """Few distinct values: heavy buckets, long stitching chains, the mag == 1 ballot path of k_digit_pass."""
    return [0, 1, 2, R.R_MOD - 1, R.R_MOD - 2, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1]


def _from_digits(c, digits_low, top):
    """The scalar whose plain recoding at window c is digits_low (all windows but the top) followed by `top`; the top digit is
    lowered until the scalar is below r (and raised to keep it non-negative)."""
    lay = window_layout(c)
    low = sum(d << off for (off, _), d in zip(lay[:-1], digits_low))
    off_top, cw_top = lay[-1]
    top = min(top, 1 << (cw_top - 1), (R.R_MOD - 1 - low) >> off_top)
    while low + (top << off_top) < 0:
        top += 1
    return low + (top << off_top)


def boundary_scalars(c, seed=0, n_mixed=6):
    """Scalars that put every window's digit of the plain recoding at window c on an edge of the signed range:
    +2^(cw-1) (the largest magnitude, no carry), -(2^(cw-1) - 1) (window value 2^(cw-1) + 1: negative, with a carry), -1 (window
    value 2^cw - 1, with a carry), a carry that runs through every window (2^k - 1, and 2^k - 1 plus a top digit), the largest top
    digit of the top window (c - 1 bits where 378 is no multiple of c), and random mixtures of those edges.  All below r."""
    lay = window_layout(c)
    W = len(lay)
    half = [1 << (cw - 1) for _, cw in lay]
    off_top = lay[-1][0]
    top_max = min(half[-1], (R.R_MOD - 1) >> off_top)                        # the largest top digit below r
    out = [
        _from_digits(c, half[:-1], half[-1]),                                  # every digit +2^(cw-1)
        _from_digits(c, [-(h - 1) for h in half[:-1]], half[-1]),              # every digit -(2^(cw-1) - 1): a carry out of each
        _from_digits(c, [-1] * (W - 1), half[-1]),                             # every digit -1: window values 2^cw - 1 + carry
        _from_digits(c, [h - 1 for h in half[:-1]], 1),                        # 2^(cw-1) - 1: the largest digit before the sign flips
        (1 << off_top) - 1,                                                    # all ones below the top window: one carry through all
        (1 << 376) - 1,                                                        # ... into the top window as well
        ((top_max - 1) << off_top) + (1 << off_top) - 1,                       # the carry lands on the top window's largest digit
        top_max << off_top,                                                    # the top window alone, at its largest digit
    ]
    rng = random.Random(seed * 1000 + c)
    for _ in range(n_mixed):
        ds = [rng.choice((h, -(h - 1), -1, 1, h - 1, 0)) for h in half[:-1]]
        out.append(_from_digits(c, ds, rng.choice((1, half[-1], half[-1] - 1))))
    assert all(0 <= s < R.R_MOD for s in out)
    return out


def naf_dense_digits(c):
    """Digit lists of the densest width-(c+1) NAFs: a digit at every position k (c + 1), as many as fit below r - all 1, all 2^c - 1
    (the largest positive digit) and all -(2^c - 1) (a carry out of each) under a positive top digit.  [(positions, digits)]."""
    step = c + 1
    out = []
    for low in (1, (1 << c) - 1, -((1 << c) - 1)):
        K = BITS // step + 1
        while True:
            pos = [k * step for k in range(K)]
            top = 1 if low < 0 else low
            s = sum(low << p for p in pos[:-1]) + (top << pos[-1])
            if 0 <= s < R.R_MOD:
                break
            K -= 1
        out.append((pos, [low] * (K - 1) + [top]))
    return out


def naf_worst_scalars(c):
    """Worst cases of the width-(c+1) NAF (merged == 2): the densest digit strings of naf_dense_digits, all-ones runs 2^m - 1 (one
    negative digit, then a carry through the run), and r - 1, r - 2."""
    dense = [sum(d << p for p, d in zip(pos, ds)) for pos, ds in naf_dense_digits(c)]
    runs = [(1 << m) - 1 for m in (c, c + 1, c + 2, 2 * c + 1, 100, 200, 376)]
    return dense + runs + [R.R_MOD - 1, R.R_MOD - 2]


def scalar_pool(cs, seed=0):
    """Every family for the windows cs, deduplicated, in a fixed order."""
    seen, out = set(), []
    for c in cs:
        for s in tiny_values(c) + boundary_scalars(c, seed) + naf_worst_scalars(c):
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out


# ---------------------------------------------------------------- bases and the closed form
_small_cache = {}


def small_multiples(oracle, g2=False):
    """{k: affine limbs of k G} for k in {0, +-1, +-2, +-3} (k = 0: the point at infinity, all-zero limbs), from oracle.scalar_mul
    and y -> q - y; never from the product's fixed-base kernel, which is under test elsewhere."""
    if g2 in _small_cache:
        return _small_cache[g2]
    g = aff_limbs(R.G2_GEN if g2 else R.G1_GEN)
    pts = {0: np.zeros(24, dtype=np.uint64)}
    for k in (1, 2, 3):
        p = oracle.jac_to_affine(oracle.scalar_mul(g, fr_limbs(k)))
        x, y = aff_point(p)
        pts[k] = p
        pts[-k] = aff_limbs((x, R.Q_MOD - y))
        assert oracle.on_curve(pts[-k], g2=g2)
    _small_cache[g2] = pts
    return pts


def bases_of(oracle, ks, g2=False):
    pts = small_multiples(oracle, g2)
    table = np.stack([pts[k] for k in SMALL_KS])
    idx = np.array([SMALL_KS.index(k) for k in ks], dtype=np.int64)
    return table[idx] if len(ks) else np.zeros((0, 24), dtype=np.uint64)


def closed_form(oracle, ks, scalars, g2=False):
    """sum s_i (k_i G) = (sum s_i k_i mod r) G as affine Montgomery limbs (all zero: infinity)."""
    dot = sum(s * k for s, k in zip(scalars, ks)) % R.R_MOD
    g = aff_limbs(R.G2_GEN if g2 else R.G1_GEN)
    return oracle.jac_to_affine(oracle.scalar_mul(g, fr_limbs(dot)))


def canonical_limbs(scalars):
    return np.array([[(s >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)] for s in scalars], dtype=np.uint64).reshape(-1, 6)


def montgomery_limbs(scalars):
    return np.array([R.int_to_limbs(R.to_mont(s, R.R_MOD, 6), 6) for s in scalars], dtype=np.uint64).reshape(-1, 6)


# ---------------------------------------------------------------- structures
STRUCTURES = ("cancel", "runs", "rows", "signs")


def make_case(structure, n, pool, seed, c=None):
    """(ks, scalars) of n terms.  structure:
    cancel: every term (P, s) also appears as (-P, s) - every bucket sums to O: every cut bucket has L = -F or an infinite piece,
            every run ends in a cancellation (an odd n keeps one unpaired term);
    runs:   runs of 2 - 5 copies of one term (P, s) - the second addition of each run is P + P;
    rows:   all bases G, scalars 1, 2, ..., 2^(c-1) over and over - one entry per bucket of the lowest window, every bucket the
            same point: every row of the bucket reduction starts with P + P (c None: the pool is used);
    signs:  bases +-G with random signs, scalars from the pool - cancel-then-reopen at every level."""
    rng = random.Random(seed)
    draw = lambda: pool[rng.randrange(len(pool))]
    if structure == "cancel":
        half = [(rng.choice((1, 2, 3, 0)), draw()) for _ in range(n // 2)]
        terms = half + [(-k, s) for k, s in half]
        if n % 2:
            terms.append((rng.choice((1, -2, 3)), draw()))
        order = list(range(n))
        rng.shuffle(order)                          # the pair of a term lands anywhere in the bucket: no order is assumed
        terms = [terms[i] for i in order]
    elif structure == "runs":
        terms = []
        while len(terms) < n:
            k, s = rng.choice((1, -1, 2, -2, 3, -3, 0)), draw()
            terms += [(k, s)] * rng.randrange(2, 6)
        terms = terms[:n]
    elif structure == "rows":
        if c is None:
            terms = [(1, draw()) for _ in range(n)]
        else:
            terms = [(1, (i % (1 << (c - 1))) + 1) for i in range(n)]
    elif structure == "signs":
        terms = [(rng.choice((1, -1)), draw()) for _ in range(n)]
    else:
        raise ValueError(structure)
    ks = [k for k, _ in terms]
    scal = [s for _, s in terms]
    return ks, scal
