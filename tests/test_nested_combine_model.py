"""The nested verifier's combined batches on the CPU: the new per-lane bodies (zecale_amd/csrc/pairing_bls.cuh: nested_rho_scale, the
strip product, the strip sum with the complete XYZZ addition) compiled for the HOST by g++ and run lane after lane in the kernels'
schedule, the integer rules of the reduction trees, and the host route of the combined check (nested_combine_host.hpp,
zkhip_bls12_377_groth16_verify_all), against Python big integers.  CPU only, no device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import nested_combine_fixtures as C
from tests import nested_verify_fixtures as N

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")
M128 = (1 << 128) - 1
ONE = N.EXT.one()
ORDER_TWO = (N.Q - 1, 0)                 # (-1, 0) on y^2 = x^3 + 1


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libnested_combine_host_shim.so")
    src = os.path.join(HERE, "nested_combine_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("pairing_bls.cuh", "pairing.cuh", "nested_combine_host.hpp", "nested_key.hpp", "nested_point_check_host.hpp",
                                            "combine_scalars.hpp", "host_field.hpp", "fp29.cuh", "fp_inv.cuh", "bw6_params.h")]
    hdrs += [os.path.join(CSRC, "circuit", h) for h in os.listdir(os.path.join(CSRC, "circuit"))]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.rho_scale_lane.argtypes = [vp, vp, vp]
    lib.gt_product_level.argtypes = [vp, sz, vp, vp]
    lib.g1_sum_level.argtypes = [vp, sz, vp, vp]
    lib.verify_all_value_host.argtypes = [vp, sz, vp, vp, sz, vp, ctypes.c_uint, vp, vp]
    lib.wide_sum.argtypes = [vp, vp, sz, vp]
    lib.draw_scalars.argtypes = [vp, sz]
    lib.tree_levels.argtypes = [sz, vp, vp]
    return lib


def g1_or_zero(P):
    return np.array(N.g1_limbs(P) if P is not None else [0] * 12, dtype=np.uint64)


def point_or_none(limbs):
    limbs = np.asarray(limbs).reshape(12)
    return None if not limbs.any() else (N.fint(limbs[:6]), N.fint(limbs[6:]))


# ---------------------------------------------------------------- the integer rules
def test_strip_constant(shim):
    from zecale_amd import zkhip
    assert shim.nested_strip() == zkhip.NESTED_VERIFIER_STRIP == 8


def test_levels_of_a_reduction_tree(shim):
    """For every n up to one past three full levels - both sides of a strip, of strip^2 and of strip^3 - and for a whole chunk: level k
    reads what level k - 1 wrote and writes ceil(n_k / STRIP) values, the levels before the last are left with more than one strip and
    the last with exactly one, and every level's output fits the buffer it goes to: the first, third, ... level writes the second
    buffer of ceil(n / STRIP) values, the second, fourth, ... writes back into the first of n."""
    from zecale_amd import zkhip
    strip = shim.nested_strip()
    reads, writes = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    for n in list(range(1, strip ** 3 + 2)) + [zkhip.NESTED_VERIFIER_CHUNK]:
        levels = shim.tree_levels(n, reads.ctypes.data, writes.ctypes.data)
        r, w = [int(x) for x in reads[:levels]], [int(x) for x in writes[:levels]]
        assert levels >= 1 and r[0] == n and r[1:] == w[:-1], n
        assert w == [-(-x // strip) for x in r], n
        assert w[-1] == 1 and all(x > 1 for x in w[:-1]), n
        second = -(-n // strip)
        assert all(x <= (second if k % 2 == 0 else n) for k, x in enumerate(w)), n
    assert shim.tree_levels(zkhip.NESTED_VERIFIER_CHUNK, reads.ctypes.data, writes.ctypes.data) == 5
    assert [shim.tree_levels(n, reads.ctypes.data, writes.ctypes.data)
            for n in (1, strip - 1, strip, strip + 1, strip ** 2 - 1, strip ** 2, strip ** 2 + 1, strip ** 3 + 1)] == [1, 1, 1, 2, 2, 2, 3, 4]


def test_sums_in_the_scalar_field(shim):
    """sum rho_i x_i mod r from the host's wide accumulator against Python, with every factor at its top: rho = 2^128 - 1, x = 2^253 - 1
    (an input's low 253 bits may exceed r), many terms, and the empty sum."""
    rng = random.Random(8)
    for count in (0, 1, 2, 300):
        rhos = [M128] * min(count, 2) + [rng.randrange(1, 1 << 128) for _ in range(max(count - 2, 0))]
        xs = [(1 << 253) - 1] * min(count, 2) + [rng.randrange(1 << 253) for _ in range(max(count - 2, 0))]
        x = np.array([[(v >> (64 * t)) & (2 ** 64 - 1) for t in range(4)] for v in xs], dtype=np.uint64).reshape(-1, 4)
        w, out = C.rho_words(rhos), np.zeros(4, dtype=np.uint64)
        shim.wide_sum(w.ctypes.data, x.ctypes.data, count, out.ctypes.data)
        assert sum(int(v) << (64 * t) for t, v in enumerate(out)) == sum(a * b for a, b in zip(rhos, xs)) % R.BLS_R, count


# ---------------------------------------------------------------- the lane bodies
def test_rho_scale_lane_against_ec_mul(shim):
    """rho P from the lane body for rho in {1, 2, 2^64, 2^128 - 1, random} and P the generator, a random point of G1 and (2, 3) (on the
    curve, outside the group of order r: the formulas never use the order); and A = (-1, 0), of order 2: the point itself under an odd
    scalar, infinity (all zero) under an even one."""
    rng = random.Random(11)
    for P in (R.BLS_G1_GEN, N.g1mul(rng.randrange(1, R.BLS_R)), (2, 3)):
        for rho in (1, 2, 1 << 64, M128, rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 128)):
            p, w, out = g1_or_zero(P), C.rho_words([rho]), np.zeros(12, dtype=np.uint64)
            shim.rho_scale_lane(p.ctypes.data, w.ctypes.data, out.ctypes.data)
            assert point_or_none(out) == R.ec_mul(rho, P, N.Q), (P, rho)
    for rho, want in ((2, None), (M128 - 1, None), (1 << 64, None), (1, ORDER_TWO), (M128, ORDER_TWO), ((1 << 127) + 1, ORDER_TWO)):
        p, w, out = g1_or_zero(ORDER_TWO), C.rho_words([rho]), np.zeros(12, dtype=np.uint64)
        shim.rho_scale_lane(p.ctypes.data, w.ctypes.data, out.ctypes.data)
        assert point_or_none(out) == want, rho


def _product_level(shim, vals, skip=None):
    n, strip = len(vals), shim.nested_strip()
    x = np.ascontiguousarray(np.array([N.fq12_limbs(v) for v in vals]))
    out = np.zeros((-(-n // strip), 12, 6), dtype=np.uint64)
    sk = None if skip is None else np.array(skip, dtype=np.uint8)
    shim.gt_product_level(x.ctypes.data, n, None if sk is None else sk.ctypes.data, out.ctypes.data)
    return [N.fq12_ints(o) for o in out]


def test_strip_product_against_ext_mul(shim):
    """One launch of the product tree on strips of length 1, 2, the strip constant, and with a last strip of 1 and of strip - 1
    values: each strip's product equals EXT.mul over exactly its own values (the operand select multiplies by one past the end), and
    over its unflagged values when skip bytes are given.  Operands include every coefficient at q - 1 (the lazy bounds' worst case)."""
    strip = shim.nested_strip()
    rng = random.Random(3)
    pool = [[rng.randrange(N.Q) for _ in range(12)] for _ in range(2 * strip)] + [[N.Q - 1] * 12, ONE]
    for n in (1, 2, strip - 1, strip, strip + 1, 2 * strip - 1, 2 * strip):
        vals = [pool[(3 * i + n) % len(pool)] for i in range(n)]
        for skip in (None, [(i * 7 + n) % 3 == 0 for i in range(n)], [True] * n):
            want = []
            for lo in range(0, n, strip):
                f = ONE
                for i, v in enumerate(vals[lo:lo + strip]):
                    if skip is None or not skip[lo + i]:
                        f = N.EXT.mul(f, v)
                want.append(f)
            assert _product_level(shim, vals, skip) == want, (n, skip)
    top = [[N.Q - 1] * 12] * strip                       # a whole strip at the bounds' worst case
    f = ONE
    for v in top:
        f = N.EXT.mul(f, v)
    assert _product_level(shim, top) == [f]


def _sum_level(shim, pts, scaled=False):
    n, strip = len(pts), shim.nested_strip()
    x = np.ascontiguousarray(np.array([g1_or_zero(P) for P in pts]))
    out = np.zeros((-(-n // strip), 12), dtype=np.uint64)
    z = np.array(N.fl(0x1234567), dtype=np.uint64)
    shim.g1_sum_level(x.ctypes.data, n, z.ctypes.data if scaled else None, out.ctypes.data)
    return [point_or_none(o) for o in out]


def test_strip_sum_against_affine_addition(shim):
    """One launch of the sum tree on strips of length 1, 2 and the strip constant and on strips that run past the end, with the group
    law's edges inside a strip: two equal summands (doubling), P and -P (infinity), infinity as first, middle and last summand, a strip
    of infinities, the point of order two twice.  Each case runs with the summands as given (ZZ = ZZZ = 1) and with every summand in
    another representation of its own (x z^2, y z^3, z^2, z^3), as the partial sums of an earlier level are: equal points then differ
    in every coordinate."""
    strip = shim.nested_strip()
    rng = random.Random(4)
    P = [N.g1mul(rng.randrange(1, R.BLS_R)) for _ in range(strip)]
    neg = lambda X: N.g1neg(X)
    add = lambda A, B: R.ec_add(A, B, N.Q)
    cases = [[P[0]], [None], [P[0], P[1]], [P[0], P[0]], [P[0], neg(P[0])], [None, P[1]], [P[1], None],
             P, [None] + P[1:], P[:-1] + [None], P[:3] + [None] + P[4:], [P[0], P[0]] + P[2:], [P[0], neg(P[0])] + P[2:],
             [P[0], neg(P[0]), None, None], [P[0], P[1], neg(add(P[0], P[1])), P[2]], [P[0], P[1], add(P[0], P[1]), P[2]], [None] * strip,
             [ORDER_TWO, ORDER_TWO, P[0]], P + [P[0]], P + [None], P + P[:2] + [neg(P[1])], P + P[:strip - 1]]
    for pts in cases:
        want = []
        for lo in range(0, len(pts), strip):
            s = None
            for X in pts[lo:lo + strip]:
                s = add(s, X)
            want.append(s)
        assert _sum_level(shim, pts) == want, pts
        assert _sum_level(shim, pts, scaled=True) == want, pts


# ---------------------------------------------------------------- the host route
def _host_value(shim, vk, n_inputs, inputs, proofs, rhos, threads=3):
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    vkl, inp, pr, w = c(N.vk_limbs(vk)), c(inputs), c(proofs).reshape(-1, 48), C.rho_words(rhos)
    out, left = np.zeros((12, 6), dtype=np.uint64), np.zeros(max(len(pr), 1), dtype=np.uint8)
    assert shim.verify_all_value_host(vkl.ctypes.data, n_inputs, inp.ctypes.data, pr.ctypes.data, len(pr), w.ctypes.data, threads, left.ctypes.data,
                                      out.ctypes.data) == 0
    return N.fq12_ints(out), list(left[:len(pr)])


@pytest.mark.parametrize("n_inputs", [0, 1, 3])
def test_host_route_value_is_the_power_of_g(shim, n_inputs):
    """The host route's reduced value equals g^(sum k_i rho_i), g = e(D, -delta), for tamperings at the first, a middle and the last
    position and at several at once, on one and on three threads; an all-valid batch and the empty batch have value one; nothing is
    left out."""
    vk = C.source(n_inputs)[0]
    count = 7
    rhos = [1, M128, 1 << 64, 2, 0x1234567890ABCDEF0FEDCBA987654321] + C.scalars(count - 5, seed=9)
    for tampered in ({0: 1}, {3: 2}, {count - 1: -1}, {0: 1, 2: -2, 6: 3}):
        inp, prf, ks = C.batch(n_inputs, count, tampered)
        want = C.expected_value(n_inputs, ks, rhos)
        assert want != ONE
        for threads in (1, 3):
            assert _host_value(shim, vk, n_inputs, inp, prf, rhos, threads) == (want, [0] * count), (tampered, threads)
    inp, prf, _ = C.batch(n_inputs, count)
    assert _host_value(shim, vk, n_inputs, inp, prf, rhos) == (ONE, [0] * count)
    assert _host_value(shim, vk, n_inputs, inp, prf, rhos, threads=1) == (ONE, [0] * count)
    assert _host_value(shim, vk, n_inputs, inp[:0], prf[:0], []) == (ONE, [])


def test_host_route_reads_the_low_253_bits_of_an_input(shim):
    """x_ij is the low 253 bits of the input's canonical value, reduced mod r: a wrong input gives a value other than one; x + r, where
    it stays below 2^253, is the same statement (the per-proof host route accepts it too) and the value stays one."""
    from zecale_amd import zkhip
    vk, stm = N.statements(1)
    pr, xs = next((pr, xs) for pr, xs in stm if xs[0] + R.BLS_R < (1 << 253))
    vkl, prl = N.vk_limbs(vk), N.proof_limbs(pr)
    bumped = [(xs[0] + 1) % R.BLS_R]
    assert _host_value(shim, vk, 1, N.input_limbs(bumped), prl, [77])[0] != ONE
    assert _host_value(shim, vk, 1, N.input_limbs(xs), prl, [77])[0] == ONE
    wrapped = [xs[0] + R.BLS_R]
    assert zkhip.bls12_377_groth16_verify(vkl, N.input_limbs(wrapped), prl)
    assert _host_value(shim, vk, 1, N.input_limbs(wrapped), prl, [77])[0] == ONE


def test_host_route_leaves_out_what_is_off_its_curve(shim):
    """A, B or C off its curve (a coordinate + 1; all zero: the nested format has no infinity): left out of the value - which then runs
    over the other proofs alone - and marked."""
    vk = N.statements(3)[0]
    rhos = C.scalars(5, seed=2)
    inp, prf, ks = C.batch(3, 5, {1: 1})
    for at in (6, 12, 36):
        bad = prf.copy(); bad[3, at:at + 6] = N.fl(N.fint(prf[3, at:at + 6]) + 1)
        assert _host_value(shim, vk, 3, inp, bad, rhos) == (C.expected_value(3, ks, rhos), [0, 0, 0, 1, 0]), at
    for lo, hi in ((0, 12), (12, 36), (36, 48)):
        bad = prf.copy(); bad[4, lo:hi] = 0
        assert _host_value(shim, vk, 3, inp, bad, rhos) == (C.expected_value(3, ks, rhos), [0, 0, 0, 0, 1]), lo
    bad = prf.copy(); bad[1, 0:6] = N.fl(N.fint(prf[1, 0:6]) + 1)            # the tampered proof itself left out: the rest is valid
    assert _host_value(shim, vk, 3, inp, bad, rhos) == (ONE, [0, 1, 0, 0, 0])


def test_an_a_of_order_two(shim):
    """A = (-1, 0) in place of a valid proof's A.  The valid proof has e(A, B) rest = 1, rest the product of its other three pairs.
    Under an even scalar rho (-1, 0) = O and the pair contributes one: the value is rest^rho = e(A, B)^(-rho).  Under an odd one
    rho (-1, 0) = (-1, 0), a finite point that goes through the Miller loop - and its pairing, of order dividing gcd(2, r), is one
    as well: the same value by the other path."""
    from zecale_amd import zkhip
    vk, stm = N.statements(1)
    pr, xs = stm[0]
    inp = N.input_limbs(xs).reshape(1, 1, 6)
    bad = N.proof_limbs(dict(pr, a=ORDER_TWO)).reshape(1, 48)
    good = N.proof_limbs(pr).reshape(1, 48)
    e_ab = N.fq12_ints(zkhip.nested_pairing_product("host", *N.pair_limbs([(pr["a"], pr["b"])]))[0])
    for rho in (6, 1 << 64):
        assert _host_value(shim, vk, 1, inp, bad, [rho]) == (N.EXT.pow(e_ab, (-rho) % R.BLS_R), [0])
        assert _host_value(shim, vk, 1, inp, good, [rho]) == (ONE, [0])
    assert _host_value(shim, vk, 1, inp, bad, [7]) == (N.EXT.pow(e_ab, (-7) % R.BLS_R), [0])


def test_groth16_verify_all_on_the_host(shim):
    """zkhip_bls12_377_groth16_verify_all through the library, no device: valid batches pass with supplied and with drawn scalars, a
    tampered proof at any position fails, C + D and C - D cancel under equal scalars only (caller-supplied scalars prove nothing), a
    point off its curve fails the batch, a zero scalar is ZKHIP_ERR_ARG, the empty batch passes."""
    from zecale_amd import zkhip
    vkl = N.vk_limbs(N.statements(3)[0])
    inp, prf, _ = C.batch(3, 5)
    assert zkhip.bls12_377_groth16_verify_all(vkl, inp, prf, C.scalars(5))
    assert zkhip.bls12_377_groth16_verify_all(vkl, inp, prf)
    assert zkhip.bls12_377_groth16_verify_all(vkl, inp[:0], prf[:0])
    for pos in (0, 2, 4):
        bad_in, bad_pr, _ = C.batch(3, 5, {pos: 1})
        assert not zkhip.bls12_377_groth16_verify_all(vkl, bad_in, bad_pr, C.scalars(5))
        assert not zkhip.bls12_377_groth16_verify_all(vkl, bad_in, bad_pr)
    two_in, two_pr, _ = C.batch(3, 3, {0: 1, 2: -1})
    assert zkhip.bls12_377_groth16_verify_all(vkl, two_in, two_pr, [77, 5, 77])
    assert not zkhip.bls12_377_groth16_verify_all(vkl, two_in, two_pr, [77, 5, 78])
    assert not zkhip.bls12_377_groth16_verify_all(vkl, two_in, two_pr)
    off = prf.copy(); off[3, 42:48] = N.fl(N.fint(prf[3, 42:48]) + 1)
    assert not zkhip.bls12_377_groth16_verify_all(vkl, inp, off, C.scalars(5))
    zero = prf.copy(); zero[0, :12] = 0
    assert not zkhip.bls12_377_groth16_verify_all(vkl, inp, zero, C.scalars(5))
    with pytest.raises(zkhip.ZkhipError) as e:
        zkhip.bls12_377_groth16_verify_all(vkl, inp, prf, [3, 0, 5, 6, 7])
    assert e.value.code == -1
    vk0 = N.vk_limbs(N.statements(0)[0])
    inp0, prf0, _ = C.batch(0, 3)
    assert zkhip.bls12_377_groth16_verify_all(vk0, inp0, prf0)
    bad_in, bad_pr, _ = C.batch(0, 3, {1: 1})
    assert not zkhip.bls12_377_groth16_verify_all(vk0, bad_in, bad_pr)


@pytest.mark.parametrize("x,negated", [(4, False), (8, True), (8, False)])
def test_the_combined_route_answers_the_group_law_on_degenerate_statements(shim, x, negated):
    """Statements, valid by the group law, on which the host's affine accumulator meets +-2^2 ABC_1: the per-proof host verifier
    rejects x = 4 and (8, negated) - the combined route has no accumulator chain, its value is one and it accepts, alone and among
    ordinary proofs of the same key."""
    from zecale_amd import zkhip
    vk, pr, xs = N.degenerate_statement(x, negated)
    vkl = N.vk_limbs(vk)
    assert zkhip.bls12_377_groth16_verify(vkl, N.input_limbs(xs), N.proof_limbs(pr)) == (x == 8 and not negated)
    items = [(pr, xs), N.degenerate_statement(3, negated)[1:], (pr, xs), N.degenerate_statement(5, negated)[1:]]
    inp = np.array([N.input_limbs(i) for _, i in items], dtype=np.uint64).reshape(4, 1, 6)
    prf = np.array([N.proof_limbs(p) for p, _ in items], dtype=np.uint64)
    rhos = C.scalars(4, seed=x)
    assert _host_value(shim, vk, 1, inp[:1], prf[:1], rhos[:1]) == (ONE, [0])
    assert _host_value(shim, vk, 1, inp, prf, rhos) == (ONE, [0] * 4)
    assert zkhip.bls12_377_groth16_verify_all(vkl, inp, prf, rhos) and zkhip.bls12_377_groth16_verify_all(vkl, inp, prf)
    wrong = N.input_limbs([6]).reshape(1, 1, 6)
    assert not zkhip.bls12_377_groth16_verify_all(vkl, np.concatenate([inp, wrong]), np.concatenate([prf, prf[1:2]]))


def test_no_point_of_the_twist_has_a_degenerate_line_schedule():
    """Why no test sends a B with a degenerate line schedule through the public route: a step of the schedule is degenerate when
    2 k Q = O (a doubling of T = k Q) or (k -+ 1) Q = O (an addition of Q to T = k Q) for a prefix k of u, so the order of Q - a divisor
    of #E'(Fq2) = r c2 - would have to divide a number below 2^65.  r is too large, and c2 is coprime to every one of them.  c2 is
    checked on a point: [c2] kills what [r] leaves of a twist point."""
    from math import gcd
    u = 0x8508c00000000001
    n = u ** 8 - 4 * u ** 7 + 5 * u ** 6 - 4 * u ** 4 + 6 * u ** 3 - 4 * u ** 2 - 4 * u + 13
    assert n % 9 == 0
    c2 = n // 9
    from tests import nested_point_check_fixtures as F
    cof = F.g2_cofactor_points()[1]
    assert cof is not None and F.g2_mul_raw(c2, cof) is None
    k, steps = 1, 0
    for i in range(62, -1, -1):
        assert gcd(c2, 2 * k) == 1, i
        k, steps = 2 * k, steps + 1
        if (u >> i) & 1:
            assert gcd(c2, k - 1) == 1 and gcd(c2, k + 1) == 1, i
            k, steps = k + 1, steps + 1
    assert k == u and steps == 69 and R.BLS_R > 1 << 66


def test_drawn_scalars_are_nonzero_and_differ(shim):
    w = np.zeros((64, 2), dtype=np.uint64)
    assert shim.draw_scalars(w.ctypes.data, 64) == 1
    vals = {int(a) | int(b) << 64 for a, b in w}
    assert len(vals) == 64 and 0 not in vals


def test_nested_combine_bodies_stand_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: nested_rho_scale with the all-ones scalar and on the point of order two, one
    launch of both trees at every length up to one past two strips with and without skip bytes, the wide sums at their top) built with
    the address and undefined-behaviour sanitizers and run on the CPU: a read past the values of a short last strip, or a shift past a
    word's width in the scalar's shifting, would stop it."""
    exe = tmp_path / "nested_combine_shim_sanitized"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DNESTED_COMBINE_SHIM_MAIN", "-o", str(exe), os.path.join(HERE, "nested_combine_host_shim.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert len(out.stdout.strip()) == 16
