"""The combined batches' new per-lane bodies (zecale_amd/csrc/pairing.cuh: rho_scale, the strip product, the strip sum) compiled for the
HOST by g++ and run lane after lane in the kernels' schedule, and the host route of the combined check (pairing_host.hpp), against
Python big integers.  CPU only."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import combine_fixtures as C
from tests import verify_fixtures as V
from tests.helpers import aff_limbs, aff_point

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")
M128 = (1 << 128) - 1


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libpairing_combine_host_shim.so")
    src = os.path.join(HERE, "pairing_combine_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("pairing.cuh", "pairing_host.hpp", "host_field.hpp", "ec.cuh", "fp29.cuh", "fp_inv.cuh", "bw6_params.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.rho_scale_lane.argtypes = [vp, vp, vp]
    lib.gt_product_level.argtypes = [vp, sz, vp]
    lib.g1_sum_level.argtypes = [vp, sz, vp]
    lib.verify_all_value_host.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp, ctypes.c_uint, vp]
    lib.draw_scalars.argtypes = [vp, sz]
    lib.batch_chunk.argtypes, lib.batch_chunk.restype = [sz], sz
    lib.tree_levels.argtypes = [sz, vp, vp]
    return lib


def rho_words(rhos):
    return np.array([[r & (2 ** 64 - 1), r >> 64] for r in rhos], dtype=np.uint64).reshape(-1, 2)


def test_strip_constant(shim):
    from zecale_amd import zkhip
    assert shim.pairing_strip() == zkhip.VERIFIER_STRIP


def test_chunk_of_the_per_proof_route(shim):
    """VERIFIER_CHUNK proofs while the chunk's terms (proofs x inputs) stay within 2^21, which is up to 128 inputs per proof; beyond
    that floor(2^21 / n_inputs), and never below one proof.  The right-hand side restates the rule the driver had inline."""
    from zecale_amd import zkhip
    chunk, terms = zkhip.VERIFIER_CHUNK, 1 << 21
    assert chunk == 16384 and chunk * 128 == terms
    for n in (0, 1, 127, 128, 129, 1000, terms, terms + 1):
        want = chunk if n == 0 or chunk * n <= terms else max(terms // n, 1)
        assert shim.batch_chunk(n) == want, n
    assert [shim.batch_chunk(n) for n in (0, 1, 127, 128)] == [16384] * 4
    assert [shim.batch_chunk(n) for n in (129, 1000, terms, terms + 1)] == [terms // 129, 2097, 1, 1]


def test_levels_of_a_reduction_tree(shim):
    """For every n up to one past three full levels, and for a whole chunk: level k reads what level k - 1 wrote and writes
    ceil(n_k / STRIP) values, the levels before the last are left with more than one strip and the last with exactly one, and every
    level's output fits the buffer it goes to - the first, third, ... level writes the second buffer of ceil(n / STRIP) values, the
    second, fourth, ... writes back into the first of n."""
    from zecale_amd import zkhip
    strip = shim.pairing_strip()
    reads, writes = np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    for n in list(range(1, strip ** 3 + 2)) + [zkhip.VERIFIER_CHUNK]:
        levels = shim.tree_levels(n, reads.ctypes.data, writes.ctypes.data)
        r, w = [int(x) for x in reads[:levels]], [int(x) for x in writes[:levels]]
        assert levels >= 1 and r[0] == n and r[1:] == w[:-1], n
        assert w == [-(-x // strip) for x in r], n
        assert w[-1] == 1 and all(x > 1 for x in w[:-1]), n
        second = -(-n // strip)
        assert all(x <= (second if k % 2 == 0 else n) for k, x in enumerate(w)), n
    assert shim.tree_levels(zkhip.VERIFIER_CHUNK, reads.ctypes.data, writes.ctypes.data) == 5
    assert [shim.tree_levels(n, reads.ctypes.data, writes.ctypes.data) for n in (1, strip, strip + 1, strip ** 2, strip ** 2 + 1, strip ** 3 + 1)] == [1, 1, 2, 2, 3, 4]


def test_rho_scale_lane_against_ec_mul(shim):
    """rho P from the lane body for rho in {1, 2, 2^64, 2^128 - 1, random} and P finite, all-zero (stays infinity), and a point of
    G2's curve: the body never uses the curve's b, it serves G1 because its caller hands it G1 points."""
    rng = random.Random(11)
    points = [V.g1mul(rng.randrange(1, R.R_MOD)), R.G1_GEN, None, V.g2mul(rng.randrange(1, R.R_MOD))]
    for P in points:
        for rho in (1, 2, 1 << 64, M128, rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 128)):
            p, w, out = np.ascontiguousarray(aff_limbs(P)), rho_words([rho]), np.zeros(24, dtype=np.uint64)
            shim.rho_scale_lane(p.ctypes.data, w.ctypes.data, out.ctypes.data)
            assert aff_point(out) == (None if P is None else R.ec_mul(rho, P)), (P, rho)


def _product_level(shim, vals):
    n, strip = len(vals), shim.pairing_strip()
    x = np.ascontiguousarray(np.array([V.fq6_limbs(v) for v in vals]))
    out = np.zeros((-(-n // strip), 6, 12), dtype=np.uint64)
    shim.gt_product_level(x.ctypes.data, n, out.ctypes.data)
    return [V.fq6_ints(o) for o in out]


def test_strip_product_against_ext_mul(shim):
    """One launch of the product tree on strips of length 1, 2, the strip constant, and with a last strip of 1 and of strip - 1
    values: each strip's product equals EXT.mul over exactly its own values (the operand select multiplies by one past the end).
    Operands include every coefficient at q - 1 (the lazy bounds' worst case)."""
    strip = shim.pairing_strip()
    rng = random.Random(3)
    pool = [[rng.randrange(R.Q_MOD) for _ in range(6)] for _ in range(2 * strip)] + [[R.Q_MOD - 1] * 6, V.EXT.one()]
    for n in (1, 2, strip - 1, strip, strip + 1, 2 * strip - 1, 2 * strip):
        vals = [pool[(3 * i + n) % len(pool)] for i in range(n)]
        want = []
        for lo in range(0, n, strip):
            f = V.EXT.one()
            for v in vals[lo:lo + strip]:
                f = V.EXT.mul(f, v)
            want.append(f)
        assert _product_level(shim, vals) == want, n


def _sum_level(shim, pts):
    n, strip = len(pts), shim.pairing_strip()
    x = np.ascontiguousarray(np.array([aff_limbs(P) for P in pts]))
    out = np.zeros((-(-n // strip), 24), dtype=np.uint64)
    shim.g1_sum_level(x.ctypes.data, n, out.ctypes.data)
    return [aff_point(o) for o in out]


def test_strip_sum_against_affine_addition(shim):
    """One launch of the sum tree on strips of length 1, 2 and the strip constant, with the group law's edges inside a strip: two equal
    summands (doubling), P and -P (infinity), infinity as first and as last summand, a strip of infinities."""
    strip = shim.pairing_strip()
    rng = random.Random(4)
    P = [V.g1mul(rng.randrange(1, R.R_MOD)) for _ in range(strip)]
    cases = [[P[0]], [None], [P[0], P[1]], [P[0], P[0]], [P[0], R.ec_neg(P[0])], [None, P[1]], [P[1], None],
             P, [None] + P[1:], P[:-1] + [None], [P[0], P[0]] + P[2:], [P[0], R.ec_neg(P[0])] + P[2:], [P[0], R.ec_neg(P[0]), None, None],
             [P[0], P[1], R.ec_neg(R.ec_add(P[0], P[1])), P[2]], [None] * strip,
             P + [P[0]], P + [None], P + P[:2] + [R.ec_neg(P[1])]]
    for pts in cases:
        want = []
        for lo in range(0, len(pts), strip):
            s = None
            for Q in pts[lo:lo + strip]:
                s = R.ec_add(s, Q)
            want.append(s)
        assert _sum_level(shim, pts) == want, pts


def _host_value(shim, n_inputs, inputs, proofs, rhos, threads=3):
    vkl = V.vk_limbs(V.statements(n_inputs)[0])
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
    al, be, de, abc, inp, pr, w = c(vkl["alpha"]), c(vkl["beta"]), c(vkl["delta"]), c(vkl["ABC"]), c(inputs), c(proofs), rho_words(rhos)
    out = np.zeros((6, 12), dtype=np.uint64)
    shim.verify_all_value_host(al.ctypes.data, be.ctypes.data, de.ctypes.data, abc.ctypes.data, n_inputs, inp.ctypes.data, pr.ctypes.data,
                               len(pr), w.ctypes.data, threads, out.ctypes.data)
    return V.fq6_ints(out)


@pytest.mark.parametrize("n_inputs", [0, 4])
def test_host_route_value_is_the_product_of_the_proofs_values(shim, n_inputs):
    """The host route's reduced value equals prod_k gt_k^(e_k): gt_k is gt_value of the four pairs of proof k in Python, e_k the sum of
    the scalars at the positions that hold proof k.  The batch repeats statements (the edge inputs 0 and r - 1 are statement 0's),
    holds a proof tampered in C and - with inputs - one with a bumped input, so that some gt_k != 1 and the input sums matter."""
    vk, stm = V.statements(n_inputs)
    kinds = {"valid0": (stm[0][0], stm[0][1]), "valid3": (stm[3][0], stm[3][1]), "c+D": (C.tamper(stm[1][0], 1), stm[1][1])}
    if n_inputs:
        bumped = list(stm[2][1]); bumped[n_inputs - 1] = (bumped[n_inputs - 1] + 7) % R.R_MOD
        kinds["input+7"] = (stm[2][0], bumped)
    order = ["valid0", "c+D", "valid3", "valid0", "c+D"] + (["input+7", "valid3", "input+7"] if n_inputs else ["valid3"])
    rhos = [1, M128, 1 << 64, 2, 0x1234567890ABCDEF0FEDCBA987654321] + C.scalars(len(order) - 5, seed=9)
    gt = {name: V.gt_value(C.four_pairs(vk, proof, xs)) for name, (proof, xs) in kinds.items()}
    assert gt["valid0"] == gt["valid3"] == V.EXT.one() and gt["c+D"] == list(C.g(n_inputs)) != V.EXT.one()
    assert n_inputs == 0 or gt["input+7"] != V.EXT.one()
    want = V.EXT.one()
    for name, rho in zip(order, rhos):
        want = V.EXT.mul(want, V.EXT.pow(gt[name], rho))
    inputs = np.array([V.input_limbs(kinds[name][1]) for name in order]).reshape(len(order), n_inputs, 6)
    proofs = np.array([V.proof_limbs(kinds[name][0]) for name in order])
    assert _host_value(shim, n_inputs, inputs, proofs, rhos) == want != V.EXT.one()
    assert _host_value(shim, n_inputs, inputs, proofs, rhos, threads=1) == want
    # the all-valid sub-batch has value one, the fixtures' closed form agrees, and an empty batch is one
    keep = [i for i, name in enumerate(order) if name.startswith("valid")]
    assert _host_value(shim, n_inputs, inputs[keep], proofs[keep], [rhos[i] for i in keep]) == V.EXT.one()
    inp, prf, ks = C.batch(n_inputs, 9, {0: 1, 4: -2, 8: 3})
    assert _host_value(shim, n_inputs, inp, prf, C.scalars(9)) == C.expected_value(n_inputs, ks, C.scalars(9)) != V.EXT.one()
    assert _host_value(shim, n_inputs, inp[:0], prf[:0], []) == V.EXT.one()


def test_groth16_verify_all_on_the_host():
    """zkhip_groth16_verify_all through the library, no device: valid batches pass with supplied and with drawn scalars, a tampered proof
    at any position fails, C + D and C - D cancel under equal scalars only, a point off its curve fails the batch, a zero scalar is
    ZKHIP_ERR_ARG, the empty batch passes."""
    from zecale_amd import zkhip
    vkl = V.vk_limbs(V.statements(4)[0])
    inp, prf, _ = C.batch(4, 5)
    assert zkhip.groth16_verify_all(vkl, inp, prf, C.scalars(5))
    assert zkhip.groth16_verify_all(vkl, inp, prf)
    assert zkhip.groth16_verify_all(vkl, inp[:0], prf[:0])
    for pos in (0, 2, 4):
        bad_in, bad_pr, _ = C.batch(4, 5, {pos: 1})
        assert not zkhip.groth16_verify_all(vkl, bad_in, bad_pr, C.scalars(5))
        assert not zkhip.groth16_verify_all(vkl, bad_in, bad_pr)
    two_in, two_pr, _ = C.batch(4, 3, {0: 1, 2: -1})
    assert zkhip.groth16_verify_all(vkl, two_in, two_pr, [77, 5, 77])
    assert not zkhip.groth16_verify_all(vkl, two_in, two_pr, [77, 5, 78])
    assert not zkhip.groth16_verify_all(vkl, two_in, two_pr)
    off = prf.copy(); off[3, 48:72] = aff_limbs((R.G1_GEN[0], (R.G1_GEN[1] + 1) % R.Q_MOD))
    assert not zkhip.groth16_verify_all(vkl, inp, off, C.scalars(5))
    with pytest.raises(zkhip.ZkhipError) as e:
        zkhip.groth16_verify_all(vkl, inp, prf, [3, 0, 5, 6, 7])
    assert e.value.code == -1


def test_drawn_scalars_are_nonzero_and_differ(shim):
    w = np.zeros((64, 2), dtype=np.uint64)
    assert shim.draw_scalars(w.ctypes.data, 64) == 1
    vals = {int(a) | int(b) << 64 for a, b in w}
    assert len(vals) == 64 and 0 not in vals


def test_combine_bodies_stand_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: rho_scale with the all-ones scalar, one launch of both trees at every length up
    to one past two strips) built with the address and undefined-behaviour sanitizers and run on the CPU: a read past the values of a
    short last strip, or a shift past a word's width in the scalar's shifting, would stop it."""
    exe = tmp_path / "pairing_combine_shim_sanitized"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DPAIRING_COMBINE_SHIM_MAIN", "-o", str(exe), os.path.join(HERE, "pairing_combine_host_shim.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert len(out.stdout.strip()) == 16
