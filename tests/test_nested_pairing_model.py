"""The nested (BLS12-377) pairing kernels' per-lane bodies (zecale_amd/csrc/pairing_bls.cuh) compiled for the HOST by g++ and checked
against Python big integers and the host route; the host route itself (route 0 of zkhip_internal_nested_pairing_product) against
pyref; the statements the GPU tests verify; and what zkhip_nested_verifier_new does before it touches a device.  CPU only."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import nested_verify_fixtures as N

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")
OPS = ["mul", "sqr", "mul_line"]


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libnested_pairing_host_shim.so")
    src = os.path.join(HERE, "nested_pairing_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("pairing_bls.cuh", "fp29.cuh", "fp_inv.cuh", "bw6_params.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.fq12_op.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.nested_product_lanes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.nested_acc.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.nested_on_curve.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("op", OPS)
def test_fq12_lane_bodies_against_big_integers(shim, op):
    """Coefficient k = 0 .. 11 of a b, a^2 and a (l0 + l1 w + l3 w^3 + l7 w^7 + l9 w^9) in Fq[w]/(w^12 + 5) from the lane bodies, on
    every fixture case: random elements, zero, one, every coefficient at q - 1, a sparse line, line x line."""
    for a, b in N.fq12_cases():
        x, y = np.ascontiguousarray(N.fq12_limbs(a)), np.ascontiguousarray(N.fq12_limbs(b))
        out = np.zeros((12, 6), dtype=np.uint64)
        shim.fq12_op(OPS.index(op), x.ctypes.data, y.ctypes.data, out.ctypes.data)
        assert N.fq12_ints(out) == N.fq12_expected(op, a, b), (op, a, b)


def _lanes_product(shim, pairs):
    """the kernels' schedule (line chains, Miller loop, final exponentiation), lane by lane on the CPU"""
    g1, g2 = N.pair_limbs(pairs)
    g1, g2, frob = np.ascontiguousarray(g1[0]), np.ascontiguousarray(g2[0]), np.ascontiguousarray(N.frob_limbs())
    out = np.zeros((12, 6), dtype=np.uint64)
    assert shim.nested_product_lanes(g1.ctypes.data, g2.ctypes.data, len(pairs), frob.ctypes.data, out.ctypes.data) == 0
    return out


def _host_product(pairs):
    from zecale_amd import zkhip
    g1, g2 = N.pair_limbs(pairs)
    return zkhip.nested_pairing_product("host", g1, g2)[0]


def test_lane_schedule_equals_host_route(shim):
    """Line preparation, Miller loop and final exponentiation as the kernels schedule them, run lane after lane on the CPU: the
    reduced value equals route 0's limb for limb for one pair of generators, the four pairs of a valid statement (value one) and a
    two-pair product."""
    vk, proofs = N.golden_statement(3)
    four = N.verification_pairs(vk, *proofs[0])
    gens = [(R.BLS_G1_GEN, R.BLS_G2_GEN)]
    for pairs in (gens, four, four[:2]):
        got = _lanes_product(shim, pairs)
        assert (got == _host_product(pairs)).all()
    assert N.fq12_ints(_lanes_product(shim, four)) == N.EXT.one()
    assert N.fq12_ints(_lanes_product(shim, gens)) != N.EXT.one()


def test_host_route_is_bilinear():
    """e(u P, v Q) = e(P, Q)^(u v mod r) under Python big integers (ExtField.pow on the returned limbs)."""
    base = N.fq12_ints(_host_product([(R.BLS_G1_GEN, R.BLS_G2_GEN)]))
    assert base != N.EXT.one() and N.EXT.pow(base, R.BLS_R) == N.EXT.one()
    rng = random.Random(5)
    for u, v in [(1, 1), (2, 3), (R.BLS_R - 1, 5), (rng.randrange(1, R.BLS_R), rng.randrange(1, R.BLS_R))]:
        got = N.fq12_ints(_host_product([(N.g1mul(u), N.g2mul(v))]))
        assert got == N.EXT.pow(base, u * v % R.BLS_R), (u, v)


def _bumped(xs, i=0):
    bad = list(xs)
    bad[i] = (bad[i] + 1) % R.BLS_R
    return bad


def test_host_route_is_one_exactly_when_pyref_says_so():
    """Route 0 on the four pairs of a verification: the fixture statements, the reference's extproof1..6.json under vk.json, and each
    of them with an input bumped."""
    cases = []
    vk, proofs = N.dummy_app()
    for pr, xs in proofs:
        cases += [(vk, pr, xs), (vk, pr, _bumped(xs))]
    vk3, proofs3 = N.golden_statement(3)
    cases += [(vk3, proofs3[0][0], proofs3[0][1]), (vk3, proofs3[0][0], _bumped(proofs3[0][1], 2))]
    vk0, proofs0 = N.statements(0)
    cases += [(vk0, proofs0[0][0], []), (vk0, dict(proofs0[0][0], c=proofs0[0][0]["a"]), [])]
    verdicts = []
    for vk, pr, xs in cases:
        pairs = N.verification_pairs(vk, pr, xs)
        one = N.fq12_ints(_host_product(pairs)) == N.EXT.one()
        assert one == R.bls12_377_pairing_product_is_one(pairs)
        verdicts.append(one)
    assert verdicts == [True, False] * (len(cases) // 2)


def _acc_lanes(shim, vk, xs):
    abc0 = np.array(N.g1_limbs(vk["ABC"][0]), dtype=np.uint64)
    chain = np.array([N.g1_limbs(P) for B in vk["ABC"][1:] for P in N.doubling_chain(B)], dtype=np.uint64).reshape(-1)
    inp = np.ascontiguousarray(N.input_limbs(xs))
    out = np.zeros(12, dtype=np.uint64)
    same_x = shim.nested_acc(abc0.ctypes.data, chain.ctypes.data if len(xs) else None, inp.ctypes.data if len(xs) else None, len(xs), out.ctypes.data)
    return same_x, (N.fint(out[:6]), N.fint(out[6:]))


def test_accumulator_body_and_the_degenerate_statement(shim):
    """The accumulator's lane body gives ABC_0 + sum x_i ABC_i for ordinary statements and never reports a same-x step for them; the
    degenerate statement is in fact degenerate (at bit 2 the accumulator equals the chain point), is a valid proof by the group law,
    and the body reports the same-x branch for it."""
    for k in (0, 1, 3):
        vk, proofs = N.statements(k) if k != 1 else N.dummy_app()
        for pr, xs in proofs[:3]:
            same_x, acc = _acc_lanes(shim, vk, xs)
            assert same_x == 0 and acc == N.accumulator(vk, xs)
    vk, pr, xs = N.degenerate_statement()
    assert xs == [4] and N.doubling_chain(vk["ABC"][1], 3)[2] == vk["ABC"][0]
    assert R.bls12_377_groth16_verify(vk, pr, xs)
    assert _acc_lanes(shim, vk, xs)[0] == 1
    assert _acc_lanes(shim, vk, [12])[0] == 1                                 # bits 2 and 3: the step at bit 2 again
    assert _acc_lanes(shim, vk, [8])[0] == 1                                  # bit 2 CLEAR: the host forms acc + 4 ABC_1 there all the same
    for x in (3, 5, 6):                                                       # bit 0 or 1 moves the accumulator off the chain first
        same_x, acc = _acc_lanes(shim, vk, [x])
        assert same_x == 0 and acc == N.accumulator(vk, [x])


def test_accumulator_body_flags_the_negated_chain_point_at_a_clear_bit(shim):
    """ABC_0 = -4 ABC_1 and x = 8: a valid statement by the group law, but at the CLEAR bit 2 the host's accumulator is the negative of
    the chain point, its slope's product check fails and its verdict is 0.  The lane body reports the same-x step (so the proof goes to
    the host), as it does at the set bit of x = 4, and for no ordinary input of that key."""
    from zecale_amd import zkhip
    vk, pr, xs = N.degenerate_statement(8, negated=True)
    assert xs == [8] and N.g1neg(N.doubling_chain(vk["ABC"][1], 3)[2]) == vk["ABC"][0]
    assert R.bls12_377_groth16_verify(vk, pr, xs)
    assert not zkhip.bls12_377_groth16_verify(N.vk_limbs(vk), N.input_limbs(xs), N.proof_limbs(pr))
    assert _acc_lanes(shim, vk, [8])[0] == 1
    assert _acc_lanes(shim, vk, [4])[0] == 1
    for x in (3, 5, 6):
        same_x, acc = _acc_lanes(shim, vk, [x])
        assert same_x == 0 and acc == N.accumulator(vk, [x])
    # the same point at a clear bit: the host happens to accept (0 / 0 passes its product check)
    vk, pr, xs = N.degenerate_statement(8)
    assert zkhip.bls12_377_groth16_verify(N.vk_limbs(vk), N.input_limbs(xs), N.proof_limbs(pr))


def test_curve_checks_of_the_lane_bodies(shim):
    vk, proofs = N.dummy_app()
    fifth_neg = np.array(N.fl(-pow(5, -1, N.Q)), dtype=np.uint64)
    for pr, _ in proofs[:2]:
        for g2, limbs in ((0, N.g1_limbs(pr["a"])), (1, N.g2_limbs(pr["b"])), (0, N.g1_limbs(pr["c"]))):
            p = np.array(limbs, dtype=np.uint64)
            assert shim.nested_on_curve(p.ctypes.data, g2, fifth_neg.ctypes.data) == 1
            for at in range(0, p.size, 6):
                bad = p.copy()
                bad[at:at + 6] = N.fl(N.fint(p[at:at + 6]) + 1)
                assert shim.nested_on_curve(bad.ctypes.data, g2, fifth_neg.ctypes.data) == 0
            zero = np.zeros_like(p)
            assert shim.nested_on_curve(zero.ctypes.data, g2, fifth_neg.ctypes.data) == 0


def test_handle_refuses_bad_keys_on_the_host_and_needs_a_device():
    """zkhip_nested_verifier_new checks the key before it touches a device: an off-curve element and ABC_1 = (-1, 0) (on the curve, of
    order two: its doubling chain is degenerate) are ZKHIP_ERR_ARG with the element named - with or without a GPU.  A good key without
    a device is ZKHIP_ERR_NO_DEVICE, not a crash."""
    import torch
    from zecale_amd import zkhip
    lib = zkhip.load()
    vk, _ = N.dummy_app()
    good = N.vk_limbs(vk)
    new = lambda limbs, k: lib.zkhip_nested_verifier_new(np.ascontiguousarray(limbs).ctypes.data_as(zkhip.c_u64p_t), k, ctypes.byref(handle))
    handle = ctypes.c_void_p()
    off = good.copy(); off[66:72] = N.fl(N.fint(good[66:72]) + 1)              # ABC_0's y
    assert new(off, 1) == -1 and b"ABC[0]" in lib.zkhip_last_error() and not handle.value
    off = good.copy(); off[12:18] = N.fl(N.fint(good[12:18]) + 1)              # beta's x.c0
    assert new(off, 1) == -1 and b"beta" in lib.zkhip_last_error()
    two = dict(vk, ABC=[vk["ABC"][0], (N.Q - 1, 0)])
    assert R.on_curve(two["ABC"][1], R.BLS_G1_B, N.Q)
    assert new(N.vk_limbs(two), 1) == -1 and b"ABC[1]" in lib.zkhip_last_error() and not handle.value
    assert new(good, 17) == -1
    if torch.cuda.is_available():
        return  # the rest is meaningful only without a GPU
    assert new(good, 1) == -2, "zkhip_nested_verifier_new must fail with ZKHIP_ERR_NO_DEVICE when there is no GPU"
    assert not handle.value
    with pytest.raises(zkhip.ZkhipError):
        zkhip.NestedVerifier(good, 1)
    g1, g2 = N.pair_limbs([(R.BLS_G1_GEN, R.BLS_G2_GEN)])
    with pytest.raises(zkhip.ZkhipError):
        zkhip.nested_pairing_product("gpu", g1, g2)
    bad = g1.copy(); bad[0, 0, :6] = N.fl(5)
    for route in ("host", "gpu"):
        with pytest.raises(zkhip.ZkhipError) as e:
            zkhip.nested_pairing_product(route, bad, g2)
        assert e.value.code == -1


def test_lane_bodies_stand_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: every coefficient at q - 1 through the Fq12 bodies and the final
    exponentiation's program) built with the address and undefined-behaviour sanitizers and run on the CPU."""
    exe = tmp_path / "nested_shim_sanitized"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DNESTED_SHIM_MAIN",
                           "-o", str(exe), os.path.join(HERE, "nested_pairing_host_shim.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert len(out.stdout.strip()) == 16
