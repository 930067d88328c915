"""The pairing kernels' per-lane bodies (zecale_amd/csrc/pairing.cuh) compiled for the HOST by g++ and checked against Python big
integers and the host pairing; the trapdoor statements the GPU tests verify, checked by pyref and the host verifier first; and the
batch verifier's refusal to run without a device.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import verify_fixtures as V
from tests.helpers import aff_limbs, fq_limbs

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libpairing_host_shim.so")
    src = os.path.join(HERE, "pairing_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("pairing.cuh", "fp29.cuh", "bw6_params.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.fq6_op.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.pairing_product_lanes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_void_p]
    return lib


@pytest.mark.parametrize("op", ["mul", "sqr", "mul_line"])
def test_lane_bodies_against_big_integers(shim, op):
    """Coefficient k = 0 .. 5 of a b, a^2 and a (l0 + l3 w^3 + l4 w^4) in Fq[w]/(w^6 + 4) from the lane bodies: random elements, zero,
    one, every coefficient at q - 1 (the lazy bounds' worst case through fp_from_abi) and a sparse line."""
    for a, b in V.fq6_cases():
        x, y = np.ascontiguousarray(V.fq6_limbs(a)), np.ascontiguousarray(V.fq6_limbs(b))
        out = np.zeros((6, 12), dtype=np.uint64)
        shim.fq6_op(["mul", "sqr", "mul_line"].index(op), x.ctypes.data, y.ctypes.data, out.ctypes.data)
        assert V.fq6_ints(out) == V.fq6_expected(op, a, b), (op, a, b)


def _lanes_product(shim, pairs):
    """the kernels' schedule, lane by lane on the CPU"""
    q = R.Q_MOD
    g1 = np.ascontiguousarray(np.array([aff_limbs(P) for P, _ in pairs]))
    g2 = np.ascontiguousarray(np.array([aff_limbs(Q) for _, Q in pairs]))
    quarter = np.ascontiguousarray(np.concatenate([fq_limbs(pow(4, -1, q)), fq_limbs(-pow(4, -1, q) % q)]))
    r_order = np.array(R.int_to_limbs(R.R_MOD, 6), dtype=np.uint64)
    e = np.array(R.int_to_limbs(V.FINAL_EXP, 66), dtype=np.uint64)
    out = np.zeros((6, 12), dtype=np.uint64)
    shim.pairing_product_lanes(g1.ctypes.data, g2.ctypes.data, len(pairs), quarter.ctypes.data, r_order.ctypes.data, e.ctypes.data,
                               V.FINAL_EXP.bit_length(), out.ctypes.data)
    return out


def test_lane_schedule_equals_host_pairing_and_pyref(shim):
    """The Miller loop and the final exponentiation as the kernels schedule them (point steps per pair, lines folded one by one,
    square-and-multiply), run lane after lane on the CPU: the reduced value equals the host route's limb for limb - and pyref's - for
    one pair of generators, a four-pair product of a valid statement (value one) and a product with a pair at infinity."""
    from zecale_amd import zkhip
    vk, proofs = V.statements(1)
    proof, xs = proofs[0]
    acc = vk["ABC"][0]
    for x, P in zip(xs, vk["ABC"][1:]):
        acc = R.ec_add(acc, R.ec_mul(x, P))
    four = [(proof["a"], proof["b"]), (acc, R.ec_neg(R.G2_GEN)), (vk["alpha"], R.ec_neg(vk["beta"])), (proof["c"], R.ec_neg(vk["delta"]))]
    for pairs in ([(R.G1_GEN, R.G2_GEN)], four, [(R.G1_GEN, R.G2_GEN), (None, R.G2_GEN), (vk["alpha"], None)]):
        got = _lanes_product(shim, pairs)
        host = zkhip.pairing_product("host", np.array([[aff_limbs(P) for P, _ in pairs]]), np.array([[aff_limbs(Q) for _, Q in pairs]]))[0]
        assert (got == host).all()
        assert V.fq6_ints(got) == V.gt_value(pairs)
    assert V.fq6_ints(_lanes_product(shim, four)) == V.EXT.one()


@pytest.mark.parametrize("n_inputs", [0, 1, 5])
def test_trapdoor_statements_are_right(n_inputs):
    """The fixtures before a GPU sees them: pyref and the host verifier accept every statement (inputs include 0 and r - 1) and
    reject it with any single input bumped."""
    from zecale_amd import zkhip
    vk, proofs = V.statements(n_inputs)
    vkl = V.vk_limbs(vk)
    for j, (proof, xs) in enumerate(proofs):
        pl = V.proof_limbs(proof)
        assert zkhip.groth16_verify(vkl, V.input_limbs(xs), pl)
        for i in range(n_inputs):
            bad = list(xs); bad[i] = (bad[i] + 1) % R.R_MOD
            assert not zkhip.groth16_verify(vkl, V.input_limbs(bad), pl)
    if n_inputs:
        assert proofs[0][1][0] == 0 and (n_inputs < 2 or proofs[0][1][1] == R.R_MOD - 1)
    proof, xs = proofs[0]                       # pyref's pairing is seconds per call: the first statement and each of its inputs
    assert R.bw6_groth16_verify(vk, proof, xs)
    for i in range(n_inputs):
        bad = list(xs); bad[i] = (bad[i] + 1) % R.R_MOD
        assert not R.bw6_groth16_verify(vk, proof, bad)


def test_no_batch_verifier_without_device():
    import torch
    if torch.cuda.is_available():
        return  # meaningful only on the CPU-only container
    from zecale_amd import zkhip
    lib = zkhip.load()
    vk = V.vk_limbs(V.statements(0)[0])
    handle = ctypes.c_void_p()
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    rc = lib.zkhip_verifier_new(c(vk["alpha"]), c(vk["beta"]), c(vk["delta"]), c(vk["ABC"]), 0, ctypes.byref(handle))
    assert rc == -2, "zkhip_verifier_new must fail with ZKHIP_ERR_NO_DEVICE when there is no GPU"
    assert not handle.value
    with pytest.raises(zkhip.ZkhipError):
        zkhip.Verifier(vk)
    with pytest.raises(zkhip.ZkhipError):
        zkhip.pairing_product("gpu", np.zeros((1, 1, 24), dtype=np.uint64), np.zeros((1, 1, 24), dtype=np.uint64))


def test_lane_bodies_stand_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: every coefficient at q - 1 through the three bodies) built with the address and
    undefined-behaviour sanitizers and run on the CPU: an out-of-range operand index or a shift past a limb's width would stop it."""
    exe = tmp_path / "pairing_shim_sanitized"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPAIRING_SHIM_MAIN",
                           "-o", str(exe), os.path.join(HERE, "pairing_host_shim.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert len(out.stdout.strip()) == 16
