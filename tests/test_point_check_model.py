"""The checked verifier without a GPU: the lane body of k_point_check (zecale_amd/csrc/pairing.cuh point_check) compiled for the HOST by
g++, against the host route (zkhip_bw6_761_point_check) and pyref's big integers on every fixture point; the host verifier with the
checks in front (zkhip_groth16_verify_checked) against the status byte pyref alone gives; keys it refuses; and the checked batch
verifier's refusal to run without a device.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests import point_check_fixtures as F
from tests import verify_fixtures as V

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libpoint_check_host_shim.so")
    src = os.path.join(HERE, "point_check_host_shim.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("pairing.cuh", "ec.cuh", "fp29.cuh", "bw6_params.h")] + [os.path.join(HERE, "..", "include", "zkhip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.point_check_lane.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.inputs_check_lane.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.refusal_byte.argtypes = [ctypes.c_void_p]
    return lib


def _lane(shim, e, g2):
    p = np.ascontiguousarray(e.limbs, dtype=np.uint64)
    return shim.point_check_lane(p.ctypes.data, int(g2))


@pytest.mark.parametrize("g2", [False, True])
def test_lane_body_equals_host_route_and_pyref_on_every_fixture(shim, g2):
    """Small order (the infinity branch of the doubling for order 2, the same-x branch of the addition for order 3), a generator plus a
    small-order point, a generic curve point, a pure cofactor point, two points off the curve, two encodings that are not reduced:
    the lane body, the host route and pyref give one code."""
    from zecale_amd import zkhip
    for e in F.bad_points(g2):
        assert e.code >= F.ENCODING
        assert _lane(shim, e, g2) == e.code, e.name
        assert zkhip.bw6_761_point_check(e.limbs, g2) == e.code, e.name
    # a G1 fixture that is on G1's curve is off G2's and the other way round, except the encodings, which come first
    for e in F.bad_points(not g2):
        want = F.ENCODING if e.code == F.ENCODING else F.OFF_CURVE
        if e.name.endswith("the other group's generator"):
            want = F.ACCEPT                                            # this group's generator
        assert _lane(shim, e, g2) == want == zkhip.bw6_761_point_check(e.limbs, g2), e.name


@pytest.mark.parametrize("g2", [False, True])
def test_lane_body_passes_the_group(shim, g2):
    """the generator, infinity and eight random multiples of the generator: every valid point ends its walk over r's bits with
    (r - 1) P + P, the same-x branch of the mixed addition"""
    from zecale_amd import zkhip
    for e in F.good_points(g2):
        assert e.code == F.ACCEPT
        assert _lane(shim, e, g2) == 0, e.name
        assert zkhip.bw6_761_point_check(e.limbs, g2) == 0, e.name
    zero_x = np.zeros(24, dtype=np.uint64); zero_x[12:] = F.fq_limbs(1)          # x = 0, y = 1 is not infinity and on neither curve
    assert shim.point_check_lane(zero_x.ctypes.data, int(g2)) == F.OFF_CURVE == zkhip.bw6_761_point_check(zero_x, g2)


def test_lane_body_inputs_and_refusal_byte(shim):
    xs = [0, 1, R.R_MOD - 1, 12345]
    good = np.ascontiguousarray(V.input_limbs(xs))
    assert shim.inputs_check_lane(good.ctypes.data, len(xs)) == 0
    assert shim.inputs_check_lane(good.ctypes.data, 0) == 0
    for pos in (0, len(xs) - 1):
        for e in F.bad_inputs(xs[pos]):
            bad = good.copy(); bad[pos] = e.limbs
            assert shim.inputs_check_lane(bad.ctypes.data, len(xs)) == F.ENCODING, (pos, e.name)
    top = np.full(6, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    assert shim.inputs_check_lane(top.ctypes.data, 1) == F.ENCODING
    below = np.array(R.int_to_limbs(R.R_MOD - 1, 6), dtype=np.uint64)             # the largest limbs that are reduced
    assert shim.inputs_check_lane(below.ctypes.data, 1) == 0
    for a in range(5):
        for b in range(5):
            for c in (0, 2, 3, 4):
                for i in (0, 2):
                    if 1 in (a, b):
                        continue
                    e = np.array([a, b, c, i], dtype=np.uint8)
                    assert shim.refusal_byte(e.ctypes.data) == F.status_byte(dict(a=a, b=b, c=c, inputs=i))


def _cases(n_inputs):
    cases = [F.make_case(n_inputs, j) for j in range(8)]                          # the eight valid statements
    cases += [F.make_case(n_inputs, j, bump=True) for j in (0, 5)]
    inf = F.point_elem("infinity", None, False)
    cases += [F.make_case(n_inputs, 1, {"a": inf}, bump=True, label="A at infinity"),    # passes the checks; the pairing rejects
              F.make_case(n_inputs, 2, {"b": F.point_elem("infinity", None, True)}, bump=True, label="B at infinity")]
    for group in F.refused_cases(n_inputs).values():
        cases += group
    return cases


@pytest.mark.parametrize("n_inputs", [0, 1, 5])
def test_host_verifier_checked(n_inputs):
    """zkhip_groth16_verify_checked on the eight valid statements with none, one or several elements replaced by fixtures: its byte is
    the one computed from pyref's codes (precedence: encoding, curve, order; the mask names exactly the elements with that code), and
    where nothing is refused its verdict is zkhip_groth16_verify's."""
    from zecale_amd import zkhip
    vkl = V.vk_limbs(V.statements(n_inputs)[0])
    seen = set()
    for case in _cases(n_inputs):
        got = zkhip.groth16_verify_checked(vkl, case.inputs, case.proof)
        assert got == case.want, (case.label, hex(got), hex(case.want))
        if got <= F.REJECT:
            assert zkhip.groth16_verify(vkl, case.inputs, case.proof) == (got == F.ACCEPT), case.label
        seen.add(got)
    assert {F.ACCEPT, F.REJECT, F.ENCODING | 0x10, F.OFF_CURVE | 0x20, F.NOT_ORDER_R | 0x40, F.NOT_ORDER_R | 0x50} <= seen
    if n_inputs:
        assert {F.ENCODING | 0x80, F.ENCODING | 0xB0} <= seen


def test_a_proof_at_infinity_passes_the_checks_and_pyref_rejects_it():
    """the all-zero point is in the group: the checks pass it and the pairing decides, as pyref's verifier does"""
    from zecale_amd import zkhip
    vk, proofs = V.statements(0)
    proof, xs = proofs[1]
    case = F.make_case(0, 1, {"a": F.point_elem("infinity", None, False)}, bump=True)
    assert not R.bw6_groth16_verify(vk, dict(proof, a=None, c=proof["a"]), xs)
    assert zkhip.groth16_verify_checked(V.vk_limbs(vk), case.inputs, case.proof) == F.REJECT


def test_refused_keys_on_the_host():
    from zecale_amd import zkhip
    proof, xs = V.statements(1)[1][0]
    for name, code, vkl in F.bad_keys(1):
        with pytest.raises(zkhip.ZkhipError) as err:
            zkhip.groth16_verify_checked(vkl, V.input_limbs(xs), V.proof_limbs(proof))
        assert err.value.code == -1                                              # ZKHIP_ERR_ARG
        assert name + ":" in str(err.value) and "(%d)" % code in str(err.value), str(err.value)
    assert zkhip.groth16_verify_checked(V.vk_limbs(V.statements(1)[0]), V.input_limbs(xs), V.proof_limbs(proof)) == F.ACCEPT


def test_no_checked_batch_verifier_without_device():
    import torch
    if torch.cuda.is_available():
        return  # meaningful only on the CPU-only container
    from zecale_amd import zkhip
    lib = zkhip.load()
    vk = V.vk_limbs(V.statements(0)[0])
    handle = ctypes.c_void_p()
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    rc = lib.zkhip_verifier_new_checked(c(vk["alpha"]), c(vk["beta"]), c(vk["delta"]), c(vk["ABC"]), 0, ctypes.byref(handle))
    assert rc in (-2, -4), "zkhip_verifier_new_checked must fail with ZKHIP_ERR_NO_DEVICE or ZKHIP_ERR_STATE when there is no GPU"
    assert not handle.value
    with pytest.raises(zkhip.ZkhipError):
        zkhip.Verifier(vk, checked=True)


def test_lane_body_stand_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: both generators through all 377 bits, infinity, a point of order 2, a coordinate
    equal to q) built with the address and undefined-behaviour sanitizers and run on the CPU."""
    exe = tmp_path / "point_check_shim_sanitized"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPOINT_CHECK_SHIM_MAIN",
                           "-o", str(exe), os.path.join(HERE, "point_check_host_shim.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "0", "0", "4", "2"]
