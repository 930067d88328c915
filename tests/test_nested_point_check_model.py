"""The checked nested (BLS12-377) verifier without a GPU: the lane bodies of k_nested_point_check (zecale_amd/csrc/pairing_bls.cuh
nested_point_check, nested_inputs_check) compiled for the HOST by g++, against the host route (zkhip_bls12_377_point_check) and Python
big integers on every fixture point; the host verifier with the checks in front (zkhip_bls12_377_groth16_verify_checked) against the
status byte the fixtures compute; keys it refuses; and the checked batch verifier's refusal to run without a device.  CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import nested_point_check_fixtures as F
from tests import nested_verify_fixtures as N

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "zecale_amd", "csrc")
SHIM_SRC = os.path.join(HERE, "nested_point_check_host_shim.cpp")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libnested_point_check_host_shim.so")
    hdrs = [os.path.join(CSRC, h) for h in ("pairing_bls.cuh", "pairing.cuh", "ec.cuh", "fp29.cuh", "fp_inv.cuh", "bw6_params.h")]
    hdrs.append(os.path.join(HERE, "..", "include", "zkhip.h"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [SHIM_SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SHIM_SRC])
    lib = ctypes.CDLL(so)
    lib.nested_point_check_lane.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.nested_inputs_check_lane.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    lib.nested_refusal_byte.argtypes = [ctypes.c_void_p]
    lib.nested_order_body_fr2.argtypes = [ctypes.c_void_p]
    lib.nested_order_body_fr.argtypes = [ctypes.c_void_p]
    return lib


def _lane(shim, e, g2):
    p = np.ascontiguousarray(e.limbs, dtype=np.uint64)
    assert p.size == (24 if g2 else 12)
    return shim.nested_point_check_lane(p.ctypes.data, int(g2))


@pytest.mark.parametrize("g2", [False, True])
def test_lane_body_equals_host_route_and_python_on_every_refused_fixture(shim, g2):
    """Orders 2, 3 and 6 (the doubling that ends at ZZ = 0, the same-x branch of the addition in the second iteration), a generator
    plus a cofactor point, a generic curve point, a pure cofactor point, points off the curve (all zero among them: the nested format
    has no point at infinity), encodings that are not reduced: the lane body, the host route and Python give one code."""
    from zecale_amd import zkhip
    for e in F.bad_points(g2):
        assert e.code >= F.ENCODING
        assert _lane(shim, e, g2) == e.code, e.name
        assert zkhip.bls12_377_point_check(e.limbs, g2) == e.code, e.name


@pytest.mark.parametrize("g2", [False, True])
def test_lane_body_passes_the_group(shim, g2):
    """the generator and eight random multiples of it: every valid point ends its walk over r's bits with (r - 1) P + P, the same-x
    branch of the mixed addition"""
    from zecale_amd import zkhip
    for e in F.good_points(g2):
        assert e.code == F.ACCEPT
        assert _lane(shim, e, g2) == 0, e.name
        assert zkhip.bls12_377_point_check(e.limbs, g2) == 0, e.name


def test_order_body_doubles_a_point_with_y_zero_over_fr2(shim):
    """The Y = 0 doubling of the Fr2 body, at body level: [r] (x, 0) = (x, 0) by the Python affine law, so the walk does not end at
    infinity; and the Fr body on (-1, 0) and on the generator, for the two answers of the same function."""
    limbs, ends_at_infinity = F.fr2_y_zero_case()
    assert not ends_at_infinity
    assert shim.nested_order_body_fr2(limbs.ctypes.data) == int(ends_at_infinity)
    gen2 = F.good_points(True)[0].limbs
    assert shim.nested_order_body_fr2(gen2.ctypes.data) == 1
    assert shim.nested_order_body_fr(F.bad_points(False)[0].limbs.ctypes.data) == 0
    assert shim.nested_order_body_fr(F.good_points(False)[0].limbs.ctypes.data) == 1


def test_lane_body_inputs_and_refusal_byte(shim):
    from zecale_amd import zkhip
    xs = [0, 1, F.RM - 1, 12345]
    good = np.ascontiguousarray(N.input_limbs(xs))
    assert shim.nested_inputs_check_lane(good.ctypes.data, len(xs)) == 0
    assert shim.nested_inputs_check_lane(good.ctypes.data, 0) == 0
    refused, fine = F.input_elems(xs[3])
    for pos in (0, len(xs) - 1):
        for e in refused:
            bad = good.copy(); bad[pos] = e.limbs
            assert shim.nested_inputs_check_lane(bad.ctypes.data, len(xs)) == F.ENCODING, (pos, e.name)
        for e in fine:
            ok = good.copy(); ok[pos] = e.limbs
            assert shim.nested_inputs_check_lane(ok.ctypes.data, len(xs)) == 0, (pos, e.name)
    top = np.full(6, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    assert shim.nested_inputs_check_lane(top.ctypes.data, 1) == F.ENCODING
    for v, want in ((F.RM + 1, F.ENCODING), (1 << 253, F.ENCODING), (F.Q - 1, F.ENCODING), (F.RM - 2, 0), (1 << 252, 0)):
        one = np.array(N.fl(v), dtype=np.uint64)
        assert shim.nested_inputs_check_lane(one.ctypes.data, 1) == want, hex(v)
    for a in range(5):
        for b in range(5):
            for c in (0, 2, 3, 4):
                for i in (0, 2):
                    if 1 in (a, b):
                        continue
                    e = np.array([a, b, c, i], dtype=np.uint8)
                    assert shim.nested_refusal_byte(e.ctypes.data) == F.status_byte(dict(a=a, b=b, c=c, inputs=i))
    assert zkhip.VERIFY_MASK_INPUT == F.MASK["inputs"]


def _cases(n_inputs):
    cases = [F.make_case(n_inputs, j) for j in range(8)]                          # eight valid statements
    cases += [F.make_case(n_inputs, j, bump=True) for j in (0, 5)]
    if n_inputs:
        cases += F.fine_input_cases(n_inputs)
    for group in F.refused_cases(n_inputs).values():
        cases += group
    return cases


@pytest.mark.parametrize("n_inputs", [0, 1, 3])
def test_host_verifier_checked(n_inputs):
    """zkhip_bls12_377_groth16_verify_checked on valid statements with none, one or several elements replaced by fixtures: its byte is
    the one computed from Python's codes (precedence: encoding, curve, order; the mask names exactly the elements with that code), and
    where nothing is refused its verdict is zkhip_bls12_377_groth16_verify's."""
    from zecale_amd import zkhip
    vkl = N.vk_limbs(N.statements(n_inputs)[0])
    seen = set()
    for case in _cases(n_inputs):
        got = zkhip.bls12_377_groth16_verify_checked(vkl, case.inputs, case.proof)
        assert got == case.want, (case.label, hex(got), hex(case.want))
        if got <= F.REJECT:
            assert zkhip.bls12_377_groth16_verify(vkl, case.inputs, case.proof) == (got == F.ACCEPT), case.label
        seen.add(got)
    want = {F.ACCEPT, F.REJECT}
    want |= {code | F.MASK[slot] for code in (F.ENCODING, F.OFF_CURVE, F.NOT_ORDER_R) for slot in "abc"}
    want |= {F.NOT_ORDER_R | 0x50}
    if n_inputs:
        want |= {F.ENCODING | 0x80, F.ENCODING | 0xB0}
    assert want <= seen, sorted(hex(w) for w in want - seen)


@pytest.mark.parametrize("x,negated", [(4, False), (8, False), (8, True)])
def test_degenerate_statements_keep_the_unchecked_host_verdict(x, negated):
    """statements on which the host's affine accumulator meets a degenerate step pass every check: the byte is 0 / 1 as the unchecked
    host function decides"""
    from zecale_amd import zkhip
    vk, pr, xs = N.degenerate_statement(x, negated)
    vkl = N.vk_limbs(vk)
    ok = zkhip.bls12_377_groth16_verify(vkl, N.input_limbs(xs), N.proof_limbs(pr))
    assert zkhip.bls12_377_groth16_verify_checked(vkl, N.input_limbs(xs), N.proof_limbs(pr)) == (F.ACCEPT if ok else F.REJECT)


def test_refused_keys_on_the_host_and_without_a_device():
    import torch
    from zecale_amd import zkhip
    lib = zkhip.load()
    proof, xs = N.statements(1)[1][0]
    c = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    for name, code, vkl in F.bad_keys(1):
        with pytest.raises(zkhip.ZkhipError) as err:
            zkhip.bls12_377_groth16_verify_checked(vkl, N.input_limbs(xs), N.proof_limbs(proof))
        assert err.value.code == -1                                              # ZKHIP_ERR_ARG
        assert name + ":" in str(err.value) and "(%d)" % code in str(err.value), str(err.value)
        # the constructor checks the key on the host before it asks for a device: the same refusal with or without one
        handle = ctypes.c_void_p()
        assert lib.zkhip_nested_verifier_new_checked(c(vkl), 1, ctypes.byref(handle)) == -1 and not handle.value
        msg = lib.zkhip_last_error().decode()
        assert name + ":" in msg and "(%d)" % code in msg, msg
    good = N.vk_limbs(N.statements(1)[0])
    assert zkhip.bls12_377_groth16_verify_checked(good, N.input_limbs(xs), N.proof_limbs(proof)) == F.ACCEPT
    if not torch.cuda.is_available():                                            # a good key: no device, no handle
        handle = ctypes.c_void_p()
        rc = lib.zkhip_nested_verifier_new_checked(c(good), 1, ctypes.byref(handle))
        assert rc in (-2, -4), "zkhip_nested_verifier_new_checked must fail with ZKHIP_ERR_NO_DEVICE or ZKHIP_ERR_STATE when there is no GPU"
        assert not handle.value
        with pytest.raises(zkhip.ZkhipError):
            zkhip.NestedVerifier(good, 1, checked=True)


def _hex(limbs):
    return "".join("%016x" % int(w) for w in limbs)


def test_lane_body_stand_alone_under_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main) built with the address and undefined-behaviour sanitizers and run on the CPU:
    both generators through all 253 bits, (-1, 0) of order 2, a coordinate equal to q.  Nothing is loaded into Python."""
    exe = tmp_path / "nested_point_check_shim_sanitized"
    # (no -g: the variable tracking of the fully inlined Fr2 walk alone takes g++ three quarters of a minute)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPOINT_CHECK_SHIM_MAIN",
                           "-o", str(exe), SHIM_SRC])
    g1 = F.bad_points(False)
    args = [_hex(F.good_points(False)[0].limbs), _hex(F.good_points(True)[0].limbs), _hex(g1[0].limbs), _hex(g1[9].limbs)]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["0", "0", "4", "2"]
