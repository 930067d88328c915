"""The five register forms of zecale_amd/csrc/ec.cuh (the ZK_HD ones) compiled for the HOST by g++ and run on the cases of
tests/point_ops_cases.py, raw limbs in and out, with the checker that tests/test_point_ops_gpu.py gives the device build.  CPU only:
it validates the cases and the checker without a GPU, and pins the three representation edges for the register forms."""
import ctypes
import os
import subprocess

import pytest

from tests import point_ops_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libpoint_ops_host_shim.so")
    src = os.path.join(HERE, "point_ops_host_shim.cpp")
    hdrs = [os.path.join(HERE, "..", "zecale_amd", "csrc", h) for h in ("ec.cuh", "fp29.cuh", "bw6_params.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.point_op.restype = ctypes.c_int
    return lib


def run(shim, name, case):
    row = (ctypes.c_uint32 * C.ROW_IN)(*C.operands(name, case))
    out = (ctypes.c_uint32 * C.ROW_OUT)()
    assert shim.point_op(C.OPS[name].code, row, out) == 0
    return list(out)


@pytest.mark.parametrize("name", C.REGISTER_OPS)
def test_register_forms_on_raw_limbs(shim, name):
    done = 0
    for case in C.cases(name):
        C.check(name, case, run(shim, name, case))
        done += 1
    assert done == C.n_cases(name) and done >= 300


def test_neg_of_zero_y_is_exactly_4p(shim):
    """xyzz_neg of Y = 0 limbs - the state xyzz_infinity() leaves, and a 2-torsion point - gives exactly 4p: the stored contract of Y
    is Y <= 4p, closed (ec.cuh), and negating again gives 0 back."""
    hits = [c for c in C.cases("xyzz_neg") if c.A[1] == 0]
    assert any(c.pa is None for c in hits) and any(c.pa == C.T2 for c in hits)
    for c in hits:
        v = C.decode("xyzz_neg", run(shim, "xyzz_neg", c))
        assert v[1] == 4 * C.p
        again = C._case(A=v, pa=c.pa)
        assert C.decode("xyzz_neg", run(shim, "xyzz_neg", again))[1] == 0


def test_zz_given_as_p_is_infinity(shim):
    """ZZ = 0 (mod p) as the limbs of p: xyzz_add and xyzz_madd take it for infinity on either side"""
    for name in ("xyzz_add", "xyzz_madd", "xyzz_dbl"):
        hits = [c for c in C.cases(name) if c.pa is None and c.A[2] == C.p]
        assert hits, name
        for c in hits:
            C.check(name, c, run(shim, name, c))
    assert any(c.pb is None and c.B[2] == C.p and c.pa is not None for c in C.cases("xyzz_add"))


def test_an_unknown_op_is_refused(shim):
    out = (ctypes.c_uint32 * C.ROW_OUT)()
    assert shim.point_op(5, (ctypes.c_uint32 * C.ROW_IN)(), out) == -1
