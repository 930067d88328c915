"""The product's device field arithmetic (zecale_amd/csrc/fp29.cuh) compiled for the HOST by g++
and checked against big integers / golden vectors.  CPU only (no compute through libzkhip)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import pyref as R
from tests.helpers import golden, h2i

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "libfp29_host_shim.so")
    src = os.path.join(HERE, "fp29_host_shim.cpp")
    hdrs = [os.path.join(HERE, "..", "zecale_amd", "csrc", h) for h in ("fp29.cuh", "fp_inv.cuh", "bw6_params.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    return ctypes.CDLL(so)


def _arr(x, n):
    return (ctypes.c_uint64 * n)(*R.int_to_limbs(x, n))


@pytest.mark.parametrize("name,p,n", [("fq", R.Q_MOD, 12), ("fr", R.R_MOD, 6)])
def test_fp29_against_golden_and_random(shim, name, p, n):
    Rm = 1 << (64 * n)
    tm = lambda x: x * Rm % p
    fm = lambda X: X * pow(Rm, -1, p) % p
    out = (ctypes.c_uint64 * n)()
    rng = random.Random(11)
    vecs = [(h2i(v["a"]), h2i(v["b"])) for v in golden("field_vectors.json")[name]]
    vecs += [(rng.randrange(p), rng.randrange(p)) for _ in range(200)]
    vecs += [(p - 1, p - 1), (p - 1, 1), (0, p - 1), (p - 2, p - 3)]
    for a, b in vecs:
        getattr(shim, name + "_mul")(_arr(tm(a), n), _arr(tm(b), n), out)
        assert fm(R.limbs_to_int(out)) == a * b % p
        getattr(shim, name + "_sqr")(_arr(tm(a), n), out)
        assert fm(R.limbs_to_int(out)) == a * a % p
        getattr(shim, name + "_add")(_arr(tm(a), n), _arr(tm(b), n), out)
        assert fm(R.limbs_to_int(out)) == (a + b) % p
        getattr(shim, name + "_sub_sub2")(_arr(tm(a), n), _arr(tm(b), n), _arr(tm((a ^ b) % p), n), out)
        assert fm(R.limbs_to_int(out)) == (a - b - 2 * ((a ^ b) % p)) % p          # one carry pass for a - b - 2c + 8p
        # the dual product (one reduction for a b + c d): plain operands, then lazily bounded ones with every limb near its maximum
        c, d = (a * 3 + 1) % p, (b * b + 7) % p
        getattr(shim, name + "_mul2")(_arr(tm(a), n), _arr(tm(b), n), _arr(tm(c), n), _arr(tm(d), n), out)
        assert fm(R.limbs_to_int(out)) == (a * b + c * d) % p
        getattr(shim, name + "_mul2_lazy")(_arr(tm(a), n), _arr(tm(b), n), out)
        assert fm(R.limbs_to_int(out)) == ((3 * a + b) * (3 * a - b) - a * 2 * b) % p
        getattr(shim, name + "_sub")(_arr(tm(a), n), _arr(tm(b), n), out)
        assert fm(R.limbs_to_int(out)) == (a - b) % p
        getattr(shim, name + "_roundtrip")(_arr(tm(a), n), out)
        assert R.limbs_to_int(out) == tm(a)
        getattr(shim, name + "_lazy_chain")(_arr(tm(a), n), _arr(tm(b), n), out)
        s = 2 * (a + b); d = s - 4 * b; m = s * d; t = m - d
        assert fm(R.limbs_to_int(out)) == t * t % p
        w = (ctypes.c_uint32 * (2 * n))()
        getattr(shim, name + "_canon_words")(_arr(tm(a), n), w)
        assert sum(int(w[i]) << (32 * i) for i in range(2 * n)) == a


@pytest.mark.parametrize("name,p,n", [("fq", R.Q_MOD, 12), ("fr", R.R_MOD, 6)])
def test_safegcd_inversion(shim, name, p, n):
    """fp_inv (zecale_amd/csrc/fp_inv.cuh: Bernstein-Yang division steps in batches of 29) against pow(a, -1, p): random values and
    the values that stress the step count (powers of two, p - 2^k, small numbers, 0 -> 0)."""
    Rm = 1 << (64 * n)
    tm = lambda x: x * Rm % p
    fm = lambda X: X * pow(Rm, -1, p) % p
    out = (ctypes.c_uint64 * n)()
    rng = random.Random(5)
    vals = [1, 2, 3, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, 0]
    vals += [1 << k for k in range(1, p.bit_length() - 1, 37)] + [p - (1 << k) for k in range(1, p.bit_length() - 1, 41)]
    vals += [rng.randrange(1, 1 << rng.randrange(1, p.bit_length())) % p for _ in range(200)]
    vals += [rng.randrange(p) for _ in range(800)]
    for a in vals:
        # the shim feeds fp_inv the device Montgomery form of a; every representative the kernels produce is covered by
        # fp_from_abi's output range [0, 2p)
        getattr(shim, name + "_inv")(_arr(tm(a), n), out)
        got = fm(R.limbs_to_int(out))
        assert got == (pow(a, -1, p) if a else 0), hex(a)


@pytest.mark.parametrize("name,p,nl", [("fq", R.Q_MOD, 27), ("fr", R.R_MOD, 14)])
def test_dual_product_at_its_column_bound(shim, name, p, nl):
    """fp_mul2 sums the 2 x NL products of a column in one 64-bit accumulator before the reduction terms join: operands with EVERY limb
    at 2^29 - 1 and the top limb as large as the lazy bound (2^10 p) allows are the worst case of that sum."""
    rng = random.Random(3)
    top_max = ((p << 10) >> (29 * (nl - 1)))            # top limb of values below 2^10 p
    full = [(1 << 29) - 1] * (nl - 1)
    val = lambda limbs: sum(v << (29 * i) for i, v in enumerate(limbs))
    Rdev = 1 << (29 * nl)
    cases = [[full + [top_max - 1]] * 4]
    for _ in range(50):
        cases.append([[rng.choice([(1 << 29) - 1, rng.randrange(1 << 29)]) for _ in range(nl - 1)] + [rng.randrange(top_max)] for _ in range(4)])
    for a, b, c, d in cases:
        if val(a) * val(b) + val(c) * val(d) >= (Rdev * p) << 10:
            a = a[:-1] + [a[-1] >> 6]; c = c[:-1] + [c[-1] >> 6]          # keep a b + c d below 2^10 R p
        arrs = [(ctypes.c_uint32 * nl)(*x) for x in (a, b, c, d)]
        out = (ctypes.c_uint32 * nl)()
        getattr(shim, name + "_mul2_raw")(*arrs, out)
        got = val(list(out))
        assert all(v < (1 << 29) for v in list(out)[:-1])
        assert got % p == (val(a) * val(b) + val(c) * val(d)) * pow(Rdev, -1, p) % p
        assert got < (val(a) * val(b) + val(c) * val(d)) // Rdev + p + 1


def _field_ops():
    from tests import field_ops_cases as C
    return [(name, op) for name, f in C.FIELDS.items() for op in C.ops_for(f)]


@pytest.mark.parametrize("name,op", _field_ops())
def test_field_ops_on_raw_limbs(shim, name, op):
    """Every op of tests/field_ops_cases.py through the g++ build, raw limbs in and out, against the generator's exact expectations: the
    same cases and the same reference that tests/test_field_ops_gpu.py gives the device build.  (On the host fp_inv leaves its loop as
    soon as its own g is 0: the wave layout of the inversion cases matters on the device only.)"""
    from tests import field_ops_cases as C
    f = C.FIELDS[name]
    cases = C.cases(name, op)
    fn = getattr(shim, "%s_op_%s" % (name, op))
    fn.restype = None
    out = (ctypes.c_uint32 * (f.nl + 1))()
    done = 0
    for case in cases:
        a, b, c = ((ctypes.c_uint32 * f.nl)(*x) for x in C.operands(f, op, case))
        fn(a, b, c, out)
        C.check(f, op, case, list(out))
        done += 1
    assert done == C.n_cases(name, op) and done >= 300
