"""The DEVICE build's field layer below the multipliers (zecale_amd/csrc/fp29.cuh, fp_inv.cuh) on raw limbs, through the C ABI's test
hook zkhip_internal_field_ops_selftest, against exact integers: the lazy linear operations at their borrow and bound edges, the range
folds and the zero test around every multiple of p, the packing at every bit, and fp_inv in waves that mix lanes of different loop
length (a finished lane keeps running batches until its wave's vote lets it go - a path only the device build has).  Cases and
expectations come from tests/field_ops_cases.py, which tests/test_fp29_host.py runs through the g++ build and
tests/test_field_ops_cases.py checks on its own.  One launch per (field, op)."""
import numpy as np
import pytest

from tests import field_ops_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,op", [(name, op) for name, f in C.FIELDS.items() for op in C.ops_for(f)])
def test_device_field_op_on_raw_limbs(zk, name, op):
    f = C.FIELDS[name]
    cases = C.cases(name, op)
    x = np.array([C.operands(f, op, c) for c in cases], dtype=np.uint32)
    got = zk.field_ops_selftest(f.index, C.OP_CODES[op], x)
    assert got.shape == (C.n_cases(name, op), f.nl + 1)
    done = 0
    for case, row in zip(cases, got.tolist()):
        C.check(f, op, case, row)
        done += 1
    assert done == C.n_cases(name, op) and done >= 300


@pytest.mark.parametrize("name", list(C.FIELDS))
def test_an_op_of_the_other_field_is_refused(zk, name):
    f = C.FIELDS[name]
    other = [o for g in C.FIELDS.values() for o in C.ops_for(g) if o not in C.ops_for(f)][0]
    with pytest.raises(zk.ZkhipError):
        zk.field_ops_selftest(f.index, C.OP_CODES[other], np.zeros((1, 3, f.nl), dtype=np.uint32))
