"""The DEVICE build's point layer (zecale_amd/csrc/ec.cuh, ec_mem.cuh, ec_edw.cuh) on raw limbs, through the C ABI's test hook
zkhip_internal_point_ops_selftest: one function per launch, operands staged in the form the library hands them over (registers, packed
points, limb-major and slot references, the LDS images with Y in a register), every coordinate at both ends of its lazy bound and
next to 0 and to k p, waves composed for the same-x vote.  Cases and the checker come from tests/point_ops_cases.py, which
tests/test_point_ops_host.py runs through the g++ build of the register forms and tests/test_point_ops_cases.py checks on its own.
One launch per (op, mem).

The cases P + (1, 0), P in G1, of edw_from_affine are the ones that exposed a defect: the function accepted them, with the packed
words of chi(P) ((1, 0) generates chi's kernel; no denominator vanishes).  It now refuses every point whose x - 1 is not a square."""
import numpy as np
import pytest

from tests import point_ops_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,mem", [(name, mem) for name in C.OPS for mem in C.mems(name)])
def test_device_point_op_on_raw_limbs(zk, name, mem):
    cases = C.cases(name)
    x = np.array([C.operands(name, c) for c in cases], dtype=np.uint32)
    table = np.array(C.lock_table(), dtype=np.uint32) if name == "edw_lock" else None
    got = zk.point_ops_selftest(C.OPS[name].code, mem, x, table)
    assert got.shape == (C.n_cases(name), C.ROW_OUT)
    done, failed = 0, []
    for i, (case, row) in enumerate(zip(cases, got.tolist())):
        try:
            C.check(name, case, row)
        except AssertionError as e:
            failed.append("case %d (lane %d of wave %d): %s" % (i, i % C.wave_cases(name), i // C.wave_cases(name), e))
        done += 1
    assert done == C.n_cases(name) and done >= 300
    print("%s mem %d: %d cases, %d failed" % (name, mem, done, len(failed)))
    assert not failed, "%d of %d cases failed; the first: %s" % (len(failed), done, "\n".join(failed[:5]))


def test_an_unknown_op_is_refused(zk):
    row = np.zeros((1, C.ROW_IN), dtype=np.uint32)
    for op, mem in ((len(C.OPS), 0), (-1, 0), (0, 1), (C.OPS["edw_lock"].code, 1), (C.OPS["madd_mem"].code, 2)):
        with pytest.raises(zk.ZkhipError):
            zk.point_ops_selftest(op, mem, row)
    bad = np.array([C.operands("edw_lock", C._case(entries=(C.LOCK_TABLE_POINTS,)))], dtype=np.uint32)       # an entry past the table
    with pytest.raises(zk.ZkhipError):
        zk.point_ops_selftest(C.OPS["edw_lock"].code, 0, bad, np.array(C.lock_table(), dtype=np.uint32))
