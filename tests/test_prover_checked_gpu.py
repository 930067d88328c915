"""Checked provers (zkhip_prover_set_checked): an assignment that is not reduced, does not start with ONE, does not satisfy the system
or is not masked gets NO proof but ZKHIP_ERR_REFUSED with the kind and the index; acceptable input gets the unchecked prover's proof
limb for limb; with checking off everything is as before.  A system of 300 constraints on a domain of 512 points (not filled) in which
constraint j alone owns variable w_j = <A_j,z><B_j,z>, so that changing w_j breaks exactly constraint j."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests.helpers import crs_from_trapdoor, csr_from_rows, fr_array, fr_limbs, make_r1cs

pytestmark = pytest.mark.gpu

N, L, AUX = 300, 3, 40
R_LIMBS = np.array(R.int_to_limbs(R.R_MOD, 6), dtype=np.uint64)            # r itself: the smallest value that is not reduced
R1_LIMBS = np.array(R.int_to_limbs(R.R_MOD + 1, 6), dtype=np.uint64)

_cache = {}


def _system(zk):
    if "s" not in _cache:
        A, B, _, z = make_r1cs(77, N, L, AUX)
        m0 = len(z)
        C = [[(m0 + j, 1)] for j in range(N)]
        z = z + [R.r1cs_eval_row(A[j], z) * R.r1cs_eval_row(B[j], z) % R.R_MOD for j in range(N)]
        m = len(z)
        rng = random.Random(8)
        tau, alpha, beta, delta, r, s = (rng.randrange(1, R.R_MOD) for _ in range(6))
        pk, d = crs_from_trapdoor(zk, A, B, C, m, L, tau, alpha, beta, delta)
        assert d == 512 and N + L + 1 < d
        csr = tuple(csr_from_rows(x) for x in (A, B, C))
        _cache["s"] = dict(pk=pk, csr=csr, m=m, m0=m0, l=L, d=d, z=fr_array(z), zi=z, r=fr_limbs(r), s=fr_limbs(s))
    return _cache["s"]


def _broken(S, rows):
    """the assignment with w_j + 1 in the place of w_j for every j of rows: exactly those constraints fail"""
    z = S["z"].copy()
    for j in rows:
        z[S["m0"] + j] = fr_limbs((S["zi"][S["m0"] + j] + 1) % R.R_MOD)
    return z


def _refused(zk, call):
    with pytest.raises(zk.ZkhipError) as e:
        call()
    assert e.value.code == zk.ERR_REFUSED, e.value
    return e.value


@pytest.fixture(scope="module")
def xyzz(zk):
    S = _system(zk)
    crs = zk.Crs(S["pk"], S["m"], S["l"], S["d"])
    desc, keep = zk.make_r1cs_desc(*S["csr"], S["m"], S["l"])
    pr = zk.Prover(crs, desc)
    ref = pr.prove(S["z"], S["r"], S["s"])                      # the unchecked prover's proof
    assert zk.groth16_verify(S["pk"]["vk"], S["z"][1:1 + L], ref)
    yield S, pr, ref
    pr.free(); crs.free()


def test_valid_assignment_gets_the_unchecked_proof(zk, xyzz):
    S, pr, ref = xyzz
    pr.set_checked(True)
    try:
        got = pr.prove(S["z"], S["r"], S["s"])
        assert (got == ref).all() and pr.last_refusal()[0] == 0
        assert zk.groth16_verify(S["pk"]["vk"], S["z"][1:1 + L], got)
        dz = zk.DeviceBuffer(S["z"])
        assert (pr.prove_dev(dz.ptr, S["r"], S["s"]) == ref).all() and pr.last_refusal()[0] == 0
        dz.free()
    finally:
        pr.set_checked(False)


@pytest.mark.parametrize("rows,first", (((0,), 0), ((N // 2 + 1,), N // 2 + 1), ((N - 1,), N - 1), ((211, 37), 37), ((N - 1, 0), 0)))
@pytest.mark.parametrize("dev", (False, True), ids=("host", "dev"))
def test_broken_constraints_are_refused_with_the_first_index(zk, xyzz, rows, first, dev):
    S, pr, ref = xyzz
    z = _broken(S, rows)
    dz = zk.DeviceBuffer(z) if dev else None
    prove = (lambda: pr.prove_dev(dz.ptr, S["r"], S["s"])) if dev else (lambda: pr.prove(z, S["r"], S["s"]))
    unchecked = prove()                                         # checking off: ZKHIP_OK, as today - a proof that does not verify
    assert not (unchecked == ref).all() and not zk.groth16_verify(S["pk"]["vk"], z[1:1 + L], unchecked)
    pr.set_checked(True)
    try:
        err = _refused(zk, prove)
        assert pr.last_refusal() == (zk.REFUSAL_UNSAT, first), err
        assert (pr.prove(S["z"], S["r"], S["s"]) == ref).all() and pr.last_refusal() == (0, 0)      # the same prover, after a refusal
    finally:
        pr.set_checked(False)
        if dz:
            dz.free()


@pytest.mark.parametrize("what,index,limbs,kind", (("r", 7, R_LIMBS, "ENCODING"), ("r + 1", 1, R1_LIMBS, "ENCODING"), ("r + 1", -1, R1_LIMBS, "ENCODING"),
                                                   ("2", 0, None, "ONE")))
def test_unreduced_entries_and_a_wrong_one(zk, xyzz, what, index, limbs, kind):
    S, pr, ref = xyzz
    z = S["z"].copy()
    index %= S["m"]
    z[index] = fr_limbs(2) if limbs is None else limbs
    assert pr.prove(z, S["r"], S["s"]).shape == (72,)           # checking off: ZKHIP_OK, as today
    pr.set_checked(True)
    try:
        _refused(zk, lambda: pr.prove(z, S["r"], S["s"]))
        assert pr.last_refusal() == (getattr(zk, "REFUSAL_" + kind), index)     # (the constraints fail too: the smallest kind is reported)
        dz = zk.DeviceBuffer(z)
        _refused(zk, lambda: pr.prove_dev(dz.ptr, S["r"], S["s"]))
        assert pr.last_refusal() == (getattr(zk, "REFUSAL_" + kind), index)
        dz.free()
        assert (pr.prove(S["z"], S["r"], S["s"]) == ref).all()
    finally:
        pr.set_checked(False)


def test_several_kinds_report_the_smallest(zk, xyzz):
    S, pr, ref = xyzz
    z = _broken(S, (5,))
    z[0] = fr_limbs(2)
    z[9] = R_LIMBS
    z[4] = R1_LIMBS
    pr.set_checked(True)
    try:
        _refused(zk, lambda: pr.prove(z, S["r"], S["s"]))
        assert pr.last_refusal() == (zk.REFUSAL_ENCODING, 4)
        z[9] = S["z"][9]; z[4] = S["z"][4]
        _refused(zk, lambda: pr.prove(z, S["r"], S["s"]))
        assert pr.last_refusal() == (zk.REFUSAL_ONE, 0)
    finally:
        pr.set_checked(False)


@pytest.mark.parametrize("strategy", ("edwards", "edwards-streaming", "streaming", "split", "separate"))
def test_every_strategy_of_a_proof(zk, xyzz, strategy):
    """the flag words come back whichever way the proof is enqueued: an Edwards key (two launch sequences), a streaming prover (chained
    from its second proof on), the split form, one launch sequence per MSM"""
    S, _, ref = xyzz
    opts = dict(edwards=zk.key_opts(table_model=1), separate=zk.key_opts(batch_msms=False)).get(strategy.split("-")[0])
    crs = zk.Crs(S["pk"], S["m"], S["l"], S["d"], opts=opts)
    desc, keep = zk.make_r1cs_desc(*S["csr"], S["m"], S["l"])
    pr = zk.Prover(crs, desc)
    if strategy == "split":
        zk.set_prove_split(1)
    try:
        if strategy.endswith("streaming"):
            pr.set_streaming(True)
        assert (pr.prove(S["z"], S["r"], S["s"]) == ref).all()
        pr.set_checked(True)
        for _ in range(2):                                      # (a streaming prover's second proof is the chained one)
            assert (pr.prove(S["z"], S["r"], S["s"]) == ref).all() and pr.last_refusal() == (0, 0)
            _refused(zk, lambda: pr.prove(_broken(S, (150, 299)), S["r"], S["s"]))
            assert pr.last_refusal() == (zk.REFUSAL_UNSAT, 150)
        z = S["z"].copy(); z[S["m"] - 1] = R1_LIMBS
        _refused(zk, lambda: pr.prove(z, S["r"], S["s"]))
        assert pr.last_refusal() == (zk.REFUSAL_ENCODING, S["m"] - 1)
        assert (pr.prove(S["z"], S["r"], S["s"]) == ref).all()
        t = pr.timings()
        if strategy.startswith("edwards"):
            assert crs.table_model == 1 and pr.last_table_model() == 1
        if strategy.endswith("streaming"):
            assert t["chained"]
        if strategy == "split":
            assert zk.load().zkhip_prover_timings_chained(pr.handle) == 2
    finally:
        zk.set_prove_split(0)
        pr.free(); crs.free()


def test_unmasked_application_assignment(zk):
    """prove_app_dev ORs a device assignment into the application's constants: unmasked, a checked prover refuses it (APP_MASK, the
    first constant's position), unchecked it returns ZKHIP_OK as today; a masked one gets the plain proof."""
    from tests.test_aggregator_gpu import _setup
    from tests.test_app_cache_gpu import _batch
    agg, desc, kp, nvk_l, proofs = _setup(zk)
    crs = kp.upload_crs()
    app = zk.AggregatorApp(agg, crs, nvk_l)
    pr = zk.Prover(crs, desc)
    r, s = fr_limbs(0x1111), fr_limbs(0x2222)
    try:
        npr, nin = _batch(proofs, 0, 1)
        z = agg.witness(nvk_l, npr, nin)
        zm = app.mask(z)
        pos = app.constants()[0]
        plain = pr.prove(z, r, s)
        d_full, d_masked = zk.DeviceBuffer(z), zk.DeviceBuffer(zm)
        assert pr.prove_app_dev(app, d_full.ptr, r, s).shape == (72,)           # checking off: ZKHIP_OK
        pr.set_checked(True)
        _refused(zk, lambda: pr.prove_app_dev(app, d_full.ptr, r, s))
        assert pr.last_refusal() == (zk.REFUSAL_APP_MASK, int(pos[0]))
        _refused(zk, lambda: pr.prove_app(app, z, r, s))                         # the host form: the same refusal
        assert pr.last_refusal() == (zk.REFUSAL_APP_MASK, int(pos[0]))
        assert (pr.prove_app_dev(app, d_masked.ptr, r, s) == plain).all() and pr.last_refusal() == (0, 0)
        assert (pr.prove_app(app, zm, r, s) == plain).all()
        assert (pr.prove(z, r, s) == plain).all()
        d_full.free(); d_masked.free()
    finally:
        pr.free(); app.free(); crs.free(); kp.free(); agg.free()
