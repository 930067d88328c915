"""Batches of 32 nested proofs on the GPU: the workgroup-per-witness interpreter (zecale_amd/csrc/witness.hip: k_witness_wide<2 | 4 | 8 |
16>) on wide synthetic programs and on the real programs of (32, 1) and (32, 9), and wrapping proofs of those circuits on the 2^20
and 2^21 domains.  Every comparison is EXACT: assignments, flags, primary inputs and proofs are equal limb for limb.

The synthetic programs (tests/witness_programs_wide.py: levels of 1 .. 20 chunks, operands in the previous level's chunks of other
waves, at the lower edge of the shared LDS ring and two and more levels back, every instruction kind) are compared with
tests/witness_programs.interpret; the real programs with the host generator; the (32, 1) proof with the C oracle's.

DESIGN.md section 9c says what has been measured."""
import time

import numpy as np
import pytest

from tests import witness_programs as W
from tests import witness_programs_wide as WW
from tests.helpers import fr_int, fr_limbs, random_fr_uniform
from tests.batch32_fixtures import big_batch, bits_without, bumped_proofs

pytestmark = pytest.mark.gpu

TRAPDOOR = (0x1234567, 0x2345678, 0x3456789, 0x456789a)
_PROGS = {seed: WW.wide_program(seed) for seed in (1, 2)}
_X = {seed: W.random_inputs(300 + seed, 5, 64) for seed in _PROGS}
_expected_cache = {}


def _expected(prog, X, i):
    k = (prog["name"], X[i].tobytes())
    if k not in _expected_cache:
        _expected_cache[k] = W.expected(prog, X[i])
    return _expected_cache[k]


def _run_and_compare(zk, prog, X, waves, seg):
    z, flags = zk.witness_run_program(prog, X, 4, seg, waves=waves)
    assert z.shape == (len(X), len(prog["out_ref"]), 6) and flags.shape == (len(X),)
    for i in range(len(X)):
        want, flag = _expected(prog, X, i)
        if not (z[i] == want).all():
            pytest.fail("%s, %d waves, segment %d, batch %d of %d: %r" % (prog["name"], waves, seg, i, len(X), W.first_difference(prog, X[i], z[i])))
        assert int(flags[i]) == flag, "%s, %d waves, segment %d: flag of batch %d is %d, expected %d" % (prog["name"], waves, seg, i, int(flags[i]), flag)
    return z, flags


def _segments(prog):
    """1: a launch per level; 25 and 41: launches of odd and even numbers of levels (asserted); the whole program in one launch"""
    assert set(WW.launches(prog, 1)) == {1}
    assert any(n > 1 and n % 2 for n in WW.launches(prog, 25)) and any(n > 1 and n % 2 for n in WW.launches(prog, 41))
    return [1, 25, 41, len(prog["code"]) // 64]


@pytest.mark.parametrize("batches", [1, 2, 5])
@pytest.mark.parametrize("waves", WW.WAVES)
@pytest.mark.parametrize("seed", sorted(_PROGS))
def test_wide_synthetic_programs(zk, seed, waves, batches):
    """levels of 1 .. 20 chunks shared by 2, 4, 8 and 16 waves, 1, 2 and 5 witnesses per launch (a workgroup each), launches cut after
    every level, after odd numbers of levels, and not at all: every value of every batch equals the reference"""
    prog = _PROGS[seed]
    ring, mem, pre = WW.operand_sources(prog)
    assert ring > 1000 and mem > 200 and pre > 1000
    for seg in _segments(prog):
        _, flags = _run_and_compare(zk, prog, _X[seed][:batches], waves, seg)
        assert not flags.any()


@pytest.mark.parametrize("waves", WW.WAVES)
def test_wide_program_flags_only_the_batch_whose_inversion_meets_zero(zk, waves):
    prog = WW.wide_program(3, inv_of_input0=True)
    assert int(prog["code"][64]) == W.WT_INV and int(prog["a"][64]) == 0
    X = W.random_inputs(404, 5, 64)
    z, flags = _run_and_compare(zk, prog, X, waves, 25)
    assert not flags.any()
    Xb = X.copy()
    Xb[2, 0] = 0
    zb, fb = _run_and_compare(zk, prog, Xb, waves, 25)
    assert [int(f) for f in fb] == [0, 0, 1, 0, 0]
    assert (zb[[0, 1, 3, 4]] == z[[0, 1, 3, 4]]).all()


def test_width_one_is_the_narrow_kernel_and_other_widths_are_refused(zk):
    """waves = 1 runs today's k_witness (cut by chunks: segment 7 splits levels, which the wide kernels never do) on the wide programs
    too; a width that does not exist is refused before anything is uploaded"""
    prog = _PROGS[1]
    _run_and_compare(zk, prog, _X[1][:2], 1, 7)
    for waves in (3, 32, -1):
        with pytest.raises(zk.ZkhipError) as e:
            zk.witness_run_program(prog, _X[1][:2], 4, 7, waves=waves)
        assert e.value.code == -1


# ---------------------------------------------------------------------------------------------------------- the real programs
def _three_batches(n, k):
    """a valid batch, one with proofs 0, n / 2 + 1 and n - 1 bumped, one under a degenerate key (ABC_1 = ABC_0: the host generator
    branches where the recorded program cannot)"""
    vk, pr, inp, _ = big_batch(n, k)
    _, _, inp_b, _ = big_batch(n, k, bumped_proofs(n))
    vk_deg = vk.copy(); vk_deg[72:84] = vk_deg[60:72]
    return [(vk, pr, inp), (vk, pr, inp_b), (vk_deg, pr, inp)]


@pytest.mark.parametrize("n,k,widths", [(32, 1, (1, 4, 8, 0)), (32, 9, (0,))], ids=["32x1", "32x9"])
def test_real_programs_of_32_proofs(zk, n, k, widths):
    """three batches per launch at every width: each assignment equals the host generator's limb for limb, the primary inputs are
    equal, the degenerate batch alone is flagged, one assignment per configuration satisfies every constraint"""
    agg = zk.AggregatorCircuit(n, k)
    r1 = zk.r1cs_from_desc(zk.r1cs_desc_from_aggregator(agg))
    batches = _three_batches(n, k)
    host = [agg.witness(*b) for b in batches[:2]]
    assert [fr_int(z[2]) for z in host] == [(1 << n) - 1, bits_without(n, bumped_proofs(n))]
    l = agg.num_primary_inputs()
    for cfg, waves in enumerate(widths):
        t = time.time()
        z, flagged, prim = agg.witness_gpu_batched(batches, waves=waves)
        print("(%d, %d) waves %d: three witnesses in %.0f ms (with allocation and copies)" % (n, k, waves, (time.time() - t) * 1e3))
        assert [bool(f) for f in flagged] == [False, False, True], (waves, list(flagged))
        for i in range(2):
            assert (z[i] == host[i]).all(), "waves %d, batch %d: first difference at variable %d" % (waves, i, int(np.nonzero((z[i] != host[i]).any(axis=1))[0][0]))
            assert (prim[i] == host[i][1:1 + l]).all()
        assert r1.is_satisfied(z[cfg % 2])
    r1.free(); agg.free()


@pytest.fixture(scope="module")
def proving32(zk):
    """the circuit of 32 one-input proofs with a key on the 2^20 domain"""
    agg = zk.AggregatorCircuit(32, 1)
    desc = zk.r1cs_desc_from_aggregator(agg)
    t = time.time()
    kp = zk.Keypair(desc, *(fr_limbs(x) for x in TRAPDOOR))
    print("setup of (32, 1): %.1f s" % (time.time() - t))
    assert kp.domain_size == 1 << 20
    crs, r1 = kp.upload_crs(), zk.r1cs_from_desc(desc)
    yield agg, desc, kp, crs, r1
    crs.free(); r1.free(); kp.free(); agg.free()


def test_wrapping_proof_of_32_proofs_equals_the_oracle(zk, oracle_lib, proving32):
    """one proof from the host assignment and one from the device assignment (generated at the auto width, proved where it lies):
    both equal the C oracle's proof limb for limb and verify; the result bits are 2^32 - 1, and the complement pattern with proofs
    0, 17 and 31 bumped"""
    O = oracle_lib
    agg, desc, kp, crs, r1 = proving32
    l = agg.num_primary_inputs()
    pk, m, l_pk, dom = kp.pk_arrays()
    assert l_pk == l and dom == 1 << 20 == O.qap_domain_size(agg.num_constraints, l, None)
    A, B, C = agg.get_constraint_system()
    rs = random_fr_uniform(3232, 2)
    vk_l, pr, inp, _ = big_batch(32, 1)
    _, _, inp_b, _ = big_batch(32, 1, bumped_proofs(32))
    z = agg.witness(vk_l, pr, inp)
    assert fr_int(z[2]) == (1 << 32) - 1
    t = time.time()
    h = O.qap_h(A, B, C, z, agg.num_constraints, l, dom)
    expect = O.groth16_prove(pk, z, l, h, rs[0], rs[1])
    print("oracle proof of (32, 1): %.1f s" % (time.time() - t))
    vk = kp.vk()
    assert zk.groth16_verify(vk, z[1:1 + l], expect)
    assert (zk.groth16_prove(crs, r1, z, rs[0], rs[1]) == expect).all()
    gw = zk.GpuWitness(agg, 2)
    pv = zk.Prover(crs, desc)
    d_z, deg, prim = gw.run([(vk_l, pr, inp), (vk_l, pr, inp_b)])
    assert not deg.any() and (prim[0] == z[1:1 + l]).all()
    assert (pv.prove_dev(d_z[0], rs[0], rs[1]) == expect).all()
    assert fr_int(prim[1][1]) == 0x7ffdfffe == bits_without(32, bumped_proofs(32))
    proof_b = pv.prove_dev(d_z[1], rs[1], rs[0])
    assert zk.groth16_verify(vk, prim[1], proof_b)
    assert (proof_b == zk.groth16_prove(crs, r1, agg.witness(vk_l, pr, inp_b), rs[1], rs[0])).all()
    tampered = prim[1].copy(); tampered[1] = fr_limbs((1 << 32) - 1)
    assert not zk.groth16_verify(vk, tampered, proof_b)
    for waves in (1, 8):                              # the handle's option: the same assignment at every width
        gw.set_waves(waves)
        d_z, deg, prim2 = gw.run([(vk_l, pr, inp)])
        assert not deg.any() and (gw.copy_out(0) == z).all() and (prim2[0] == prim[0]).all()
    with pytest.raises(zk.ZkhipError) as e:
        gw.set_waves(3)
    assert e.value.code == -1
    pv.free(); gw.free()


def test_application_handle_and_pipeline_at_32_proofs(zk, proving32):
    """with an application handle the masked proof equals the plain proof; a streaming prover with the GPU generator gives the serial
    path's proofs for two batches"""
    agg, desc, kp, crs, r1 = proving32
    vk = kp.vk()
    vk_l, pr, inp, _ = big_batch(32, 1)
    _, _, inp_b, _ = big_batch(32, 1, bumped_proofs(32))
    rs = random_fr_uniform(3233, 4)
    plain = [zk.groth16_prove(crs, r1, agg.witness(vk_l, pr, x), rs[2 * i], rs[2 * i + 1]) for i, x in enumerate((inp, inp_b))]
    app = zk.AggregatorApp(agg, crs, vk_l)
    assert (app.prove(r1, app.witness(pr, inp), rs[0], rs[1]) == plain[0]).all()
    (zd, zd_b), _ = app.witness_gpu([(pr, inp), (pr, inp_b)])          # the application's own program (auto width)
    assert (zd == app.witness(pr, inp)).all() and (zd_b == app.witness(pr, inp_b)).all()
    app.free()
    pipe = zk.AggregatorPipeline(agg, crs, gpu_slots=2, witness_workers=2, gpu_witness=True)
    tickets = [pipe.submit(vk_l, pr, x, rs[2 * i], rs[2 * i + 1]) for i, x in enumerate((inp, inp_b))]
    for i, t in enumerate(tickets):
        prim, proof = pipe.wait(t)
        assert (proof == plain[i]).all()
        assert fr_int(prim[1]) == ((1 << 32) - 1 if i == 0 else 0x7ffdfffe)
        assert zk.groth16_verify(vk, prim, proof)
    pipe.free()


def test_wrapping_proof_of_32_nine_input_proofs(zk):
    """(32, 9) on the 2^21 domain: the proofs from the host assignment and from the device assignment are identical and verify"""
    agg = zk.AggregatorCircuit(32, 9)
    desc = zk.r1cs_desc_from_aggregator(agg)
    t = time.time()
    kp = zk.Keypair(desc, *(fr_limbs(x) for x in TRAPDOOR))
    print("setup of (32, 9): %.1f s" % (time.time() - t))
    assert kp.domain_size == 1 << 21
    crs, r1 = kp.upload_crs(), zk.r1cs_from_desc(desc)
    l = agg.num_primary_inputs()
    rs = random_fr_uniform(3299, 2)
    vk_l, pr, inp, _ = big_batch(32, 9)
    z = agg.witness(vk_l, pr, inp)
    assert fr_int(z[2]) == (1 << 32) - 1
    proof = zk.groth16_prove(crs, r1, z, rs[0], rs[1])
    assert zk.groth16_verify(kp.vk(), z[1:1 + l], proof)
    gw = zk.GpuWitness(agg, 1)
    pv = zk.Prover(crs, desc)
    d_z, deg, prim = gw.run([(vk_l, pr, inp)])
    assert not deg.any() and (prim[0] == z[1:1 + l]).all()
    assert (pv.prove_dev(d_z[0], rs[0], rs[1]) == proof).all()
    pv.free(); gw.free(); crs.free(); r1.free(); kp.free(); agg.free()
