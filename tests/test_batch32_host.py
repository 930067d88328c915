"""Batches of up to 32 nested proofs on the host (NumProofs is a template parameter of the reference, aggregator_circuit.hpp:32-37; its
gadget loops over the proofs, aggregator_gadget.tcc:41-71): the circuit's shape, the host generator's assignment under the C oracle,
the packed result bits, and the plan of the GPU witness generator (zkhip_gpu_witness_plan), which is host code.  CPU only.

The counts of constraints, variables and primary inputs were taken from the circuit with nothing but the limit lifted: lifting it
must not move the circuit."""
import ctypes

import numpy as np
import pytest

from tests import witness_programs_wide as WW
from tests.batch32_fixtures import big_batch, bits_without, bumped_proofs
from tests.helpers import fr_int, fr_limbs

SHAPES = {(32, 1): (575723, 575866, 34), (32, 9): (1230075, 1230234, 290), (17, 3): (397731, 397818, 53)}


_circuits = {}


def circuit_of(n, k):
    """(built once per shape and module: two seconds at 32 proofs of nine inputs)"""
    from zecale_amd import zkhip
    if (n, k) not in _circuits:
        _circuits[(n, k)] = zkhip.AggregatorCircuit(n, k)
    return _circuits[(n, k)]


@pytest.mark.parametrize("n,k", sorted(SHAPES))
def test_shape_is_what_it_was_with_only_the_limit_lifted(n, k):
    c = circuit_of(n, k)
    assert (c.num_constraints, c.num_variables, c.num_primary_inputs()) == SHAPES[(n, k)]
    assert c.num_primary_inputs() == 2 + n * k


def test_limits():
    from zecale_amd import zkhip
    for n, k in ((33, 1), (0, 1), (32, 17), (32, 0), (64, 1)):
        with pytest.raises(zkhip.ZkhipError) as e:
            zkhip.AggregatorCircuit(n, k)
        assert e.value.code == -1, (n, k)
    assert bits_without(32, bumped_proofs(32)) == 0x7ffdfffe and bits_without(17, bumped_proofs(17)) == 0xfdfe


@pytest.mark.parametrize("n,k", sorted(SHAPES))
def test_host_assignment_satisfies_every_constraint(oracle_lib, n, k):
    """a valid batch gives 2^n - 1; with proofs 0, n / 2 + 1 and n - 1 bumped the complement pattern; either assignment satisfies every
    constraint under the C oracle and the other value of one result bit violates one; z[1] is the key's hash; the nested inputs are
    echoed"""
    from zecale_amd import zkhip
    c = circuit_of(n, k)
    A, B, C = c.get_constraint_system()
    for bumped in ((), bumped_proofs(n)):
        vk, pr, inp, xs = big_batch(n, k, bumped)
        z = c.witness(vk, pr, inp)
        assert fr_int(z[0]) == 1
        assert fr_int(z[2]) == bits_without(n, bumped), hex(fr_int(z[2]))
        assert (z[1] == zkhip.aggregator_vk_hash(vk, k)).all() and fr_int(z[1]) != 0
        assert [fr_int(z[3 + i]) for i in range(n * k)] == xs
        assert oracle_lib.r1cs_first_unsatisfied(A, B, C, z) == -1
        zb = z.copy(); zb[2] = fr_limbs(fr_int(z[2]) ^ (1 << (n // 2)))
        assert oracle_lib.r1cs_first_unsatisfied(A, B, C, zb) >= 0
    # the same batch again: the assignment does not depend on which worker thread took which section
    assert (c.witness(vk, pr, inp) == z).all()


def test_application_host_generator_equals_the_full_generator_at_32():
    """zk_app_host_* (what zkhip_aggregator_witness_app runs on the host) at (32, 1), as
    tests/test_aggregator_host.py::test_application_host_generator_equals_the_full_generator does it at two proofs: everything it
    writes equals the full generator's assignment, the key's own sections stay zero"""
    from zecale_amd import zkhip
    lib = zkhip.load()
    lib.zk_app_host_new.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    lib.zk_app_host_witness.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    lib.zk_app_host_free.argtypes = [ctypes.c_void_p]
    agg = circuit_of(32, 1)
    st = ctypes.c_void_p()
    vk = np.ascontiguousarray(big_batch(32, 1)[0])
    assert lib.zk_app_host_new(agg.handle, vk.ctypes.data, ctypes.byref(st)) == 0
    for bumped in ((), bumped_proofs(32)):
        _, pr, inp, _ = big_batch(32, 1, bumped)
        pr, inp = np.ascontiguousarray(pr), np.ascontiguousarray(inp)
        z = agg.witness(vk, pr, inp)
        out = np.full_like(z, 0xFFFFFFFFFFFFFFFF)                     # (every entry must be written)
        h = np.ascontiguousarray(z[1])
        assert lib.zk_app_host_witness(agg.handle, st, vk.ctypes.data, pr.ctypes.data, inp.ctypes.data, None, 0, h.ctypes.data, out.ctypes.data) == 0
        differ = np.nonzero((out != z).any(axis=1))[0]
        assert len(differ) > 8000 and not out[differ].any()          # the key's own sections, left at zero
        assert differ.max() < len(z) // 16                            # ... which precede the 32 proof sections
        assert (out[:3] == z[:3]).all()
    lib.zk_app_host_free(st)


def test_tape_of_32_proofs_passes_the_program_validation():
    """the recorded program of (32, 1) through zkhip_internal_witness_run_program's host-side validation (batches = 0: no device)"""
    from zecale_amd import zkhip
    tape = circuit_of(32, 1).witness_tape()
    assert int(tape["chain_start"]) // 64 == 85716 and len(tape["level_start"]) - 1 == 15901
    z, flags = zkhip.witness_run_program(tape, np.zeros((0, int(tape["n_inputs"]), 6), dtype=np.uint64))
    assert z.shape[0] == 0 and len(flags) == 0
    z, flags = zkhip.witness_run_program(tape, np.zeros((0, int(tape["n_inputs"]), 6), dtype=np.uint64), waves=8)
    assert z.shape[0] == 0
    with pytest.raises(zkhip.ZkhipError) as e:
        zkhip.witness_run_program(tape, np.zeros((0, int(tape["n_inputs"]), 6), dtype=np.uint64), waves=3)
    assert e.value.code == -1


@pytest.mark.parametrize("n,k", [(32, 1), (32, 9), (2, 1)])
def test_plan_equals_the_counts_from_level_start(n, k):
    from zecale_amd import zkhip
    c = circuit_of(n, k)
    tape = c.witness_tape()
    ls = tape["level_start"]
    chunks, levels = int(tape["chain_start"]) // 64, len(ls) - 1
    assert int(ls[-1]) == int(tape["chain_start"])
    for w in (1, 4, 8, 16):
        plan = c.gpu_witness_plan(w)
        assert plan == dict(chunks=chunks, levels=levels, waves=w, steps=WW.steps(ls, w), value_bytes=64 * len(tape["code"])), (w, plan)
    assert c.gpu_witness_plan(1)["steps"] == chunks
    auto = c.gpu_witness_plan(0)
    assert auto["waves"] in (1, 2, 4, 8, 16) and auto["steps"] == WW.steps(ls, auto["waves"])
    if 2 * chunks < 3 * levels:                       # (a wide program may still get 1: the measured default decides)
        assert auto["waves"] == 1
    with pytest.raises(zkhip.ZkhipError) as e:
        c.gpu_witness_plan(3)
    assert e.value.code == -1


def test_plan_counts_of_the_issue_table():
    """the static counts the default width was reasoned from"""
    p = {w: circuit_of(32, 1).gpu_witness_plan(w) for w in (1, 4, 8, 16)}
    assert (p[1]["chunks"], p[1]["levels"]) == (85716, 15901)
    assert [p[w]["steps"] for w in (1, 4, 8, 16)] == [85716, 28903, 19837, 16928]
    q = {w: circuit_of(32, 9).gpu_witness_plan(w) for w in (1, 4, 8, 16)}
    assert (q[1]["chunks"], q[1]["levels"]) == (196415, 64641)
    assert [q[w]["steps"] for w in (1, 4, 8, 16)] == [196415, 88300, 72944, 66770]


@pytest.mark.parametrize("n,k", [(2, 1), (3, 1), (2, 9)])
def test_auto_stays_narrow_for_the_shapes_that_exist_today(n, k):
    c = circuit_of(n, k)
    plan = c.gpu_witness_plan(0)
    assert plan["waves"] == 1 and plan["steps"] == plan["chunks"]
    assert plan["chunks"] < 1.5 * plan["levels"]


def test_wide_generator_reaches_every_operand_source():
    """tests/witness_programs_wide.py keeps producing operands for the ring, for the load after the barrier and for the prefetch,
    levels of every width from 1 to 20 chunks, and the reference accepts its programs"""
    from tests import witness_programs as W
    for seed in (1, 2):
        prog = WW.wide_program(seed)
        assert set(WW.level_chunks(prog)) >= set(range(1, 21))
        ring, mem, pre = WW.operand_sources(prog)
        assert ring > 1000 and mem > 200 and pre > 1000, (ring, mem, pre)
        X = W.random_inputs(7, 1, 64)
        _, z, flag, bnd = W.interpret(prog, X[0])
        assert flag == 0 and max(bnd) <= W.CAP and len(z) == len(prog["code"])
        for seg in (1, 25, 41, len(prog["code"]) // 64):
            assert sum(WW.launches(prog, seg)) == len(prog["level_start"]) - 1
        assert set(WW.launches(prog, 1)) == {1}
        assert any(n > 1 and n % 2 for n in WW.launches(prog, 25) + WW.launches(prog, 41))


def test_pipeline_keeps_its_witness_work_space_under_a_quarter_of_the_device():
    """zkhip_internal_pipeline_witness_sizing, the arithmetic of a GPU-witness pipeline's constructor: witnesses per launch x batcher
    threads x value bytes <= a quarter of the device's memory, the batch halved first (rounding up), then batchers dropped; every
    shape up to sixteen proofs keeps sixteen per launch and its eight batchers on a 288 GB device"""
    from zecale_amd import zkhip
    lib = zkhip.load()
    fn = lib.zkhip_internal_pipeline_witness_sizing
    fn.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    fn.restype = ctypes.c_int

    def sized(value_bytes, mem, batch, workers):
        out = (ctypes.c_size_t * 2)()
        assert fn(value_bytes, mem, batch, workers, out) == 0
        return out[0], out[1]

    mem = 288 << 30
    values = {s: circuit_of(*s).gpu_witness_plan(1)["value_bytes"] for s in ((2, 1), (2, 9), (32, 1), (32, 9))}
    assert sized(values[(2, 1)], mem, 16, 8) == (16, 8) and sized(values[(2, 9)], mem, 16, 8) == (16, 8)
    assert sized(192 * 10**6, mem, 16, 8) == (16, 8)                    # (16, 1), the widest shape there was
    assert sized(values[(32, 1)], mem, 16, 8) == (16, 8)                # 45 GB of 77
    assert sized(values[(32, 9)], mem, 16, 8) == (8, 8)                 # 103 GB at sixteen: halved once
    assert sized(values[(32, 9)], mem, 5, 8) == (5, 8)                  # a batch the user set and that fits stays
    assert sized(values[(32, 9)], 64 << 30, 16, 8) == (2, 8)
    assert sized(values[(32, 9)], 64 << 30, 5, 8) == (2, 8)             # 5 -> 3 -> 2: halving rounds up
    assert sized(values[(32, 9)], 16 << 30, 16, 8) == (1, 5)            # one per launch, then fewer batchers
    assert sized(values[(32, 9)], 2 << 30, 16, 8) == (1, 1)             # never below one of each: the generator then fails by itself
    for b, w, m in ((16, 8, mem), (16, 8, 64 << 30), (7, 3, 16 << 30)):
        sb, sw = sized(values[(32, 9)], m, b, w)
        assert sb * sw * values[(32, 9)] <= m // 4 and 1 <= sb <= b and 1 <= sw <= w
    out = (ctypes.c_size_t * 2)()
    assert fn(0, mem, 16, 8, out) == -1 and fn(64, mem, 0, 8, out) == -1 and fn(64, mem, 16, 0, out) == -1
