"""CPU half of the witness interpreter's tests (no GPU): the test hook refuses every program that breaks a structural rule BEFORE
anything could be uploaded (validate-only calls: zero batches, no device); every generated program keeps the value contract that
tests/witness_programs.interpret asserts; and `interpret` - the reference of tests/test_witness_programs_gpu.py - reproduces the
host generator's assignment limb for limb on the circuit's own exported tape, which is what entitles it to be the reference."""
import numpy as np
import pytest

from tests import witness_programs as W
from zecale_amd import zkhip as zk


def _validate(prog, wpg=4, segment=1):
    z, flags = zk.witness_run_program(prog, np.zeros((0, int(prog["n_inputs"]), 6), dtype=np.uint64), wpg, segment)
    assert z.shape[0] == 0 and len(flags) == 0


def _mutated(prog, **changes):
    """a copy of `prog` with single entries replaced: code={position: value}, ..."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in prog.items()}
    for field, edits in changes.items():
        if isinstance(edits, dict):
            for i, v in edits.items():
                out[field][i] = v
        else:
            out[field] = edits
    return out


@pytest.fixture(scope="module")
def base():
    """levelled_and_chain_65: inputs at 0, 1; MULs at 64, 65; ADD / SUBK at 128, 129; INV0 at 192; the chain from 256"""
    prog = [p for p in W.chain_programs() if p["name"] == "levelled_and_chain_65"][0]
    code = prog["code"]
    assert prog["chain_start"] == 256 and len(code) == 321 and list(prog["level_start"]) == [0, 64, 128, 192, 256]
    assert (code[64], code[65], code[128], code[129], code[192], code[256], code[66]) == (W.WT_MUL, W.WT_MUL, W.WT_ADD, W.WT_SUBK + 2, W.WT_INV0, W.WT_INPUT, W.WT_NOP)
    assert code[300] != W.WT_NOP and code[300] != W.WT_INPUT
    return prog


REFUSED = {
    "level_not_whole_chunks": dict(level_start={1: 32}),
    "levels_do_not_end_at_chain_start": dict(level_start={4: 192}),
    "level_starts_decrease": dict(level_start={2: 192, 3: 128}),
    "chain_start_inside_a_chunk": dict(chain_start=250),
    "chain_start_past_the_end": dict(chain_start=384),
    "levelled_operand_in_its_own_level": dict(a={65: 64}),
    "levelled_operand_b_in_its_own_level": dict(b={129: 128}),
    "levelled_operand_in_a_later_level": dict(a={64: 128}),
    "levelled_operand_is_itself": dict(b={128: 128}),
    "levelled_operand_in_the_chain": dict(a={128: 256}),
    "levelled_operand_past_the_end": dict(a={128: 1 << 20}),
    "operand_is_a_no_op_slot": dict(a={128: 66}),
    "chain_operand_in_the_levelled_part": dict(a={300: 192}),
    "chain_operand_is_itself": dict(a={300: 300}),
    "chain_operand_later_in_the_chain": dict(a={300: 301}),
    "chain_operand_past_the_end": dict(a={300: 321}),
    "constant_index_out_of_range": dict(code={128: W.WT_ADD}, a={128: -1}),                   # (this program has no constants)
    "constant_index_most_negative": dict(a={128: -(1 << 31)}),
    "input_index_out_of_range": dict(a={1: 2}),
    "input_index_negative": dict(a={256: -1}),
    "out_ref_past_the_end": dict(out_ref={0: 321}),
    "out_ref_constant_out_of_range": dict(out_ref={0: -1}),
    "out_ref_reads_a_no_op_slot": dict(out_ref={0: 66}),
    "bit_index_384": dict(code={128: W.WT_BIT}, b={128: 384}),
    "bit_index_negative": dict(code={128: W.WT_BIT}, b={128: -1}),
    "subk_with_k_0": dict(code={129: W.WT_SUBK}),
    "subk_with_k_12": dict(code={129: W.WT_SUBK + 12}),
    "subk_with_k_239": dict(code={129: 255}),
    "plain_sub": dict(code={129: W.WT_SUB}),
    "unknown_code_9": dict(code={128: 9}),
    "unknown_code_15": dict(code={300: 15}),
}


def test_the_hook_accepts_every_generated_program_without_a_device():
    for prog in W.all_small_programs() + [W.addressing_program(1), W.addressing_program(2, inv_of_input0=True)]:
        for wpg in (1, 2, 4):
            _validate(prog, wpg, 1)


@pytest.mark.parametrize("rule", sorted(REFUSED))
def test_the_hook_refuses_a_program_that_breaks_a_structural_rule(base, rule):
    _validate(base)
    with pytest.raises(zk.ZkhipError) as e:
        _validate(_mutated(base, **REFUSED[rule]))
    assert e.value.code == -1, e.value                      # ZKHIP_ERR_ARG, from the host-side validation


def test_the_hook_refuses_widths_and_segments_outside_their_range(base):
    for wpg, seg in ((3, 1), (0, 1), (8, 1), (4, 0), (4, (1 << 20) + 1)):
        with pytest.raises(zk.ZkhipError) as e:
            _validate(base, wpg, seg)
        assert e.value.code == -1
    empty = dict(base, code=base["code"][:0], a=base["a"][:0], b=base["b"][:0], level_start=np.zeros(1, dtype=np.uint32), chain_start=0)
    with pytest.raises(zk.ZkhipError):
        _validate(empty)


def test_every_generated_program_keeps_the_value_contract():
    """interpret raises ContractError for a bound above 2^12, a subtrahend above its 2^k or an inversion operand above 4: every
    program of every generator runs clean on its own inputs, and the bound extremes really are at the extremes."""
    top = 0
    for prog in W.bound_extreme_programs():
        for x in W.extreme_batches(prog):
            _, _, _, bnd = W.interpret(prog, x)
        top = max(top, max(bnd))
        if prog["name"].startswith("double_to_cap"):
            assert max(bnd) == W.CAP
    assert top == W.CAP
    for prog in W.chain_programs():
        for x in W.extreme_batches(prog):
            W.interpret(prog, x)
    for seed, flagged in ((1, False), (2, False), (3, False), (4, True)):
        prog = W.addressing_program(seed, inv_of_input0=flagged)
        x = W.random_inputs(seed, 2, 64)
        _, _, flag, bnd = W.interpret(prog, x[0])
        assert flag == 0 and max(bnd) > 1024            # sums pile up to the cap's neighbourhood before a WT_RED brings them down
        if flagged:
            x[1, 0] = 0
            assert W.interpret(prog, x[1])[2] == 1


def test_addressing_programs_put_operands_on_both_sides_of_every_ring_boundary():
    """the point of the addressing family: for each ring size, operands at every distance RING - 64 .. RING + 64 from the end of
    the reading chunk occur (the kernel's ring_lo switches between ring and prefetch inside that window), for readers in odd and
    even chunks; and some operand precedes the start of the reader's segment for every segment length"""
    prog = W.addressing_program(1)
    code, a, b = prog["code"], prog["a"], prog["b"]
    seen = {ring: set() for ring in W.RINGS}
    before_segment = {seg: 0 for seg in (1, 2, 3, 5, 7)}
    for p in range(len(code)):
        refs = [int(a[p])] if code[p] not in (W.WT_NOP, W.WT_INPUT) else []
        if W.binary(int(code[p])):
            refs.append(int(b[p]))
        for ref in refs:
            d = (p // 64 + 1) * 64 - ref
            for ring in W.RINGS:
                if abs(d - ring) <= 64:
                    seen[ring].add((d - ring, (p // 64) % 2))
            for seg in before_segment:
                before_segment[seg] += ref < (p // 64) // seg * seg * 64
    for ring in W.RINGS:
        assert {d for d, _ in seen[ring]} == set(range(-64, 65)), (ring, sorted(set(range(-64, 65)) - {d for d, _ in seen[ring]}))
        assert {par for _, par in seen[ring]} == {0, 1}
        assert (0, 0) in seen[ring] or (0, 1) in seen[ring]                   # the boundary itself: the oldest entry the ring still holds
        assert (1, 0) in seen[ring] or (1, 1) in seen[ring]                   # and the newest the prefetch must fetch
    assert all(n > 50 for n in before_segment.values()), before_segment


def test_interpret_equals_the_host_generator_on_the_exported_tape():
    """zkhip_internal_witness_tape gives the batch-2 program exactly as the GPU generator uploads it; interpret on it reproduces
    zkhip_aggregator_witness limb for limb, on the valid fixture batch and on the bumped one; and the hook's validation accepts it."""
    import bench
    nvk_l, npr, nin, _ = bench.aggregator_inputs()
    agg = zk.AggregatorCircuit(2, 1)
    prog = agg.witness_tape()
    assert len(prog["out_ref"]) == agg.num_variables and prog["n_inputs"] == 32 and prog["chain_start"] % 64 == 0
    assert len(prog["code"]) > 100000 and prog["chain_start"] < len(prog["code"])
    _validate(prog, 4, 2048)
    bumped = nin.copy()
    bumped[1][0] += 1
    for inputs in (nin, bumped):
        x = np.concatenate([nvk_l, npr, inputs.reshape(-1)]).astype(np.uint64).reshape(-1, 6)
        want = agg.witness(nvk_l, npr, inputs)
        got, flag = W.expected(prog, x)
        assert flag == 0
        assert (got == want).all(), "first difference at variable %d" % int(np.nonzero((got != want).any(axis=1))[0][0])
    assert (agg.witness(nvk_l, npr, nin) != agg.witness(nvk_l, npr, bumped)).any()
    agg.free()
