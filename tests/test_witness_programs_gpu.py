"""The GPU witness interpreter (zecale_amd/csrc/witness.hip: k_witness, k_witness_chain, k_witness_out) on programs of the tests'
own making and on full batches of the real ones.  Every comparison is EXACT - output limbs and flag words are equal.

The synthetic programs come from tests/witness_programs.py and are compared with its `interpret` (Python integers mod r, checked
against the host generator in tests/test_witness_programs.py).  They go through zkhip_internal_witness_run_program, which validates
a program on the host before it uploads anything and then runs the product's own witness_prog_upload and witness_launch; the
witnesses per workgroup (1, 2, 4: a 1,024-, 512- or 256-entry LDS ring per witness) and the chunks per launch are arguments, so
nothing here depends on ZKHIP_WITNESS_WPG / ZKHIP_WITNESS_SEGMENT or on the order of the tests.

  * bound extremes: the top of every range the tape builder's static bounds allow (sums at 2^12 r, the largest subtrahend of every
    a - b + 2^k r, inversions of 4r - 4 and of zeros that arrive as r, 2r, 3r, every bit) - real witness values are uniform field
    elements and never come near them;
  * addressing: operands on both sides of every boundary of ring and prefetch, for every ring size and segment length;
  * chain: the 64-entry ring of k_witness_chain, chain-only and levelled-only programs;
  * five batches per launch: at four witnesses per workgroup one full workgroup and one with a single live wave;
  * batch isolation: 1 .. 17 batches, then the same with one batch in the middle whose WT_INV meets zero.
The real programs (three circuit shapes and the application's program) run 5 and 16 batches per launch at every width."""
import numpy as np
import pytest

from tests import witness_programs as W
from tests.helpers import fr_limbs
from tests.test_witness_gpu import _batch

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4)
BATCHES = 5
_SMALL = {p["name"]: p for p in W.all_small_programs()}
_expected_cache = {}


def _expected(prog, key, X, i):
    k = (prog["name"], key, i)
    if k not in _expected_cache:
        _expected_cache[k] = W.expected(prog, X[i])
    return _expected_cache[k]


def _run_and_compare(zk, prog, key, X, wpg, seg):
    z, flags = zk.witness_run_program(prog, X, wpg, seg)
    assert z.shape == (len(X), len(prog["out_ref"]), 6) and flags.shape == (len(X),)
    for i in range(len(X)):
        want, flag = _expected(prog, key, X, i)
        if not (z[i] == want).all():
            pytest.fail("%s, %d per workgroup, segment %d, batch %d of %d: %r" % (prog["name"], wpg, seg, i, len(X), W.first_difference(prog, X[i], z[i])))
        assert int(flags[i]) == flag, "%s, %d per workgroup, segment %d: flag of batch %d is %d, expected %d" % (prog["name"], wpg, seg, i, int(flags[i]), flag)
    return z, flags


@pytest.mark.parametrize("wpg", WIDTHS)
@pytest.mark.parametrize("name", sorted(_SMALL))
def test_bound_extremes_and_chain_programs(zk, name, wpg):
    """every small program, five distinct input vectors (batch 0 feeds the largest device integer, r - 1, to input 0), in one launch
    per level's worth of chunks and in launches of three chunks"""
    prog = _SMALL[name]
    X = W.extreme_batches(prog, batches=BATCHES)
    assert len({x.tobytes() for x in X}) == BATCHES
    whole = max(1, int(prog["chain_start"]) // 64)
    _run_and_compare(zk, prog, "extreme", X, wpg, whole)
    if whole > 1:
        _run_and_compare(zk, prog, "extreme", X, wpg, 3)


_ADDRESSING = {seed: W.addressing_program(seed) for seed in (1, 2, 3)}


@pytest.mark.parametrize("wpg", WIDTHS)
@pytest.mark.parametrize("segment", ["1", "2", "3", "5", "7", "whole"])
@pytest.mark.parametrize("seed", sorted(_ADDRESSING))
def test_ring_and_prefetch_addressing(zk, seed, segment, wpg):
    """random levelled programs whose operands sit at the boundaries of ring and prefetch (every value is an assignment entry): segment
    lengths 1, 2, 3, 5, 7 make the segment start odd and even, the last segment short, and put operands before the segment start"""
    prog = _ADDRESSING[seed]
    seg = int(prog["chain_start"]) // 64 if segment == "whole" else int(segment)
    X = W.random_inputs(100 + seed, BATCHES, 64)
    _run_and_compare(zk, prog, "random", X, wpg, seg)


@pytest.mark.parametrize("wpg", WIDTHS)
def test_batches_do_not_see_each_other(zk, wpg):
    """1 .. 17 batches of one program with distinct inputs (empty waves in the last workgroup, a second and a fifth workgroup): every
    batch equals the reference; then the same with one batch in the middle whose input 0 is zero, which the program inverts with
    WT_INV: exactly that batch's flag is set and every other batch's values are what they were"""
    prog = W.addressing_program(4, inv_of_input0=True)
    assert int(prog["code"][64]) == W.WT_INV and int(prog["a"][64]) == 0
    X = W.random_inputs(204, 17, 64)
    for n in (1, 2, 3, 4, 5, 8, 16, 17):
        z, flags = _run_and_compare(zk, prog, "isolation", X[:n], wpg, 7)
        assert not flags.any()
        bad = n // 2
        Xb = X[:n].copy()
        Xb[bad, 0] = 0
        zb, fb = zk.witness_run_program(prog, Xb, wpg, 7)
        assert [int(f) for f in fb] == [1 if i == bad else 0 for i in range(n)], (n, list(fb))
        keep = [i for i in range(n) if i != bad]
        assert (zb[keep] == z[keep]).all()
        want, flag = W.expected(prog, Xb[bad])
        assert flag == 1 and (zb[bad] == want).all()              # the flagged batch's other values are still the program's


# ---------------------------------------------------------------------------------------------------------- the real programs
def _real_batches(num_proofs, k, n):
    """n distinct batches from the six fixture proofs: rotated, every third with a bumped input, later rounds with another last input;
    batch n // 2 carries a degenerate key (ABC_1 = ABC_0: the host generator branches where the recorded program cannot)"""
    out = []
    for i in range(n):
        vk, pr, inp = _batch(num_proofs, k, bump_last=(i % 3 == 1), first=i)
        inp = inp.copy()
        if i >= 6:
            inp[-1] = fr_limbs(0x5eed0000 + i)
        if i == n // 2:
            vk = vk.copy(); vk[72:84] = vk[60:72]
        out.append((vk, pr, inp))
    assert len({b[0].tobytes() + b[1].tobytes() + b[2].tobytes() for b in out}) == n
    return out


@pytest.mark.parametrize("n", [5, 16])
@pytest.mark.parametrize("num_proofs,k", [(2, 1), (3, 1), (2, 9)])
def test_real_programs_in_full_batches(zk, num_proofs, k, n):
    """zkhip_gpu_witness_run_batched on the generic program of three circuit shapes, 5 and 16 batches per launch (16 is the streaming
    prover's default), at every width, with the default segment and an odd one: each assignment equals the host generator's limb for
    limb, the degenerate batch alone is flagged, one assignment per configuration satisfies every constraint"""
    agg = zk.AggregatorCircuit(num_proofs, k)
    r1 = zk.r1cs_from_desc(zk.r1cs_desc_from_aggregator(agg))
    batches = _real_batches(num_proofs, k, n)
    deg = n // 2
    host = [None if i == deg else agg.witness(*b) for i, b in enumerate(batches)]
    l = agg.num_primary_inputs()
    for cfg, (wpg, seg) in enumerate((w, s) for w in WIDTHS for s in (None, 333)):
        z, flagged, prim = agg.witness_gpu_batched(batches, wpg=wpg, segment=seg)
        assert [bool(f) for f in flagged] == [i == deg for i in range(n)], (wpg, seg, list(flagged))
        for i in range(n):
            if i != deg:
                assert (z[i] == host[i]).all(), "%d per workgroup, segment %s, batch %d: first difference at variable %d" % (
                    wpg, seg, i, int(np.nonzero((z[i] != host[i]).any(axis=1))[0][0]))
                assert (prim[i] == host[i][1:1 + l]).all()
        pick = [i for i in range(n) if i != deg][cfg % (n - 1)]
        assert r1.is_satisfied(z[pick])
    r1.free(); agg.free()


def test_application_program_in_a_full_batch(zk):
    """the application's own program (its key folded in as constants, no chain), 16 batches per launch at every width and two segment
    lengths: the masked host generator's assignment limb for limb; unmasked, one per configuration satisfies every constraint"""
    from tests.test_aggregator_gpu import _setup
    agg, desc, kp, nvk_l, proofs = _setup(zk)
    crs, r1 = kp.upload_crs(), zk.r1cs_from_desc(desc)
    app = zk.AggregatorApp(agg, crs, nvk_l)
    pos, val, _, _ = app.constants()
    n = 16
    batches = []
    for i in range(n):
        _, pr, inp = _batch(2, 1, bump_last=(i % 3 == 1), first=i)
        inp = inp.copy()
        if i >= 6:
            inp[-1] = fr_limbs(0x5eed0000 + i)
        batches.append((nvk_l, pr, inp))
    host = [app.witness(b[1], b[2]) for b in batches]
    for cfg, (wpg, seg) in enumerate((w, s) for w in WIDTHS for s in (None, 333)):
        z, flagged, prim = agg.witness_gpu_batched(batches, wpg=wpg, segment=seg, app=app)
        assert not flagged.any()
        for i in range(n):
            assert (z[i] == host[i]).all(), "%d per workgroup, segment %s, batch %d" % (wpg, seg, i)
        full = z[cfg].copy()
        full[pos] = val
        assert (full == agg.witness(*batches[cfg])).all() and r1.is_satisfied(full)
    app.free(); crs.free(); r1.free(); kp.free(); agg.free()
