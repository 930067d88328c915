"""WIDE synthetic programs for k_witness_wide (zecale_amd/csrc/witness.hip): levels of 1 .. 20 chunks, so that the waves of a workgroup
share a level, read what OTHER waves wrote in the level before, and levels wider than the LDS ring (1,012 entries, less than 16
chunks) exist.  No GPU, no library call; the reference is tests/witness_programs.interpret, which also checks the value contract.

Where the wide kernel changes the source of an operand (k_witness_wide's comment): an operand of the level before the reader's comes
from the ring when it lies within WIDE_RING positions of the END of the reader's level, from memory after the barrier otherwise;
anything older is prefetched from memory.  Operand distances are therefore drawn around (end of the reader's level - WIDE_RING), from
every chunk of the previous level, from two and more levels back, from the first position of levels (where launches are cut) and
from position 0."""
import random

from tests import witness_programs as W

CHUNK = W.CHUNK
WIDE_RING = 1012            # witness.hip: 1024 - WT_SUBK_LEVELS
WAVES = (2, 4, 8, 16)


def wide_program(seed, n_levels=34, max_width=20, inv_of_input0=False):
    """A random levelled DAG, every position filled (index = position).  Level 0: 64 inputs; level 1 (inv_of_input0): one chunk of
    inversions whose first is WT_INV of input 0; then levels of 1 .. max_width chunks, every width from 1 to max_width at least once,
    of one kind each.  Every instruction kind occurs (asserted)."""
    rng = random.Random(seed)
    n_inputs = 64
    ops, bnd = [(0, W.WT_INPUT, i, 0) for i in range(n_inputs)], [1] * n_inputs
    starts = [0]                      # first index of every level so far
    widths = list(range(1, max_width + 1)) + [rng.randint(1, max_width) for _ in range(max(0, n_levels - max_width))]
    rng.shuffle(widths)
    kinds = [0, 1, 2] * (len(widths) // 3 + 1)
    rng.shuffle(kinds)
    for level, width_chunks in enumerate(widths, start=1):
        start, width = len(ops), width_chunks * CHUNK
        kind = kinds[level]
        if inv_of_input0 and level == 1:
            kind, width = 2, CHUNK
        end, prev_start = start + width, starts[-1]

        def pick(want_small=False):
            u = rng.random()
            if u < 0.30:                                       # the ring's lower edge, seen from the end of the reader's level
                ref = end - WIDE_RING + rng.randint(-70, 70)
            elif u < 0.60:                                     # the level before: any chunk of it, whichever wave wrote it
                ref = rng.randrange(prev_start, start)
            elif u < 0.75 and len(starts) >= 2:                # two and more levels back, at a level's first / last positions or inside
                s = rng.randrange(len(starts) - 1)
                ref = rng.choice((starts[s], starts[s + 1] - 1, rng.randrange(starts[s], starts[s + 1])))
            elif u < 0.80:
                ref = 0
            else:
                ref = rng.randrange(start)
            if not 0 <= ref < start:
                ref = rng.randrange(prev_start, start)
            if want_small:
                while bnd[ref] > 4:
                    ref -= 1                                   # (inputs have bound 1: terminates)
            return ref

        for p in range(start, end):
            if kind == 2:
                if inv_of_input0 and p == start and level == 1:
                    ops.append((level, W.WT_INV, 0, 0))
                else:
                    ops.append((level, W.WT_INV0, pick(True), 0))
                bnd.append(2)
            elif kind == 1:
                if rng.random() < 0.8:
                    ops.append((level, W.WT_MUL, pick(), pick())); bnd.append(2)
                else:
                    ops.append((level, W.WT_BIT, pick(), rng.randrange(384))); bnd.append(1)
            else:
                a, b = pick(), pick()
                if rng.random() < 0.1:
                    b = a
                c, unary = W._lin(rng, bnd[a], bnd[b])
                ops.append((level, c, a, 0 if unary else b))
                bnd.append(3 if c == W.WT_RED else bnd[a] + bnd[b] if c == W.WT_ADD else bnd[a] + (1 << (c - W.WT_SUBK)))
        starts.append(start)
    prog = W.layout(ops, n_inputs=n_inputs, name="wide_%d%s" % (seed, "_inv" if inv_of_input0 else ""))
    assert all(int(prog["code"][p]) == ops[p][1] for p in range(len(ops))) and len(prog["code"]) == len(ops)      # index = position
    codes = set(int(c) for c in prog["code"])
    assert {W.WT_INPUT, W.WT_ADD, W.WT_MUL, W.WT_INV0, W.WT_BIT, W.WT_RED} <= codes and any(c >= W.WT_SUBK for c in codes)
    assert not inv_of_input0 or W.WT_INV in codes
    return prog


def level_chunks(prog):
    """chunks of every level"""
    ls = [int(x) for x in prog["level_start"]]
    return [(ls[i + 1] - ls[i]) // CHUNK for i in range(len(ls) - 1)]


def launches(prog, seg):
    """the levels per launch of the wide kernels for segment length `seg` (witness_launch: whole levels, the first boundary at which
    the launch holds seg chunks or more)"""
    out, n, c = [], 0, 0
    for w in level_chunks(prog):
        n, c = n + 1, c + w
        if c >= seg:
            out.append(n); n, c = 0, 0
    if n:
        out.append(n)
    return out


def steps(level_start, waves):
    """sum over levels of ceil(chunks of the level / waves)"""
    ls = [int(x) for x in level_start]
    return sum(-(-((ls[i + 1] - ls[i]) // CHUNK) // waves) for i in range(len(ls) - 1))


def operand_sources(prog):
    """how many operands the wide kernel takes from (the ring, memory after the barrier, the prefetch) when every launch runs the
    whole program: a generator that stops producing one of the three no longer tests that path"""
    ls = [int(x) for x in prog["level_start"]]
    ring = mem = pre = 0
    for l in range(len(ls) - 1):
        plim = ls[l - 1] if l else 0
        ring_lo = max(0, ls[l + 1] - WIDE_RING)
        for p in range(ls[l], ls[l + 1]):
            c = int(prog["code"][p])
            if c in (W.WT_NOP, W.WT_INPUT):
                continue
            for q in ([int(prog["a"][p]), int(prog["b"][p])] if W.binary(c) else [int(prog["a"][p])]):
                if q < 0 or q < plim:
                    pre += 1
                elif q >= ring_lo:
                    ring += 1
                else:
                    mem += 1
    return ring, mem, pre
