"""Reference and program generators for the GPU witness interpreter (zecale_amd/csrc/witness.hip).  No GPU, no library call.

`interpret` is the instruction set of witness_tape.h on Python integers mod r, TRUE values (the device works on Montgomery residues
in 14 limbs of 29 bits, lazily reduced).  Beside every value it carries the static bound - a multiple of r - by the rules of
tools/sanitize/tape_check.cpp and asserts the value contract the device code relies on: no bound above 2^12, a subtrahend's bound at
most the 2^k of its WT_SUBK + k, an inversion's operand at most 4.  A generator that breaks the contract fails here, in Python, and
never reaches the device.  tests/test_witness_programs.py checks `interpret` against the host generator on the circuit's own tape.

`layout` turns a list of operations into the laid-out form (levels of one kind padded to whole 64-position chunks with WT_NOP, an
optional chain part in execution order, out_ref).  The generators are seeded and deterministic.

What "extreme" means on the device.  A value v is held as the integer v 2^406 mod r (plus a multiple of r when lazily reduced), so
the true value r - 1 is NOT the largest integer a slot can hold: dev(d) = d 2^-406 mod r is the true value whose device integer is
d.  The input pool therefore holds dev(r - 1) and dev(r - 2) next to r - 1 and r - 2: a doubling chain of dev(r - 1) reaches the
integer 4096 (r - 1), the top of the range the tape allows; a doubling chain of r - 1 reaches some other multiple.  Both run."""
import random

import numpy as np

from oracle import pyref as R

R_MOD = R.R_MOD
WT_NOP, WT_INPUT, WT_ADD, WT_SUB, WT_MUL, WT_INV, WT_INV0, WT_BIT, WT_RED, WT_SUBK = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16
CAP = 4096                      # witness_tape.cpp: no bound above 2^12 r
CHUNK = 64
RINGS = (256, 512, 1024)        # k_witness<4, 256>, <2, 512>, <1, 1024>
_MONT = pow(2, 384, R_MOD)      # the ABI's Montgomery factor
_MONT_INV = pow(_MONT, -1, R_MOD)
_DEV_INV = pow(pow(2, 406, R_MOD), -1, R_MOD)


class ContractError(AssertionError):
    """A program breaks the value contract of the device code (bounds of the lazy reduction)."""


def abi(v):
    """true value -> 6 ABI limbs (Montgomery form, canonical)"""
    x = v % R_MOD * _MONT % R_MOD
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def from_abi(limbs):
    return sum(int(w) << (64 * i) for i, w in enumerate(limbs)) * _MONT_INV % R_MOD


def dev(d):
    """the true value whose canonical device integer (v 2^406 mod r) is d"""
    return d % R_MOD * _DEV_INV % R_MOD


def binary(c):
    return c == WT_ADD or c == WT_MUL or c >= WT_SUBK


def klass(c):
    """the kind a level is made of (witness_tape.cpp): 2 inversions, 1 multiplications and bits, 0 the cheap rest"""
    return 2 if c in (WT_INV, WT_INV0) else 1 if c in (WT_MUL, WT_BIT) else 0


def interpret(prog, inputs):
    """One input vector ([n_inputs][6] ABI limbs) through `prog` -> (values per position (None at a WT_NOP), assignment as integers,
    flag, bounds per position).  Raises ContractError where the program breaks the value contract."""
    code, a, b = [int(x) for x in prog["code"]], [int(x) for x in prog["a"]], [int(x) for x in prog["b"]]
    consts = [from_abi(c) for c in np.asarray(prog["consts"]).reshape(-1, 6)]
    xin = [from_abi(x) for x in np.asarray(inputs).reshape(-1, 6)]
    if len(xin) != int(prog["n_inputs"]):
        raise ValueError("input vector of %d elements, the program takes %d" % (len(xin), int(prog["n_inputs"])))
    n = len(code)
    val, bnd, flag = [None] * n, [0] * n, 0

    def get(ref, p):
        if ref < 0:
            return consts[-1 - ref], 1
        if val[ref] is None or ref >= p:
            raise ContractError("position %d reads position %d, which is not defined before it" % (p, ref))
        return val[ref], bnd[ref]

    for p in range(n):
        c = code[p]
        if c == WT_NOP:
            continue
        if c == WT_INPUT:
            v, bd = xin[a[p]], 1
        else:
            x, bx = get(a[p], p)
            if binary(c):
                y, by = get(b[p], p)
            if c == WT_ADD:
                v, bd = (x + y) % R_MOD, bx + by
            elif c >= WT_SUBK:
                k = c - WT_SUBK
                if not 1 <= k <= 11:
                    raise ContractError("position %d: a - b + 2^%d r" % (p, k))
                if by > (1 << k):
                    raise ContractError("position %d: subtrahend bound %d above 2^%d" % (p, by, k))
                v, bd = (x - y) % R_MOD, bx + (1 << k)
            elif c == WT_RED:
                v, bd = x, 3
            elif c == WT_MUL:
                v, bd = x * y % R_MOD, 2
            elif c == WT_INV or c == WT_INV0:
                if bx > 4:
                    raise ContractError("position %d: inversion of a value bounded by %d r" % (p, bx))
                if x == 0 and c == WT_INV:
                    flag = 1
                v, bd = (pow(x, -1, R_MOD) if x else 0), 2
            elif c == WT_BIT:
                if not 0 <= b[p] < 384:
                    raise ContractError("position %d: bit %d" % (p, b[p]))
                v, bd = (x >> b[p]) & 1, 1
            else:
                raise ContractError("position %d: code %d" % (p, c))
        if bd > CAP:
            raise ContractError("position %d: bound %d r" % (p, bd))
        val[p], bnd[p] = v, bd
    z = []
    for ref in prog["out_ref"]:
        ref = int(ref)
        z.append(consts[-1 - ref] if ref < 0 else val[ref])
        if z[-1] is None:
            raise ContractError("assignment entry reads position %d, a no-op" % ref)
    return val, z, flag, bnd


def expected(prog, inputs):
    """-> (u64 [n_vars, 6] as k_witness_out writes them, flag word) for one input vector"""
    _, z, flag, _ = interpret(prog, inputs)
    return np.array([abi(v) for v in z], dtype=np.uint64).reshape(-1, 6), flag


def first_difference(prog, inputs, got):
    """the first wrong POSITION of a run, for a failure message: (position, code, a, b, want, got) or None"""
    want, _ = expected(prog, inputs)
    bad = np.nonzero((want != np.asarray(got)).any(axis=1))[0]
    if not len(bad):
        return None
    i = int(bad[0])
    ref = int(prog["out_ref"][i])
    return dict(entry=i, position=ref, code=int(prog["code"][ref]) if ref >= 0 else None, a=int(prog["a"][ref]) if ref >= 0 else None,
                b=int(prog["b"][ref]) if ref >= 0 else None, want=hex(from_abi(want[i])), got=hex(from_abi(got[i])))


# ------------------------------------------------------------------------------------------------------------------------ layout
def layout(ops, chain=(), consts=(), n_inputs=0, outs=None, name=""):
    """ops: the levelled part, a list of (level, code, a, b); chain: the chain part in execution order, a list of (code, a, b).
    An operand >= 0 is an INDEX into ops + chain, < 0 the constant -1 - index (`consts`: true values).  Operations of one level
    number are grouped by kind, each group a level of its own padded to whole chunks.  outs: the indices the assignment reads
    (default: every operation, then every constant) - so every value a program computes is compared."""
    order = sorted(range(len(ops)), key=lambda i: (ops[i][0], klass(ops[i][1])))
    code, a, b, level_start, pos_of, prev = [], [], [], [0], {}, None

    def pad():
        while len(code) % CHUNK:
            code.append(WT_NOP); a.append(0); b.append(0)

    for i in order:
        key = (ops[i][0], klass(ops[i][1]))
        if prev is not None and key != prev:
            pad()
            level_start.append(len(code))
        prev = key
        pos_of[i] = len(code)
        code.append(ops[i][1]); a.append(ops[i][2]); b.append(ops[i][3])
    if ops:
        pad()
        level_start.append(len(code))
    chain_start = len(code)
    for j, (c, ra, rb) in enumerate(chain):
        pos_of[len(ops) + j] = len(code)
        code.append(c); a.append(ra); b.append(rb)
    for p, c in enumerate(code):
        if c in (WT_NOP, WT_INPUT):
            continue
        if a[p] >= 0:
            a[p] = pos_of[a[p]]
        if binary(c) and b[p] >= 0:
            b[p] = pos_of[b[p]]
    if outs is None:
        out_ref = [pos_of[i] for i in range(len(ops) + len(chain))] + [-1 - i for i in range(len(consts))]
    else:
        out_ref = [pos_of[i] if i >= 0 else i for i in outs]
    return dict(name=name, code=np.array(code, dtype=np.uint8), a=np.array(a, dtype=np.int32), b=np.array(b, dtype=np.int32),
                level_start=np.array(level_start, dtype=np.uint32), chain_start=chain_start, out_ref=np.array(out_ref, dtype=np.int32),
                consts=np.array([abi(v) for v in consts], dtype=np.uint64).reshape(-1, 6), n_inputs=n_inputs)


class _B:
    """a program written operation by operation; every operation gets the level after its operands' (so a level per step)"""

    def __init__(self, n_inputs, consts=()):
        self.ops, self.lvl, self.consts, self.n_inputs = [], [], list(consts), n_inputs
        self.inp = [self._emit(0, WT_INPUT, i, 0) for i in range(n_inputs)]

    def _emit(self, level, c, a, b):
        self.ops.append((level, c, a, b)); self.lvl.append(level)
        return len(self.ops) - 1

    def const(self, v):
        if v % R_MOD not in [c % R_MOD for c in self.consts]:
            self.consts.append(v % R_MOD)
        return -1 - [c % R_MOD for c in self.consts].index(v % R_MOD)

    def op(self, c, a, b=0):
        l = 1 + max([self.lvl[r] for r in ([a, b] if binary(c) else [a]) if r >= 0] + [-1])
        return self._emit(l, c, a, b)

    def add(self, a, b): return self.op(WT_ADD, a, b)
    def subk(self, k, a, b): return self.op(WT_SUBK + k, a, b)

    def double_to(self, x, bound, start=1):
        """x + x + ... : the operation whose bound is `bound` (x has bound `start`), and the chain up to it"""
        out, bd = [x], start
        while bd < bound:
            out.append(self.add(out[-1], out[-1])); bd *= 2
        assert bd == bound
        return out

    def done(self, name):
        return layout(self.ops, consts=self.consts, n_inputs=self.n_inputs, name=name)


def input_pool(seed, n):
    """n values: the fixed extremes first, then random ones"""
    rng = random.Random(seed)
    fixed = [dev(R_MOD - 1), R_MOD - 1, 0, 1, dev(R_MOD - 2), 2, R_MOD - 2, (R_MOD + 1) // 2, (R_MOD - 1) // 2, dev(1)]
    return (fixed + [rng.randrange(R_MOD) for _ in range(max(0, n - len(fixed)))])[:n]


def extreme_batches(prog, seed=1, batches=5):
    """`batches` DISTINCT input vectors for a bound-extremes program: batch i takes its inputs from the pool, rotated by i - so
    batch 0 feeds dev(r - 1), the largest device integer, to input 0, batch 1 the true value r - 1, batch 2 zero."""
    n = int(prog["n_inputs"])
    pool = input_pool(seed, 10 + batches)
    return np.array([[abi(pool[(i + 3 * j) % len(pool)]) for j in range(n)] for i in range(batches)], dtype=np.uint64).reshape(batches, n, 6)


# ------------------------------------------------------------------------------------------------------- bound extremes
def bound_extreme_programs():
    """One small program per case; every operation is an assignment entry.  Input 0 is `x`."""
    progs = []
    # doubling chains up to the cap, then one reader of the 4096 r value (2048 r for the minuend: 2048 + 2^11 = 4096 is the cap)
    for tail in ("red", "mul", "bit", "subk11"):
        B = _B(1)
        d = B.double_to(B.inp[0], CAP)
        if tail == "red":
            for v in d:
                B.op(WT_RED, v)
        elif tail == "mul":
            B.op(WT_MUL, d[-1], d[-1]); B.op(WT_MUL, d[-1], d[0]); B.op(WT_MUL, B.const(R_MOD - 1), d[-1]); B.op(WT_MUL, d[-1], d[-2])
        elif tail == "bit":
            for bit in (0, 1, 28, 29, 63, 64, 375, 376, 377, 383):
                B.op(WT_BIT, d[-1], bit)
        else:
            B.subk(11, d[-2], d[-2]); B.subk(11, d[-2], B.const(0)); B.subk(11, B.const(0), d[-2]); B.subk(11, d[-2], d[0])
        progs.append(B.done("double_to_cap_" + tail))
    # constants take the other way into a slot (k_witness_consts): the same chain from the constants r - 1 and dev(r - 1)
    B = _B(1)
    for cv in (R_MOD - 1, dev(R_MOD - 1)):
        c = B.const(cv)
        d = B.double_to(B.add(c, c), CAP, start=2)
        B.op(WT_RED, d[-1]); B.op(WT_MUL, d[-1], d[-1]); B.op(WT_BIT, d[-1], 376); B.subk(11, d[-2], d[-2])
    progs.append(B.done("double_constants_to_cap"))
    # 0 - b + 2^k r with the largest subtrahend k admits, and with b = 0
    for k in range(1, 12):
        B = _B(1)
        zero = B.const(0)
        b = B.double_to(B.inp[0], 1 << k)[-1]
        B.subk(k, zero, b); B.subk(k, zero, zero); B.subk(k, B.inp[0], b); B.subk(k, b, b) if (2 << k) <= CAP else None
        bc = B.double_to(B.add(B.const(dev(R_MOD - 1)), B.const(dev(R_MOD - 1))), 1 << k, start=2)[-1]
        B.subk(k, zero, bc)
        progs.append(B.done("subk_%d_largest_subtrahend" % k))
    # inversions: operands of bound 1 .. 4 with value 1, -1, -4, dev(-1) summed (the largest integer an inversion sees), x; and zeros
    for c in (WT_INV0, WT_INV):
        B = _B(1)
        x = B.inp[0]
        for v in (1, R_MOD - 1, R_MOD - 4, dev(R_MOD - 1)):
            B.op(c, B.const(v))                                                 # bound 1
        B.op(c, B.op(WT_MUL, B.const(R_MOD - 1), B.const(1)))                   # -1 at bound 2
        B.op(c, B.op(WT_RED, B.const(R_MOD - 4)))                               # -4 at bound 3
        for q in (pow(4, -1, R_MOD), R_MOD - pow(4, -1, R_MOD), R_MOD - 1, dev(R_MOD - 1)):      # 1, -1, -4, 4 dev(-1) at bound 4
            h = B.add(B.const(q), B.const(q))
            B.op(c, h); B.op(c, B.add(h, h))
        B.op(c, x); B.op(c, B.add(x, x)); B.op(c, B.add(B.add(x, x), B.add(x, x)))
        progs.append(B.done("inverse_bounds_1_to_4_" + ("inv0" if c == WT_INV0 else "inv")))
        # zeros in lazy dress: x - x + 2r (the integer 2r), (r - 1) + 1 (r), r + r (2r), r - 0 + 2r (3r), WT_RED of k r
        B = _B(1)
        x = B.inp[0]
        z_r = B.add(B.const(R_MOD - 1), B.const(1))                            # integer r, bound 2
        z_2r = B.subk(1, x, x)                                                  # integer 2r, bound 3
        B.op(c, z_r); B.op(c, z_2r); B.op(c, B.add(z_r, z_r)); B.op(c, B.subk(1, z_r, B.const(0))); B.op(c, B.const(0))
        kr = B.double_to(z_r, CAP, start=2)                                     # r, 2r, 4r .. 2048 r
        for v in kr:
            B.op(c, B.op(WT_RED, v))
        for i, j in ((0, 1), (1, 2), (2, 3), (0, 3), (4, 6), (9, 10), (0, 10)):      # 3r, 6r, 12r, 9r, 80r, 1536r, 1025r
            B.op(c, B.op(WT_RED, B.add(kr[i], kr[j])))
        progs.append(B.done("inverse_of_lazy_zeros_" + ("inv0" if c == WT_INV0 else "inv")))
    # every bit of r - 1, 2^376, x, and of a zero that arrives as the integer r
    B = _B(1)
    z_r = B.add(B.const(R_MOD - 1), B.const(1))
    for src in (B.const(R_MOD - 1), B.const(1 << 376), B.inp[0], z_r):
        for bit in range(384):
            B.op(WT_BIT, src, bit)
    progs.append(B.done("every_bit"))
    # a constant on either side, on both, and a == b
    B = _B(2)
    x, y, c1, c2 = B.inp[0], B.inp[1], B.const(R_MOD - 1), B.const(dev(R_MOD - 1))
    for c in (WT_ADD, WT_MUL, WT_SUBK + 1, WT_SUBK + 7):
        for l, r_ in ((c1, x), (x, c1), (c1, c2), (c2, c2), (x, x), (x, y), (y, x)):
            B.op(c, l, r_)
    progs.append(B.done("constant_operands"))
    return progs


# ------------------------------------------------------------------------------------------------------------- addressing
def _lin(rng, ba, bb):
    """a cheap operation on operands of bounds ba, bb that keeps the contract: (code, unary)"""
    choice = rng.random()
    k = max(1, (bb - 1).bit_length())
    if choice < 0.45 and ba + bb <= CAP:
        return WT_ADD, False
    if choice < 0.9 and k <= 11 and ba + (1 << k) <= CAP:
        ks = [kk for kk in range(k, 12) if ba + (1 << kk) <= CAP]
        return WT_SUBK + (ks[0] if rng.random() < 0.7 else rng.choice(ks)), False
    return WT_RED, True


def addressing_program(seed, n_positions=3200, inv_of_input0=False):
    """A random levelled DAG, every position filled (index = position), levels 1 .. 5 chunks wide, each of one kind.  Operand
    distances come mostly from where the kernel changes its source: for each ring size RING - 65 .. RING + 65 back from the END of
    the reading chunk (ring_lo: the ring on one side, the chunk-ahead prefetch on the other), the previous level, the start of the
    reader's segment for segment lengths 1, 2, 3, 5, 7, and position 0.  inv_of_input0: position 64 is WT_INV of input 0 (the
    flag of the batch-isolation test)."""
    rng = random.Random(seed)
    n_inputs = 64
    ops, bnd = [(0, WT_INPUT, i, 0) for i in range(n_inputs)], [1] * n_inputs
    level, prev_start = 0, 0
    while len(ops) < n_positions:
        level += 1
        start, width = len(ops), rng.randint(1, 5) * CHUNK
        kind = rng.choices((0, 1, 2), weights=(6, 3, 1))[0]
        if inv_of_input0 and level == 1:
            kind, width = 2, CHUNK

        def pick(p, want_small=False):
            end = (p // CHUNK + 1) * CHUNK
            u = rng.random()
            if u < 0.55:
                ref = end - rng.choice(RINGS) + rng.randint(-65, 65)
            elif u < 0.70:
                ref = rng.randrange(prev_start, start)
            elif u < 0.80:
                seg = rng.choice((1, 2, 3, 5, 7))
                ref = (p // CHUNK) // seg * seg * CHUNK + rng.randint(-66, 2)
            elif u < 0.85:
                ref = 0
            else:
                ref = rng.randrange(start)
            if not 0 <= ref < start:
                ref = rng.randrange(prev_start, start) if rng.random() < 0.5 else rng.randrange(start)
            if want_small:                      # an inversion's operand: bound at most 4 - the nearest such position at or below
                while bnd[ref] > 4:
                    ref -= 1                    # (inputs have bound 1: terminates)
            return ref

        for p in range(start, start + width):
            if kind == 2:
                if inv_of_input0 and p == start:
                    ops.append((level, WT_INV, 0, 0))
                else:
                    ops.append((level, WT_INV0, pick(p, True), 0))
                bnd.append(2)
            elif kind == 1:
                if rng.random() < 0.8:
                    ops.append((level, WT_MUL, pick(p), pick(p))); bnd.append(2)
                else:
                    ops.append((level, WT_BIT, pick(p), rng.randrange(384))); bnd.append(1)
            else:
                a, b = pick(p), pick(p)
                if rng.random() < 0.1:
                    b = a
                c, unary = _lin(rng, bnd[a], bnd[b])
                ops.append((level, c, a, 0 if unary else b))
                bnd.append(3 if c == WT_RED else bnd[a] + bnd[b] if c == WT_ADD else bnd[a] + (1 << (c - WT_SUBK)))
        prev_start = start
    prog = layout(ops, n_inputs=n_inputs, name="addressing_%d" % seed)
    assert all(int(prog["code"][p]) == ops[p][1] for p in range(len(ops))) and len(prog["code"]) == len(ops)      # index = position
    return prog


def random_inputs(seed, batches, n_inputs):
    rng = random.Random(seed)
    return np.array([[abi(rng.randrange(1, R_MOD)) for _ in range(n_inputs)] for _ in range(batches)], dtype=np.uint64).reshape(batches, n_inputs, 6)


def segment_lengths(prog):
    """1, 2, 3, 5, 7 chunks and the whole levelled part in one launch"""
    return [1, 2, 3, 5, 7, max(1, int(prog["chain_start"]) // CHUNK)]


# ------------------------------------------------------------------------------------------------------------------ chain
def chain_ops(rng, length, base, n_inputs):
    """`length` chain operations whose indices start at `base`: the chain's own copies of the inputs first, then operations whose
    operands lie 1, 63, 64, 65 entries back (the 64-entry ring test) or at the chain's first entry"""
    out, bnd = [], []
    for i in range(length):
        if i < n_inputs:
            out.append((WT_INPUT, i, 0)); bnd.append(1)
            continue

        def pick():
            d = rng.choice((1, 1, 63, 64, 65, i, rng.randint(1, i)))
            return i - d if d <= i else 0
        a, b = pick(), pick()
        u = rng.random()
        if u < 0.2:
            c, b, bd = WT_MUL, b, 2
        elif u < 0.27:
            c, b, bd = WT_BIT, rng.randrange(384), 1
        elif u < 0.33 and bnd[a] <= 4:
            c, b, bd = WT_INV0, 0, 2
        else:
            c, unary = _lin(rng, bnd[a], bnd[b])
            bd = 3 if c == WT_RED else bnd[a] + bnd[b] if c == WT_ADD else bnd[a] + (1 << (c - WT_SUBK))
            b = 0 if unary else b
        out.append((c, base + a, base + b if binary(c) else b)); bnd.append(bd)
    return out


def chain_programs(seed=5):
    """chain only (chain_start = 0), levelled only (chain_start = n_pos), and both; chain lengths 1, 63, 64, 65, 200"""
    rng = random.Random(seed)
    progs = []
    for length in (1, 63, 64, 65, 200):
        progs.append(layout([], chain=chain_ops(rng, length, 0, 1), n_inputs=2, name="chain_only_%d" % length))
    lev = [(0, WT_INPUT, i, 0) for i in range(2)] + [(1, WT_MUL, 0, 1), (1, WT_MUL, 1, 1), (2, WT_ADD, 2, 3), (2, WT_SUBK + 2, 3, 2), (3, WT_INV0, 4, 0)]
    progs.append(layout(lev, n_inputs=2, name="levelled_only"))
    for length in (1, 63, 64, 65, 200):
        progs.append(layout(lev, chain=chain_ops(rng, length, len(lev), 2), n_inputs=2, name="levelled_and_chain_%d" % length))
    return progs


def all_small_programs():
    return bound_extreme_programs() + chain_programs()
