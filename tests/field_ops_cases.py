"""Cases and exact expectations for the field layer of zecale_amd/csrc/fp29.cuh and fp_inv.cuh on RAW limbs (test-side helpers, no GPU
needed to build them).  One generator and one reference serve the g++ build (tests/test_fp29_host.py) and the device build
(tests/test_field_ops_gpu.py, through zkhip_internal_field_ops_selftest); tests/test_field_ops_cases.py checks the generator itself.

A case is three operands (a, b, c) as Python integers.  Every operand of a limb op has normalised limbs (limbs 0 .. NL-2 below 2^29, the
top limb takes the rest), so its limbs are the base-2^29 digits of the integer; the word ops take the base-2^32 digits.  Each op's
documented precondition is ASSERTED on every case (precondition()): a case that breaks one is an error of this file, never skipped.

Expectations are exact integers, not residues.  The linear ops and the folds are exact by their contracts.  The ops that go through a
Montgomery multiplication are exact too: the reduction adds the one multiple m p, 0 <= m < R, that makes the low 29 NL bits vanish,
so fp_mul(x, y) = (x y + (-x y / p mod R) p) / R as an integer, whatever order the limbs are processed in (redc()).

The inversion cases are laid out by wave of 64 lanes (the device leaves its loop on a vote of the wave: a lane that is done keeps
running batches with g = 0 until the slowest lane is done).  inv_model() is an integer model of that loop - 29 division steps a batch,
zeta = -1 at the start, the batches counted until g = 0 - so that the generator KNOWS which waves mix lanes of different length."""
import functools
import random
from collections import namedtuple

from oracle import pyref as R

B = 29
FULL = (1 << B) - 1


class Field:
    def __init__(self, name, index, p, nl, n64, lazy_log, sub_k):
        self.name, self.index, self.p, self.nl, self.n64, self.n32 = name, index, p, nl, n64, 2 * n64
        self.nbits = p.bit_length()
        self.lazy_log = lazy_log              # operands of the linear ops go up to 2^lazy_log p
        self.sub_k = sub_k                    # the K of fp_sub_k<K> the tree instantiates for this field
        self.sh = B * (nl - 1)                # weight of the top limb
        self.S = 1 << self.sh
        self.Rdev = 1 << (B * nl)
        self.Rabi = 1 << (64 * n64)
        self.pinv = (-pow(p, -1, self.Rdev)) % self.Rdev
        self.lazy_max = self.below(p << lazy_log)

    def limbs(self, v):
        assert 0 <= v < 1 << (self.sh + 32), "does not fit NL limbs"
        return [(v >> (B * i)) & FULL for i in range(self.nl - 1)] + [v >> self.sh]

    def words(self, v):
        assert 0 <= v < 1 << (32 * self.n32)
        return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(self.n32)] + [0] * (self.nl - self.n32)

    def redc(self, t):
        """the Montgomery reduction of fp_mul / fp_sqr / fp_mul2 as an exact integer"""
        return (t + (t * self.pinv % self.Rdev) * self.p) >> (B * self.nl)

    def below(self, vmax, lower=None):
        """the largest value of a limb pattern that stays at or below vmax: the given lower limbs (default: all full) under the top limb
        of vmax less one"""
        top = (vmax >> self.sh) - 1
        assert top >= 0
        lower = [FULL] * (self.nl - 1) if lower is None else lower
        v = sum(x << (B * i) for i, x in enumerate(lower)) + (top << self.sh)
        assert v <= vmax
        return v

    def alt(self, vmax, phase):
        """alternating full and empty limbs (phase 0: the even limbs full), top limb as in below()"""
        return self.below(vmax, [FULL if i % 2 == phase else 0 for i in range(self.nl - 1)])


# fp_sub_k<K> call sites: Fq K = 1 (ec_edw.cuh), 32 (pairing.cuh); Fr K = 16, 64, 128 (pairing_bls.cuh) and, through fr2_sub<K> and
# nf_sub<K> (pairing_bls.cuh), 2, 4, 8, 16.  Lazy bounds: fp29.cuh states 2^10 p for the multipliers' operands; the witness tape lets
# an Fr operand reach 2^12 r (tests/test_field_gpu.py uses the same two bounds).
FQ = Field("fq", 0, R.Q_MOD, 27, 12, 10, (1, 32))
FR = Field("fr", 1, R.R_MOD, 14, 6, 12, (2, 4, 8, 16, 64, 128))
FIELDS = {"fq": FQ, "fr": FR}

# op codes of zkhip_internal_field_ops_selftest (include/zkhip.h); fp_sub_k<K> is 32 + log2 K
OP_CODES = {"add": 0, "dbl": 1, "sub_2": 2, "sub_4": 3, "sub_8": 4, "sub_16": 5, "sub_sub2_8": 6, "cond_sub_p": 7, "cond_sub_kp_1": 8,
            "cond_sub_kp_2": 9, "cond_sub_kp_4": 10, "cond_sub_kp_8": 11, "canon_4p": 12, "canon": 13, "is_zero_2p": 14, "unpack_pack": 15,
            "pack_unpack": 16, "abi_roundtrip": 17, "abi_to_canonical_words": 18, "inv": 19}
OP_CODES.update({"sub_k_%d" % (1 << i): 32 + i for i in range(8)})
WORD_OPS = ("unpack_pack", "abi_to_canonical_words")          # N32 words in operand a, N32 words out
N_RANDOM = 300


def ops_for(f):
    return [o for o in OP_CODES if not o.startswith("sub_k_")] + ["sub_k_%d" % k for k in f.sub_k]


def _k_of(op):
    return int(op.rsplit("_", 1)[1])


# ---------------------------------------------------------------- the inversion loop on integers
def safegcd_batches(nbits):
    """fp_inv.cuh: Pornin's bound on the division steps for an nbits modulus, in batches of 29, plus one spare batch"""
    return ((45907 * nbits + 26313) // 19929 + 29 + 28) // 29


def inv_model(a, p):
    """The loop of fp_inv on integers.  State (zeta, f, g) with f odd; a division step: if g is odd, add f to it - or, when zeta is
    negative, subtract f, let the old g become the new f and flip zeta to -zeta - 1; then zeta drops by one and g is halved.  The
    coefficients (D, E) follow without the division (D doubles where g halves), so after k steps 2^k f = D a and 2^k g = E a modulo p.
    A batch is 29 steps; the loop looks at g before each batch.  Returns (batches run until g = 0, f, D)."""
    f, g, D, E, zeta, n = p, a, 0, 1, -1, 0
    while g:
        for _ in range(B):
            if g & 1:
                if zeta < 0:
                    f, g, D, E, zeta = g, g - f, E, E - D, -zeta - 1
                else:
                    g, E = g + f, E + D
            zeta -= 1
            g >>= 1
            D <<= 1
        n += 1
    return n, f, D


InvWave = namedtuple("InvWave", "kind start size mixed")


def _inv_values(f):
    p = f.p
    step = max(1, f.nbits // 40)
    vals = [1, 2, 3, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, f.Rdev % p]
    vals += [1 << k for k in range(1, f.nbits, step)] + [p - (1 << k) for k in range(1, f.nbits - 1, step)]
    return vals


@functools.lru_cache(maxsize=None)
def inv_layout(name):
    """(inputs, waves, counts): the inputs of the inversion op in lane order, the waves they form, and each input's modelled batch
    count (of its canonical residue: fp_inv folds [0, 2p) to [0, p) first)."""
    f = FIELDS[name]
    p = f.p
    rng = random.Random(0x1177 + f.index)
    count = functools.lru_cache(maxsize=None)(lambda v: inv_model(v % p, p)[0])
    structured = _inv_values(f)
    randoms = [rng.randrange(1, p) for _ in range(N_RANDOM)]
    by_count = {}
    for v in structured + randoms:
        by_count.setdefault(count(v), []).append(v)
    classes = sorted(by_count, key=lambda c: -len(by_count[c]))
    assert len(classes) >= 2, "every nonzero input takes the same number of batches: no wave can mix lengths"
    inputs, waves = [], []

    def wave(kind, vals, mixed):
        assert len(inputs) % 64 == 0 and 1 <= len(vals) <= 64
        waves.append(InvWave(kind, len(inputs), len(vals), mixed))
        inputs.extend(vals)

    wave("one nonzero lane among 63 zeros", [0] * 17 + [randoms[0]] + [0] * 46, True)
    wave("one zero among 63 nonzeros", randoms[1:42] + [0] + randoms[42:64], True)
    la, lb = by_count[classes[0]], by_count[classes[1]]
    wave("two batch counts, lane by lane", [(la, lb)[i % 2][(i // 2) % len((la, lb)[i % 2])] for i in range(64)], True)
    wave("64 zeros", [0] * 64, False)
    wave("64 copies of one value", [randoms[64]] * 64, False)
    for i in range(0, len(structured), 64):
        chunk = structured[i:i + 64]
        chunk = chunk + randoms[65:65 + 64 - len(chunk)]
        wave("structured values", chunk, len({count(v) for v in chunk}) > 1)
    # a + p in [p, 2p): exactly p (lane 0), 2p - 1 (lane 63), the structured small values and randoms in between
    top = [p, p + 1, p + 2, p + 3, 2 * p - 2, p + (p + 1) // 2] + [p + v for v in randoms[130:187]] + [2 * p - 1]
    wave("inputs in [p, 2p)", top, True)
    for i in range(0, 256, 64):
        chunk = randoms[i:i + 64] if i + 64 <= len(randoms) else randoms[-64:]
        wave("random values", chunk, len({count(v) for v in chunk}) > 1)
    wave("a last wave of one lane", [randoms[7]], False)
    return inputs, waves, [count(v) for v in inputs]


# ---------------------------------------------------------------- cases
def _mix(f, rng, vmax):
    """a random value at or below vmax whose limbs are full, empty or random"""
    lower = [rng.choice([FULL, 0, rng.randrange(1 << B), rng.randrange(1 << B)]) for _ in range(f.nl - 1)]
    top = vmax >> f.sh
    v = sum(x << (B * i) for i, x in enumerate(lower)) + (rng.randrange(top) << f.sh if top else 0)
    return v if v <= vmax else rng.randrange(vmax + 1)


def _a_set(f):
    lazy = (f.p << f.lazy_log) - 1
    return [0, 1, f.lazy_max, f.alt(lazy, 0), f.alt(lazy, 1), f.S - 1]


def _around_multiples(f, hi):
    """m p - 1, m p, m p + 1 for every m with m p in [0, hi), as far as they lie in [0, hi), and both ends of the range"""
    out = []
    m = 0
    while m * f.p < hi:
        out += [v for v in (m * f.p - 1, m * f.p, m * f.p + 1) if 0 <= v < hi]
        m += 1
    out.append(hi - 1)
    return out


def _fold_range(f, op):
    """the stated input range [0, hi) of a fold or of the zero test"""
    if op in ("cond_sub_p", "is_zero_2p", "inv"):
        return 2 * f.p
    if op == "canon_4p":
        return 4 * f.p
    if op in ("canon", "abi_roundtrip"):
        return f.p << 10
    return 2 * _k_of(op) * f.p


@functools.lru_cache(maxsize=None)
def cases(name, op):
    """the cases of one op of one field, a tuple of (a, b, c); deterministic"""
    f = FIELDS[name]
    p = f.p
    rng = random.Random(1000 * f.index + OP_CODES[op])
    lazy = (p << f.lazy_log) - 1
    out = []
    if op in ("add", "dbl"):
        A = _a_set(f)
        out = [(a, b, 0) for a in A for b in (A if op == "add" else [0])]
        out += [(_mix(f, rng, lazy), _mix(f, rng, lazy) if op == "add" else 0, 0) for _ in range(N_RANDOM)]
    elif op.startswith("sub_") and op != "sub_sub2_8":
        kp = _k_of(op) * p
        Bs = [0, 1, kp - 1, kp, f.below(kp), f.alt(kp, 0), f.alt(kp, 1)]
        out = [(a, b, 0) for a in _a_set(f) for b in Bs]
        out += [(_mix(f, rng, lazy), _mix(f, rng, kp), 0) for _ in range(N_RANDOM)]
    elif op == "sub_sub2_8":
        kp = 8 * p
        T = (kp >> f.sh) - 3                     # tb + 2 tc = T with every lower limb full: b + 2c = (T + 3) S - 3 <= 8p
        assert T >= 1
        lower = f.S - 1
        BC = [(0, 0), (kp, 0), (0, 4 * p), (kp - 2, 1), (1, (kp - 1) // 2)]
        BC += [(kp - 2 * c, c) for c in (f.below(4 * p), f.alt(4 * p, 0), f.alt(4 * p, 1))]
        BC += [(kp - 2 * (b // 2), b // 2) for b in (f.alt(kp, 0), f.alt(kp, 1))]
        BC += [(lower + ((T - 2 * tc) << f.sh), lower + (tc << f.sh)) for tc in sorted({0, 1 if T >= 2 else 0, T // 2})]
        out = [(a, b, c) for a in _a_set(f) for b, c in BC]
        for _ in range(N_RANDOM):
            c = _mix(f, rng, 4 * p)
            out.append((_mix(f, rng, lazy), _mix(f, rng, kp - 2 * c), c))
    elif op in ("cond_sub_p", "canon_4p", "canon", "abi_roundtrip") or op.startswith("cond_sub_kp_"):
        hi = _fold_range(f, op)
        out = [(v, 0, 0) for v in _around_multiples(f, hi)]
        out += [(v, 0, 0) for v in (f.below(hi - 1), f.alt(hi - 1, 0), f.alt(hi - 1, 1))]
        if op == "abi_roundtrip":                # m p + x across the lazy range
            out += [(m * p + x, 0, 0) for m in (0, 1, 2, 3, 511, 1023) for x in (2, p // 2, p - 2, rng.randrange(p))]
        out += [(_mix(f, rng, hi - 1), 0, 0) for _ in range(N_RANDOM)]
    elif op == "is_zero_2p":
        hi = 2 * p
        vals = _around_multiples(f, hi)
        pl = f.limbs(p)
        for i in range(f.nl):                    # one limb away from 0 or from p, at every limb position that stays inside [0, 2p)
            w = 1 << (B * i)
            cand = [w, FULL * w if i < f.nl - 1 else None, p ^ w, p - pl[i] * w if pl[i] else None,
                    p + (FULL - pl[i]) * w if i < f.nl - 1 and pl[i] != FULL else None]
            vals += [v for v in cand if v is not None and v < hi]
        out = [(v, 0, 0) for v in vals] + [(_mix(f, rng, hi - 1), 0, 0) for _ in range(N_RANDOM)]
    elif op in ("unpack_pack", "pack_unpack"):
        nb = 32 * f.n32
        vals = [0, (1 << nb) - 1] + [1 << k for k in range(nb)]
        vals += [((1 << nb) - 1) & (FULL << (B * i)) for i in range(f.nl)]       # exactly one full limb (the top one as far as the words reach)
        vals += [((1 << nb) - 1) ^ (1 << k) for k in range(0, nb, 7)]
        vals += [rng.getrandbits(nb) for _ in range(N_RANDOM)]
        out = [(v, 0, 0) for v in vals]
    elif op == "abi_to_canonical_words":
        vals = [0, 1, 2, p - 1, p - 2, f.Rabi % p] + [1 << k for k in range(f.nbits - 1)] + [p - (1 << k) for k in range(0, f.nbits - 1, 5)]
        vals += [rng.randrange(p) for _ in range(N_RANDOM)]
        out = [(v, 0, 0) for v in vals]
    elif op == "inv":
        out = [(v, 0, 0) for v in inv_layout(name)[0]]
    else:
        raise KeyError(op)
    out = tuple(out) if op == "inv" else tuple(dict.fromkeys(out))          # (the inversion repeats values on purpose)
    for c in out:
        precondition(f, op, c)
    return out


def precondition(f, op, case):
    """the documented input contract of the op, on one case"""
    a, b, c = case
    p = f.p
    fits = lambda v: 0 <= v < 1 << (f.sh + 32)
    assert fits(a) and fits(b) and fits(c)
    if op in ("add", "dbl"):
        assert a < p << f.lazy_log and b < p << f.lazy_log
    elif op == "sub_sub2_8":
        assert a < p << f.lazy_log and b + 2 * c <= 8 * p and (8 * p >> f.sh) >= 4
    elif op.startswith("sub_"):
        assert a < p << f.lazy_log and b <= _k_of(op) * p and _k_of(op) * p < f.Rdev
        assert not op.startswith("sub_k_") or _k_of(op) in f.sub_k
    elif op in ("unpack_pack", "pack_unpack"):
        assert a < 1 << (32 * f.n32)
    elif op == "abi_to_canonical_words":
        assert a < p
    else:
        assert a < _fold_range(f, op)


def operands(f, op, case):
    """the three operands as NL 32-bit words each: limbs, or N32 packed words and padding for the word ops"""
    conv = f.words if op in WORD_OPS else f.limbs
    return [conv(case[0]), f.limbs(case[1]), f.limbs(case[2])]


def n_cases(name, op):
    return len(cases(name, op))


# ---------------------------------------------------------------- the reference
def expected(f, op, case):
    """(value, flag): the result as an exact integer - of its limbs, or of its N32 words for the word ops - and the flag word"""
    a, b, c = case
    p = f.p
    if op == "add":
        return a + b, 0
    if op == "dbl":
        return 2 * a, 0
    if op == "sub_sub2_8":
        return a - b - 2 * c + 8 * p, 0
    if op.startswith("sub_"):
        return a - b + _k_of(op) * p, 0
    if op == "cond_sub_p" or op.startswith("cond_sub_kp_"):
        kp = p if op == "cond_sub_p" else _k_of(op) * p
        return (a - kp if a >= kp else a), 0
    if op in ("canon_4p", "canon"):
        return a % p, 0
    if op == "is_zero_2p":
        return a, int(a in (0, p))
    if op in ("unpack_pack", "pack_unpack"):
        return a, 0
    if op == "abi_roundtrip":
        x = a * f.Rabi * pow(f.Rdev, -1, p) % p                                  # fp_to_abi: canonical, radix 2^(64 N64)
        return f.redc(x * (f.Rdev * f.Rdev * pow(f.Rabi, -1, p) % p)), 0        # fp_from_abi: one multiplication by R^2 / Rabi
    if op == "abi_to_canonical_words":
        return a * pow(f.Rabi, -1, p) % p, 0
    if op == "inv":
        r2 = f.Rdev * f.Rdev % p
        x = pow(a % p, -1, p) if a % p else 0
        return f.redc(f.redc(x * r2) * r2), 0
    raise KeyError(op)


def check(f, op, case, row):
    """one output row of the hook (NL words and the flag word) against the reference; raises AssertionError"""
    row = [int(x) for x in row]
    assert len(row) == f.nl + 1
    want, flag = expected(f, op, case)
    what = "%s %s case %s" % (f.name, op, tuple(hex(v) for v in case))
    if op in WORD_OPS:
        got = sum(w << (32 * j) for j, w in enumerate(row[:f.n32]))
        assert all(w == 0 for w in row[f.n32:f.nl]), what
    else:
        assert all(x < 1 << B for x in row[:f.nl - 1]), what + ": limbs not normalised"
        got = sum(x << (B * i) for i, x in enumerate(row[:f.nl]))
    assert got == want, what + ": got %#x, want %#x" % (got, want)
    assert row[f.nl] == flag, what + ": flag %d, want %d" % (row[f.nl], flag)
    if op == "inv":                              # the contract in its own terms, beside the exact value
        a = case[0]
        assert got < 2 * f.p, what
        assert got * a % f.p == (f.Rdev * f.Rdev % f.p if a % f.p else 0), what
        if a % f.p == 0:
            assert got == 0, what
    if op == "abi_roundtrip":
        assert got < 2 * f.p and got % f.p == case[0] % f.p, what
