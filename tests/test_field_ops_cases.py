"""The generator of tests/field_ops_cases.py itself (CPU only): the division-step model inverts, the inversion cases mix lanes of
different length where they claim to, and every op has the cases its tests count on."""
import random

import pytest

from tests import field_ops_cases as C


@pytest.mark.parametrize("name", list(C.FIELDS))
def test_divstep_model_inverts(name):
    """after n batches g = 0, f = +-1 and D a = 2^(29 n) f (mod p): f D / 2^(29 n) is the inverse pow() gives"""
    f = C.FIELDS[name]
    p = f.p
    rng = random.Random(41)
    vals = [1, 2, 3, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, f.Rdev % p] + [rng.randrange(1, p) for _ in range(60)]
    for a in vals:
        n, ff, D = C.inv_model(a, p)
        assert ff in (1, -1)
        assert (D * a - (ff << (C.B * n))) % p == 0
        assert ff * D * pow(2, -C.B * n, p) % p == pow(a, -1, p)
    assert C.inv_model(0, p) == (0, p, 0)


@pytest.mark.parametrize("name,seen", [("fq", {53, 54}), ("fr", {26, 27})])
def test_inversion_waves_mix_batch_counts(name, seen):
    f = C.FIELDS[name]
    inputs, waves, counts = C.inv_layout(name)
    assert len(inputs) == len(counts) == C.n_cases(name, "inv")
    nonzero = {c for v, c in zip(inputs, counts) if v % f.p}
    # 1. nonzero inputs show at least two distinct batch counts (a model run over 3000 random and 1500 structured inputs per field
    #    found exactly these two; no input that needs more is known)
    assert len(nonzero) >= 2 and nonzero == seen
    # 2. every wave that is meant to mix really holds lanes whose counts differ
    assert sum(w.mixed for w in waves) >= 4
    for w in waves:
        cs = set(counts[w.start:w.start + w.size])
        assert (len(cs) > 1) == w.mixed, w
        assert w.start % 64 == 0 and (w.size == 64 or w is waves[-1])
    # 3. the largest count stays below the loop's bound
    assert max(counts) < C.safegcd_batches(f.nbits)
    assert C.safegcd_batches(f.nbits) == {"fq": 62, "fr": 31}[name]
    kinds = [w.kind for w in waves]
    for k in ("one nonzero lane among 63 zeros", "one zero among 63 nonzeros", "two batch counts, lane by lane", "64 zeros",
              "64 copies of one value", "inputs in [p, 2p)", "a last wave of one lane"):
        assert k in kinds
    assert waves[-1].size == 1
    top = next(w for w in waves if w.kind == "inputs in [p, 2p)")
    tv = inputs[top.start:top.start + top.size]
    assert all(f.p <= v < 2 * f.p for v in tv) and f.p in tv and 2 * f.p - 1 in tv
    zeros = next(w for w in waves if w.kind == "64 zeros")
    assert inputs[zeros.start:zeros.start + 64] == [0] * 64


@pytest.mark.parametrize("name", list(C.FIELDS))
def test_every_op_has_its_edges(name):
    f = C.FIELDS[name]
    p = f.p
    assert set(C.ops_for(f)) <= set(C.OP_CODES) and len({C.OP_CODES[o] for o in C.ops_for(f)}) == len(C.ops_for(f))
    for op in C.ops_for(f):
        cs = C.cases(name, op)
        assert len(cs) == len(set(cs)) or op == "inv", op              # (the inversion repeats values on purpose)
        assert 300 <= len(cs) <= 4000, op
        for c in cs:
            C.precondition(f, op, c)
            ops = C.operands(f, op, c)
            assert all(len(o) == f.nl and all(0 <= x < 1 << 32 for x in o) for o in ops)
            if op not in C.WORD_OPS:
                assert all(x < 1 << C.B for o in ops for x in o[:-1])
    for op in [o for o in C.ops_for(f) if o.startswith("sub_") and o != "sub_sub2_8"]:
        kp = C._k_of(op) * p
        cs = C.cases(name, op)
        assert {0, 1, kp - 1, kp} <= {b for _, b, _ in cs}
        assert (f.lazy_max, kp, 0) in cs and (0, kp, 0) in cs and (0, 0, 0) in cs
        assert all(x == C.FULL for x in f.limbs(f.lazy_max)[:-1]) and f.lazy_max + f.S >= p << f.lazy_log
    assert any(b + 2 * c == 8 * p and b and c for _, b, c in C.cases(name, "sub_sub2_8"))
    for op in C.ops_for(f):
        if op in ("cond_sub_p", "canon_4p", "canon", "is_zero_2p") or op.startswith("cond_sub_kp_"):
            hi = C._fold_range(f, op)
            vals = {a for a, _, _ in C.cases(name, op)}
            assert {0, hi - 1} <= vals
            for m in range(hi // p + 1):
                assert {v for v in (m * p - 1, m * p, m * p + 1) if 0 <= v < hi} <= vals, (op, m)
    nb = 32 * f.n32
    for op in ("unpack_pack", "pack_unpack"):
        assert {1 << k for k in range(nb)} | {(1 << nb) - 1} <= {a for a, _, _ in C.cases(name, op)}
    assert max(a for a, _, _ in C.cases(name, "abi_roundtrip")) == (p << 10) - 1


def test_redc_is_the_montgomery_product():
    for f in C.FIELDS.values():
        rng = random.Random(3)
        for _ in range(50):
            x, y = rng.randrange(f.p << 5), rng.randrange(f.p << 5)
            v = f.redc(x * y)
            assert v * f.Rdev % f.p == x * y % f.p and v < x * y // f.Rdev + f.p + 1
