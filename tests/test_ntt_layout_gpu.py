"""The transform passes in DEVICE LAYOUT (zkhip_internal_ntt_packed -> ntt_dev_packed_batch), as the QAP map drives them and
zkhip_ntt does not: input on the transposed side, up to three vectors per launch, lazily reduced operands up to the contract's 8 r,
and the wide tiles behind ZKHIP_NTT_ONE_EACH_MAX.  The hook permutes nothing: all layout knowledge is in tests/ntt_layout.py.
Input is placed on the side `in_transposed` names and the output is read from the other side.  The reference is the CPU oracle
(pinned on the golden vectors) or a closed form in Python integers; every comparison is exact - limb for limb for ABI limbs, the
residue mod r for packed device words."""
import functools

import numpy as np
import pytest

from oracle import pyref as R
from tests.helpers import fr_array, random_fr_canonical, random_fr_uniform
from tests.ntt_layout import abi_ints, from_packed, from_transposed, layout_logk, packed_raw, to_packed, to_transposed

pytestmark = pytest.mark.gpu

# (inverse, coset, input transposed): everything but the forward coset transform of transposed input, which the engine refuses
KINDS = [(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1)]
MODES = [(0, 0), (1, 0), (0, 1), (1, 1)]
KIND_ID = lambda k: ("i" if k[0] else "") + ("coset" if k[1] else "") + "fft-" + ("t2n" if k[2] else "n2t")

_inputs, _expected = {}, {}


def _input(log_d, seed):
    """one random vector per (size, seed), uniform in [0, r); made once, never written"""
    key = (log_d, seed)
    if key not in _inputs:
        for k in [k for k in _inputs if k[0] != log_d]:      # (one size at a time: a 2^20 vector is 48 MiB)
            del _inputs[k]
        a = random_fr_uniform(seed, 1 << log_d)
        a.setflags(write=False)
        _inputs[key] = a
    return _inputs[key]


def _oracle(oracle_lib, log_d, seed, inv, coset):
    """the oracle's transform of _input(log_d, seed), natural order; shared by the kinds (both input sides) and tests of one size"""
    key = (log_d, seed, inv, coset)
    if key not in _expected:
        for k in [k for k in _expected if k[0] != log_d]:
            del _expected[k]
        e = oracle_lib.ntt(_input(log_d, seed), log_d, inverse=bool(inv), coset=bool(coset))
        e.setflags(write=False)
        _expected[key] = e
    return _expected[key]


def _run(zk, vecs, log_d, kind):
    """vecs: natural-order arrays [d, 6] (ABI limbs) or [d, 12] (device words) -> the transforms in natural order, [nbuf, d, .]"""
    inv, coset, in_t = kind
    dev = np.stack([to_transposed(v, log_d) if in_t else np.asarray(v) for v in vecs])
    out = zk.ntt_packed(dev, log_d, inverse=inv, coset=coset, in_transposed=in_t)
    return np.stack([o if in_t else from_transposed(o, log_d) for o in out])


# ---- all seven kinds against the oracle, three different vectors per launch ---------------------------------------------------------
@pytest.mark.parametrize("log_d,kind", [(n, k) for n in (12, 13, 14, 15, 18, 19) for k in KINDS], ids=lambda v: KIND_ID(v) if isinstance(v, tuple) else str(v))
def test_seven_kinds_three_vectors_vs_oracle(zk, oracle_lib, log_d, kind):
    """12, 13: the smallest two-pass shapes, equal and unequal factors; 14, 15: LOGK 7 and 8; 18, 19: LOGK 9 and 10.  Each output is
    compared with the transform of ITS OWN input: a vector that was not picked, or picked twice, fails."""
    seeds = [1000 + 10 * log_d + v for v in range(3)]
    got = _run(zk, [_input(log_d, s) for s in seeds], log_d, kind)
    for v, s in enumerate(seeds):
        assert (got[v] == _oracle(oracle_lib, log_d, s, kind[0], kind[1])).all(), (log_d, KIND_ID(kind), "vector", v)


def test_forward_coset_of_transposed_input_is_refused(zk):
    import ctypes
    log_d = 12
    a = np.stack([_input(log_d, 1120)]).copy()
    before = a.copy()
    lib = zk.load()
    lib.zkhip_internal_ntt_packed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    assert lib.zkhip_internal_ntt_packed(a.ctypes.data, 0, 1, log_d, 0, 1, 1) == -1            # ZKHIP_ERR_ARG
    assert b"natural order" in lib.zkhip_last_error()
    assert (a == before).all()
    for bad in ((2, 1, log_d, 0, 0, 0), (0, 0, log_d, 0, 0, 0), (0, 4, log_d, 0, 0, 0), (0, 1, 23, 0, 0, 0), (0, 1, log_d, 2, 0, 0), (0, 1, log_d, 0, 0, 2)):
        assert lib.zkhip_internal_ntt_packed(a.ctypes.data, *bad) == -1, bad
        assert (a == before).all()
    assert lib.zkhip_internal_ntt_packed(None, 0, 1, log_d, 0, 0, 0) == -1
    assert lib.zkhip_internal_ntt_set_one_each_max(23) == -1 and lib.zkhip_internal_ntt_set_one_each_max(-2) == -1


# ---- one-tile sizes in batches ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_d", [0, 1, 2, 5, 8, 11])
def test_one_tile_sizes_in_batches(zk, oracle_lib, log_d):
    """below 2^12 a vector is in natural order on both sides: in_transposed is accepted and ignored"""
    assert layout_logk(log_d) == 0
    seeds = [2000 + 10 * log_d + v for v in range(3)]
    a = np.stack([_input(log_d, s) for s in seeds])
    for inv, coset in MODES:
        got = zk.ntt_packed(a, log_d, inverse=inv, coset=coset, in_transposed=0)
        for v, s in enumerate(seeds):
            assert (got[v] == _oracle(oracle_lib, log_d, s, inv, coset)).all(), (log_d, inv, coset, "vector", v)
        assert (zk.ntt_packed(a, log_d, inverse=inv, coset=coset, in_transposed=1) == got).all(), (log_d, inv, coset)


# ---- the input contract at its edge -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _lazy_case(log_d, top=7):
    """three vectors of x uniform below r as packed device words: x + top r everywhere; x + m r, m in 0 .. top per element (an
    operand of 0 r beside one of 7 r is what the first stage's subtraction must survive); x alone"""
    d = 1 << log_d
    seeds = [3000 + 10 * log_d + v for v in range(3)]
    xs = [abi_ints(_input(log_d, s)) for s in seeds]                              # the values the ABI limbs stand for
    ms = np.random.RandomState(3000 + log_d).randint(0, top + 1, size=d)
    if d <= 4:                                                                     # too few draws to leave the widest gaps to chance:
        ms[:] = [0, top] if d == 2 else [0, 0, top, top]                           # the first butterflies (elements 0 - 2 and 1 - 3 of four) subtract top r from 0 r
    words = [to_packed(xs[0], top), to_packed(xs[1], ms.tolist()), to_packed(xs[2], 0)]
    for w in words:
        w.setflags(write=False)
    return seeds, words


def _stored_below(log_d, kind, B=8):
    """The multiple of r every stored output of `kind` stays below for inputs below B r, from the bounds of the arithmetic alone
    (ntt.hip, 'What each producer of a transform's input stores').  A store that ends in a product is below 2 r: the inverse coset
    kind and the one-tile inverse kinds.  The plain two-pass inverse does NOT end in one (its 1 / d is folded into pass 1's table),
    nor does a forward kind: L plain stages on an input below b r (b <= 8) leave less than (2 b + 12 + 2 L) r - the first radix-4
    round 2 b + 16, every later stage 2 more - and the second pass of a two-pass kind starts from pass 1's products, b = 2.  The
    one-tile forward coset transform multiplies in its first stage too: B + 2 L."""
    inv, coset, in_t = kind
    lk = layout_logk(log_d)
    if lk == 0:
        return 2 if inv else (B + 2 * log_d if coset else 2 * B + 12 + 2 * log_d)
    if inv and coset:
        return 2
    L = lk if in_t else log_d - lk                           # the last pass: the columns (size K) for transposed input, else the rows
    return 2 * 2 + 12 + 2 * L


@pytest.mark.parametrize("log_d,kind", [(n, (i, c, 0)) for n in (1, 2, 11) for i, c in MODES] + [(n, k) for n in (12, 13) for k in KINDS],
                         ids=lambda v: KIND_ID(v) if isinstance(v, tuple) else str(v))
def test_lazily_reduced_input_up_to_8r(zk, oracle_lib, log_d, kind):
    """'Inputs < 8r' (ntt.hip): operands carry up to 7 r on top of a value below r.  The outputs, as stored, are congruent mod r to
    the oracle's transform of the residues, and below the producer bound: 2 r where the last pass ends in a multiplication, the
    growth bound of the stages where it does not (_stored_below)."""
    seeds, words = _lazy_case(log_d)
    got = _run(zk, words, log_d, kind)
    assert got.dtype == np.uint32
    for v, s in enumerate(seeds):
        assert from_packed(got[v]) == abi_ints(_oracle(oracle_lib, log_d, s, kind[0], kind[1])), (log_d, KIND_ID(kind), "vector", v)
        assert max(packed_raw(got[v])) < _stored_below(log_d, kind) * R.R_MOD, (log_d, KIND_ID(kind), "vector", v)


@pytest.mark.parametrize("log_d", [2, 11, 12, 13])
def test_forward_coset_takes_inputs_up_to_64r(zk, oracle_lib, log_d):
    """The forward coset transform reads what the plain two-pass inverse stores - up to 38 r, not the 8 r of the other kinds; its first
    stage multiplies the subtrahend, and ntt.hip gives it 64 r.  Operands of x + 63 r; then the QAP map's own chain on the device
    words as they are: iFFT (transposed -> natural) of the 8 r vectors, its output straight into the cosetFFT (natural -> transposed)."""
    kind = (0, 1, 0)
    seeds, words = _lazy_case(log_d, 63)
    got = _run(zk, words, log_d, kind)
    for v, s in enumerate(seeds):
        assert from_packed(got[v]) == abi_ints(_oracle(oracle_lib, log_d, s, 0, 1)), (log_d, "vector", v)
        assert max(packed_raw(got[v])) < _stored_below(log_d, kind, 64) * R.R_MOD, (log_d, "vector", v)
    seeds, words = _lazy_case(log_d)
    in_t = 1 if layout_logk(log_d) else 0
    dev = np.stack([to_transposed(w, log_d) for w in words])
    mid = zk.ntt_packed(dev, log_d, inverse=1, coset=0, in_transposed=in_t)                   # natural order, never reduced
    out = zk.ntt_packed(mid, log_d, inverse=0, coset=1, in_transposed=0)
    for v, s in enumerate(seeds):
        exp = oracle_lib.ntt(_oracle(oracle_lib, log_d, s, 1, 0), log_d, coset=True)
        assert from_packed(from_transposed(out[v], log_d)) == abi_ints(exp), (log_d, "chain, vector", v)


# ---- closed forms, independent of the oracle ----------------------------------------------------------------------------------------
G = R.FR_GENERATOR


def _powers(base, n, first=1):
    out, acc = [], first % R.R_MOD
    for _ in range(n):
        out.append(acc)
        acc = acc * base % R.R_MOD
    return out


def _expected_of_delta(log_d, j, inv, coset):
    """transform of the vector with a one at index j (running products)"""
    d = 1 << log_d
    w = R.fr_root_of_unity(log_d)
    if not inv:
        return _powers(pow(w, j, R.R_MOD), d, pow(G, j, R.R_MOD) if coset else 1)              # g^j w^(jk)
    winv, ginv, dinv = pow(w, -1, R.R_MOD), pow(G, -1, R.R_MOD), pow(d, -1, R.R_MOD)
    return _powers(pow(winv, j, R.R_MOD) * (ginv if coset else 1) % R.R_MOD, d, dinv)          # w^(-jk) / d, times g^-k


def _expected_of_ones(log_d, inv, coset):
    d = 1 << log_d
    if inv:
        return [1] + [0] * (d - 1)                                                             # d delta_0 / d (g^-0 = 1)
    if not coset:
        return [d] + [0] * (d - 1)
    w, gd = R.fr_root_of_unity(log_d), pow(G, d, R.R_MOD)                                      # sum_j (g w^k)^j = (g^d - 1) / (g w^k - 1)
    return [(gd - 1) * pow(gw - 1, -1, R.R_MOD) % R.R_MOD for gw in _powers(w, d, G)]


@pytest.mark.parametrize("log_d,kind", [(n, k) for n in (12, 13) for k in KINDS], ids=lambda v: KIND_ID(v) if isinstance(v, tuple) else str(v))
def test_closed_forms(zk, log_d, kind):
    """a one at index j in {1, K - 1, K, N2, d - 1} gives w^(jk) (times g^j on the coset; the inverse kinds w^(-jk) / d, times g^-k);
    the constant vector gives d delta_0"""
    inv, coset, _ = kind
    d = 1 << log_d
    K = 1 << layout_logk(log_d)
    N2 = d // K
    js = sorted({1, K - 1, K, N2, d - 1})
    one, zero = fr_array([1])[0], np.zeros((d, 6), dtype=np.uint64)
    vecs, exps = [], []
    for j in js:
        v = zero.copy()
        v[j] = one
        vecs.append(v)
        exps.append(_expected_of_delta(log_d, j, inv, coset))
    vecs.append(np.tile(one, (d, 1)))
    exps.append(_expected_of_ones(log_d, inv, coset))
    for lo in range(0, len(vecs), 3):
        got = _run(zk, vecs[lo:lo + 3], log_d, kind)
        for v in range(got.shape[0]):
            what = "ones" if lo + v == len(js) else "delta at %d" % js[lo + v]
            assert (got[v] == fr_array(exps[lo + v])).all(), (log_d, KIND_ID(kind), what)


# ---- the wide tiles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_d,kind", [(n, k) for n in (19, 20) for k in KINDS], ids=lambda v: KIND_ID(v) if isinstance(v, tuple) else str(v))
def test_wide_tiles(zk, oracle_lib, log_d, kind):
    """one-each up to 2^18 only: 2^19 runs k_ntt_pass<10, 1> on the columns and <9, 2> on the rows, 2^20 runs <10, 1> twice.  The
    same call with the default choice gives the identical array: results do not depend on the knob."""
    seed = 4000 + log_d
    a = [_input(log_d, seed)]
    zk.ntt_set_one_each_max(18)
    try:
        wide = _run(zk, a, log_d, kind)
    finally:
        zk.ntt_set_one_each_max(-1)
    assert (wide[0] == _oracle(oracle_lib, log_d, seed, kind[0], kind[1])).all(), (log_d, KIND_ID(kind))
    assert (_run(zk, a, log_d, kind) == wide).all(), (log_d, KIND_ID(kind))


# ---- full tiles (2^11-point sub-transforms), transposed input -----------------------------------------------------------------------
ROUND_TRIPS = {"fft-ifft": ((0, 0, 0), (1, 0, 1)), "cosetfft-icosetfft": ((0, 1, 0), (1, 1, 1)), "ifft-fft": ((1, 0, 0), (0, 0, 1))}


@pytest.mark.parametrize("log_d,trip", [(n, t) for n in (21, 22) for t in ROUND_TRIPS])
def test_full_tile_round_trips(zk, log_d, trip):
    """natural -> transposed, then its inverse transposed -> natural, returns the input (the oracle is too slow at 2^22)"""
    a = random_fr_canonical(5000 + log_d, 1 << log_d)[None]
    (i0, c0, t0), (i1, c1, t1) = ROUND_TRIPS[trip]
    mid = zk.ntt_packed(a, log_d, inverse=i0, coset=c0, in_transposed=t0)          # left in transposed order: the next call's input
    assert (zk.ntt_packed(mid, log_d, inverse=i1, coset=c1, in_transposed=t1) == a).all(), (log_d, trip)


def test_log_d_21_transposed_vs_oracle(zk, oracle_lib):
    log_d = 21
    a = random_fr_canonical(5000 + log_d, 1 << log_d)
    got = _run(zk, [a], log_d, (1, 1, 1))
    assert (got[0] == oracle_lib.ntt(a, log_d, inverse=True, coset=True)).all()
