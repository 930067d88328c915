"""The rare branches of the bucket-method MSM against closed forms, bit for bit: same-x additions (P + P, P + (-P)), runs, pieces
and rows that cancel to infinity and reopen, signed digits on the edges of their range and carries through every window.

Inputs come from tests/msm_cases.py: bases from {O, +-G, +-2G, +-3G} (every base a known multiple k_i G, built by the C oracle),
so every result is (sum s_i k_i mod r) G - one oracle scalar multiplication at any n - and structures that force the branches
whatever order the bucket sort leaves inside a bucket.  Paths: plain handles at c in {4, auto, 12, 18} (at c = 18, 2^14 terms put
the row sums over 65,536 outputs: the one-lane k_sum_lds), forced batched-affine levels (PK_DBL / PK_INF), both kinds of window
table up to c = 22, G2, the 2^20 table-backed stream of the headline, and the five merged MSMs of the prover (k_accumulate<5>) with
and without the streaming geometry."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import msm_cases as M
from tests.helpers import csr_from_rows, fr_array, fr_ints, fr_limbs, make_r1cs, random_fr_uniform

pytestmark = pytest.mark.gpu

POOL = M.scalar_pool((4, 9, 12, 16, 18, 22))
SIZES = (1, 2, 3, 257, 1025, 5000, 1 << 14)


def _run_structures(zk, O, n, c, make_handle, g2=False, seed=0, structures=M.STRUCTURES):
    """Every structure at n terms through a handle from make_handle(bases); scalars as canonical integers and as Montgomery
    residues.  Returns nothing; asserts the closed form."""
    for j, st in enumerate(structures):
        ks, scal = M.make_case(st, n, POOL, seed=seed * 97 + j * 7 + n, c=c or 9)
        bases = M.bases_of(O, ks, g2)
        exp = M.closed_form(O, ks, scal, g2)
        b = make_handle(bases)
        try:
            got_can = zk.jac_to_affine(b.msm(M.canonical_limbs(scal), montgomery=False))
            got_mont = zk.jac_to_affine(b.msm(M.montgomery_limbs(scal), montgomery=True))
        finally:
            b.free()
        assert (got_can == exp).all(), (st, n, c, "canonical")
        assert (got_mont == exp).all(), (st, n, c, "montgomery")
        if n <= 257:
            assert (O.jac_to_affine(O.msm(bases, M.montgomery_limbs(scal))) == exp).all()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", [4, 0, 12, 18], ids=["c4", "auto", "c12", "c18"])
def test_plain_handles(zk, oracle_lib, c, n):
    _run_structures(zk, oracle_lib, n, c, lambda bases: zk.Bases.upload(bases).set_window(c), seed=1)


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("n", (2, 3, 257, 1025))
@pytest.mark.parametrize("c", [4, 0, 12], ids=["c4", "auto", "c12"])
def test_plain_handles_forced_affine_levels(zk, oracle_lib, c, n, levels):
    """Batched-affine levels in front of the XYZZ accumulation: pairs with the same x take pair_kind_same_x (PK_DBL, PK_INF)."""
    zk.set_affine_levels(levels)
    try:
        _run_structures(zk, oracle_lib, n, c, lambda bases: zk.Bases.upload(bases).set_window(c), seed=2)
    finally:
        zk.set_affine_levels(-1)


@pytest.mark.parametrize("n", (3, 1025, 5000))
@pytest.mark.parametrize("naf,c", [(False, 4), (False, 9), (False, 16), (False, 22), (True, 4), (True, 9), (True, 16)],
                         ids=["win4", "win9", "win16", "win22", "naf4", "naf9", "naf16"])
def test_window_tables(zk, oracle_lib, naf, c, n):
    def handle(bases):
        b = zk.Bases.upload(bases).precompute(c, table_naf=naf)
        assert b.table_window == c
        return b
    _run_structures(zk, oracle_lib, n, c, handle, seed=3)


@pytest.mark.parametrize("kind", ["plain_auto", "table_win9"])
def test_g2(zk, oracle_lib, kind):
    if kind == "plain_auto":
        handle, c = (lambda bases: zk.Bases.upload(bases).set_window(0)), 0
    else:
        handle, c = (lambda bases: zk.Bases.upload(bases).precompute(9, table_naf=False)), 9
    for n in (3, 1025, 5000):
        _run_structures(zk, oracle_lib, n, c, handle, g2=True, seed=4)


def test_headline_2_20_stream_with_colliding_bases(zk, oracle_lib):
    """The headline path (2^20 bases with their window table, MsmStream): k_fixup_fold and the one-lane reduction under same-x
    additions everywhere - the bases are O and +-G, +-2G, +-3G tiled at random, the scalars uniform in [0, r) with a tenth of them
    from the adversarial pool, sent as canonical integers; checked by one scalar multiplication (and a second for a sub-range)."""
    O = oracle_lib
    n = 1 << 20
    rng = np.random.default_rng(20)
    kidx = rng.integers(0, len(M.SMALL_KS), n)
    ks = [M.SMALL_KS[i] for i in kidx.tolist()]
    pts = M.small_multiples(O)
    bases = np.stack([pts[k] for k in M.SMALL_KS])[kidx]
    scal = random_fr_uniform(0xED6E, n)
    pick = np.nonzero(rng.random(n) < 0.1)[0]
    pool_limbs = M.canonical_limbs(POOL)
    scal[pick] = pool_limbs[rng.integers(0, len(POOL), pick.size)]
    ints = [int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192 | int(x[4]) << 256 | int(x[5]) << 320
            for x in scal.tolist()]
    dot = sum(s * k for s, k in zip(ints, ks)) % R.R_MOD
    exp = O.jac_to_affine(O.scalar_mul(M.small_multiples(O)[1], fr_limbs(dot)))
    b = zk.Bases.upload(bases).precompute()
    dev = zk.DeviceBuffer(scal)
    stream = zk.MsmStream(b, depth=2)
    try:
        tickets = [stream.submit(dev.ptr, n, montgomery=False), stream.submit(dev.ptr, n - 12345, offset=12345, montgomery=False)]
        assert (zk.jac_to_affine(stream.collect(tickets[0])) == exp).all()
        dot2 = sum(s * k for s, k in zip(ints[:n - 12345], ks[12345:])) % R.R_MOD
        exp2 = O.jac_to_affine(O.scalar_mul(M.small_multiples(O)[1], fr_limbs(dot2)))
        assert (zk.jac_to_affine(stream.collect(tickets[1])) == exp2).all()
    finally:
        stream.free(); dev.free(); b.free()


def _small_key(O, m, n_primary, d, seed):
    """A proving key whose A, B1, B2, H and L queries are drawn from {O, +-G, +-2G, +-3G} (G1; B2 from G2), alpha, beta, delta
    random: not a real setup (the proof does not verify), but every MSM of the prover is full of same-x additions.  Returns the key
    and the multiples of G behind each query."""
    rng = random.Random(seed)
    draw = lambda cnt: [rng.choice(M.SMALL_KS) for _ in range(cnt)]
    ks = dict(A=draw(m), B1=draw(m), B2=draw(m), H=draw(d - 1), L=draw(m - n_primary - 1))
    alpha, beta, delta = (rng.randrange(1, R.R_MOD) for _ in range(3))
    g1 = M.small_multiples(O)[1]
    g2 = M.small_multiples(O, g2=True)[1]
    mul = lambda g, x: O.jac_to_affine(O.scalar_mul(g, fr_limbs(x)))
    pk = dict(alpha_g1=mul(g1, alpha), beta_g1=mul(g1, beta), beta_g2=mul(g2, beta), delta_g1=mul(g1, delta), delta_g2=mul(g2, delta),
              A=M.bases_of(O, ks["A"]), B1=M.bases_of(O, ks["B1"]), B2=M.bases_of(O, ks["B2"], g2=True),
              H=M.bases_of(O, ks["H"]), L=M.bases_of(O, ks["L"]))
    return pk, ks, (alpha, beta, delta)


@pytest.mark.parametrize("bool_frac", [0.0, 0.6])
@pytest.mark.parametrize("key_mode", ["plain", "tables", "tables+batched"])
def test_prover_five_msms_over_a_colliding_key(zk, oracle_lib, key_mode, bool_frac):
    """k_accumulate<5> and the reductions of the five merged MSMs of a proof (and the one-at-a-time and plain-key paths), each with
    the single-proof geometry and the streaming one (zkhip_prover_set_streaming: quad_below 1024, one stream, doubled slices,
    one-lane fold): the proof equals the oracle's limb for limb and each element's closed form."""
    O = oracle_lib
    n, n_primary = 3000, 4
    A, B, C, z = make_r1cs(90 + int(bool_frac * 10), n, n_primary, n, bool_frac)
    m = len(z)
    Ac, Bc, Cc = csr_from_rows(A), csr_from_rows(B), csr_from_rows(C)
    d = O.qap_domain_size(n, n_primary)
    pk, ks, (alpha, beta, delta) = _small_key(O, m, n_primary, d, seed=7)
    zl = fr_array(z)
    assert O.r1cs_first_unsatisfied(Ac, Bc, Cc, zl) == -1
    h_or = O.qap_h(Ac, Bc, Cc, zl, n, n_primary, d)
    rng = random.Random(8)
    r, s = rng.randrange(1, R.R_MOD), rng.randrange(1, R.R_MOD)
    exp = O.groth16_prove(pk, zl, n_primary, h_or, fr_limbs(r), fr_limbs(s))
    # per-element closed forms
    hi = fr_ints(h_or)
    dot = lambda xs, kk: sum(x * k for x, k in zip(xs, kk)) % R.R_MOD
    sa = (alpha + dot(z, ks["A"]) + r * delta) % R.R_MOD
    sb = (beta + dot(z, ks["B2"]) + s * delta) % R.R_MOD
    sb1 = (beta + dot(z, ks["B1"]) + s * delta) % R.R_MOD
    sc = (dot(z[n_primary + 1:], ks["L"]) + dot(hi[:d - 1], ks["H"]) + s * sa + r * sb1 - r * s % R.R_MOD * delta) % R.R_MOD
    g1, g2 = M.small_multiples(O)[1], M.small_multiples(O, g2=True)[1]
    mul = lambda g, x: O.jac_to_affine(O.scalar_mul(g, fr_limbs(x)))
    assert (exp[:24] == mul(g1, sa)).all() and (exp[24:48] == mul(g2, sb)).all() and (exp[48:] == mul(g1, sc)).all()
    crs = zk.Crs(pk, m, n_primary, d, opts=zk.key_opts(precompute=key_mode != "plain", batch_msms=key_mode == "tables+batched"))
    desc, keep = zk.make_r1cs_desc(Ac, Bc, Cc, m, n_primary)
    try:
        assert (crs.table_window > 0) == (key_mode != "plain")
        for streaming in (False, True):
            pr = zk.Prover(crs, desc)
            try:
                pr.set_streaming(streaming)
                for _ in range(2):                     # (a second proof on the same instance reuses its plans and slots)
                    proof = pr.prove(zl, fr_limbs(r), fr_limbs(s))
                    assert (proof == exp).all(), (key_mode, streaming)
            finally:
                pr.free()
    finally:
        crs.free()
