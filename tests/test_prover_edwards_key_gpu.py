"""Proving keys on the Edwards model (zkhip_key_opts.table_model = 1): the four G1 MSMs of a proof - A, B-G1, H, L - go through ONE
launch sequence that adds on G1's 2-isogenous twisted Edwards curve, B-G2 through an XYZZ sequence of its own.  The proof must equal,
limb for limb, the proof under the same key uploaded with table_model = 0 (and the oracle's, where one exists), in every place that
can be handed such a key; and zkhip_prover_last_table_model / zkhip_last_prove_table_model must say that the launches really took the
Edwards route: without that observable a silent fall-back to XYZZ passes every parity check."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests.helpers import aff_limbs, crs_from_trapdoor, csr_from_rows, fr_array, fr_int, fr_limbs, golden, h2i, make_r1cs, pt_from_json
from tests.point_check_fixtures import bad_points
from tests.test_aggregator_host import nested_proof_limbs, nested_vk_limbs
from tests.test_oracle_pins import load_nested_fixtures

pytestmark = pytest.mark.gpu

_cache = {}


def _golden_system(zk, O):
    g = golden("groth16_small.json")
    pts = lambda L: np.array([aff_limbs(pt_from_json(p)) for p in L]).reshape(-1, 24)
    pk = {k: (aff_limbs(pt_from_json(v)) if k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2") else pts(v)) for k, v in g["pk"].items()}
    csr = tuple(csr_from_rows(g[k]) for k in "ABC")
    want = np.concatenate([aff_limbs(pt_from_json(g["proof"][k])) for k in "abc"])          # (computed by oracle/pyref.py, pairing-checked)
    return dict(pk=pk, csr=csr, m=len(g["z"]), l=g["n_primary"], d=1 << g["log_d"], z=fr_array([h2i(x) for x in g["z"]]),
                r=fr_limbs(h2i(g["r"])), s=fr_limbs(h2i(g["s"])), oracle=want)


def _random_system(zk, O):
    """about 1,000 constraints, a boolean-heavy witness, known toxic waste; the expected proof from the C oracle (made once)"""
    if "random" not in _cache:
        n, l = 1000, 4
        A, B, C, z = make_r1cs(2024, n, l, n, 0.5)
        m = len(z)
        rng = random.Random(6)
        tau, alpha, beta, delta, r, s = (rng.randrange(1, R.R_MOD) for _ in range(6))
        pk, d = crs_from_trapdoor(zk, A, B, C, m, l, tau, alpha, beta, delta)
        csr = (csr_from_rows(A), csr_from_rows(B), csr_from_rows(C))
        zl = fr_array(z)
        want = O.groth16_prove(pk, zl, l, O.qap_h(*csr, zl, n, l, d), fr_limbs(r), fr_limbs(s))
        _cache["random"] = dict(pk=pk, csr=csr, m=m, l=l, d=d, z=zl, r=fr_limbs(r), s=fr_limbs(s), oracle=want)
    return _cache["random"]


def _edw(zk, **kw):
    return zk.key_opts(table_model=1, **kw)


@pytest.mark.parametrize("system", ["golden", "random"])
def test_small_systems_same_proof_and_the_edwards_route(zk, oracle_lib, system):
    S = (_golden_system if system == "golden" else _random_system)(zk, oracle_lib)
    r1 = zk.R1cs(*S["csr"], S["m"], S["l"])
    desc, keep = zk.make_r1cs_desc(*S["csr"], S["m"], S["l"])
    xyzz = zk.Crs(S["pk"], S["m"], S["l"], S["d"], opts=zk.key_opts(table_model=0))
    edw = zk.Crs(S["pk"], S["m"], S["l"], S["d"], opts=_edw(zk))
    try:
        assert (xyzz.table_model, xyzz.table_kind) == (0, 1)
        assert (edw.table_model, edw.table_kind) == (1, 1) and edw.table_window == xyzz.table_window
        p_x = zk.groth16_prove(xyzz, r1, S["z"], S["r"], S["s"])
        assert zk.last_prove_table_model() == 0
        n_x = zk.last_accumulate_entries()
        p_e = zk.groth16_prove(edw, r1, S["z"], S["r"], S["s"])
        assert zk.last_prove_table_model() == 1
        n_e = zk.last_accumulate_entries()                        # both sequences together: the digits are the same
        assert (p_e == p_x).all() and (p_e == S["oracle"]).all()
        assert n_e == n_x and n_e > 0
        for crs, model, n_want in ((edw, 1, n_x), (xyzz, 0, n_x)):
            pr = zk.Prover(crs, desc)
            for _ in range(2):
                assert (pr.prove(S["z"], S["r"], S["s"]) == S["oracle"]).all()
                assert pr.last_table_model() == model and pr.last_accumulate_entries() == n_want
            pr.free()
    finally:
        xyzz.free(); edw.free(); r1.free()


def test_option_rules(zk, oracle_lib):
    S = _golden_system(zk, oracle_lib)
    key = lambda opts: zk.Crs(S["pk"], S["m"], S["l"], S["d"], opts=opts)
    r1 = zk.R1cs(*S["csr"], S["m"], S["l"])
    for bad in (_edw(zk, precompute=False), _edw(zk, table_naf=True), zk.key_opts(table_model=2), zk.key_opts(table_model=-1)):
        with pytest.raises(zk.ZkhipError) as e:
            key(bad)
        assert e.value.code == -1                                  # ZKHIP_ERR_ARG
    zk.set_crs_precompute(False)                                   # the RESOLVED option counts: no tables by the process-wide default
    try:
        with pytest.raises(zk.ZkhipError) as e:
            key(_edw(zk))
        assert e.value.code == -1
    finally:
        zk.set_crs_precompute(True)
    zk.set_table_naf(1)                                            # table_naf = -1: one level per window whatever the process default says
    try:
        crs = key(_edw(zk))
        assert (crs.table_model, crs.table_kind) == (1, 1)
        crs.free()
        crs = key(zk.key_opts())                                   # (the default key does follow it)
        assert (crs.table_model, crs.table_kind) == (0, 2)
        crs.free()
    finally:
        zk.set_table_naf(-1)
    crs = key(_edw(zk, table_naf=False, window=11))
    assert (crs.table_model, crs.table_kind, crs.table_window) == (1, 1, 11)
    assert (zk.groth16_prove(crs, r1, S["z"], S["r"], S["s"]) == S["oracle"]).all() and zk.last_prove_table_model() == 1
    crs.free()
    for opts in (zk.KeyOpts(-1, -1, 0, -1), zk.KeyOpts(), None):   # the four earlier fields alone, all zeros (plain base sets), no options
        crs = key(opts)
        assert crs.table_model == 0
        assert (zk.groth16_prove(crs, r1, S["z"], S["r"], S["s"]) == S["oracle"]).all() and zk.last_prove_table_model() == 0
        crs.free()
    r1.free()


def test_a_key_that_cannot_go_edwards_stays_xyzz(zk, oracle_lib):
    """One L point replaced by generator + a point of order 2: on the curve, not of order r.  msm_table_edw refuses L; the forms built
    for A, B-G1 and H are freed, the upload succeeds, and the key proves as the same key uploaded with table_model = 0."""
    S = _random_system(zk, oracle_lib)
    bad = bad_points(False)[1]
    assert bad.name == "g1 generator + small order"
    pk = dict(S["pk"])
    pk["L"] = S["pk"]["L"].copy()
    at = next(i for i in range(S["m"] - S["l"] - 1) if S["z"][S["l"] + 1 + i].any())      # an L base whose scalar is not zero
    pk["L"][at] = bad.limbs
    r1 = zk.R1cs(*S["csr"], S["m"], S["l"])
    xyzz = zk.Crs(pk, S["m"], S["l"], S["d"], opts=zk.key_opts(table_model=0))
    edw = zk.Crs(pk, S["m"], S["l"], S["d"], opts=_edw(zk))
    try:
        assert edw.table_model == 0 and edw.table_kind == 1
        want = zk.groth16_prove(xyzz, r1, S["z"], S["r"], S["s"])
        assert not (want == S["oracle"]).all()                     # (the replaced point does take part)
        assert (zk.groth16_prove(edw, r1, S["z"], S["r"], S["s"]) == want).all()
        assert zk.last_prove_table_model() == 0
    finally:
        xyzz.free(); edw.free(); r1.free()


@pytest.mark.parametrize("batch", [True, False], ids=["one-g1-sequence", "sequence-per-msm"])
def test_batch_msms_off_takes_the_single_msm_edwards_kernels(zk, oracle_lib, batch):
    S = _random_system(zk, oracle_lib)
    r1 = zk.R1cs(*S["csr"], S["m"], S["l"])
    crs = zk.Crs(S["pk"], S["m"], S["l"], S["d"], opts=_edw(zk, batch_msms=batch))
    try:
        assert crs.table_model == 1
        assert (zk.groth16_prove(crs, r1, S["z"], S["r"], S["s"]) == S["oracle"]).all()
        assert zk.last_prove_table_model() == 1
    finally:
        crs.free(); r1.free()


def test_two_slices_add_up_to_the_whole_key(zk, oracle_lib):
    """zkhip_crs_upload_slice_ex with table_model = 1: the partial sums of two slices are the five sums of the whole key."""
    S = _random_system(zk, oracle_lib)
    m, l, d = S["m"], S["l"], S["d"]
    r1 = zk.R1cs(*S["csr"], m, l)
    whole = zk.Crs.upload_slice(S["pk"], m, l, d, (0, m), (0, d - 1), (0, m - l - 1), opts=zk.key_opts(table_model=0))      # (the whole key is a slice too)
    cuts = zk.key_partition(S["pk"], m, l, d, 2)
    try:
        want = zk.groth16_prove_partial(whole, r1, S["z"])
        total = None
        for rank in range(2):
            sl = zk.Crs.upload_slice(S["pk"], m, l, d, *((int(c[rank]), int(c[rank + 1])) for c in cuts), opts=_edw(zk))
            assert sl.table_model == 1
            part = zk.groth16_prove_partial(sl, r1, S["z"])
            assert zk.last_prove_table_model() == 1
            total = part if total is None else np.array([zk.jac_add(total[k], part[k]) for k in range(5)])
            sl.free()
        for k in range(5):
            assert (zk.jac_to_affine(total[k]) == zk.jac_to_affine(want[k])).all(), k
        assert (zk.groth16_finish(S["pk"], total, S["r"], S["s"]) == S["oracle"]).all()
    finally:
        whole.free(); r1.free()


# ---- the real wrapping circuit: batch 2 on the 65,536-point domain, host witness ---------------------------------------------------
def _wrapping(zk):
    """circuit, trusted setup and four witnesses of the reference's nested fixtures (made once for this module)"""
    if "wrap" not in _cache:
        agg = zk.AggregatorCircuit(2, 1)
        desc = zk.r1cs_desc_from_aggregator(agg)
        kp = zk.Keypair(desc, fr_limbs(0x1234567), fr_limbs(0x2345678), fr_limbs(0x3456789), fr_limbs(0x456789a))
        assert kp.domain_size == 65536
        nvk, proofs = load_nested_fixtures()
        nvk_l = nested_vk_limbs(nvk)
        batches = []
        for a, b in ((0, 1), (2, 3), (4, 5), (1, 0)):
            (pa, ia), (pb, ib) = proofs[a], proofs[b]
            batches.append((np.concatenate([nested_proof_limbs(pa), nested_proof_limbs(pb)]), np.array([fr_limbs(ia[0]), fr_limbs(ib[0])])))
        zs = [agg.witness(nvk_l, npr, nin) for npr, nin in batches]
        rs = [(fr_limbs(0x1111 + i), fr_limbs(0x2222 + 3 * i)) for i in range(4)]
        _cache["wrap"] = dict(agg=agg, desc=desc, kp=kp, nvk=nvk_l, batches=batches, zs=zs, rs=rs, vk=kp.vk())
    return _cache["wrap"]


def _wrapping_keys(zk):
    """the XYZZ key, the Edwards key and the serial XYZZ proofs of the four witnesses"""
    W = _wrapping(zk)
    if "keys" not in _cache:
        xyzz, edw = W["kp"].upload_crs(zk.key_opts(table_model=0)), W["kp"].upload_crs(_edw(zk))
        r1 = zk.r1cs_from_desc(W["desc"])
        assert (xyzz.table_model, edw.table_model, edw.table_kind) == (0, 1, 1) and edw.table_window == xyzz.table_window
        serial = [zk.groth16_prove(xyzz, r1, z, r, s) for z, (r, s) in zip(W["zs"], W["rs"])]
        _cache["keys"] = (xyzz, edw, r1, serial)
    return (W,) + _cache["keys"]


def test_wrapping_proof_plain_and_through_an_application_handle(zk):
    W, xyzz, edw, r1, serial = _wrapping_keys(zk)
    n_prim = W["agg"].num_primary_inputs()
    z, (r, s) = W["zs"][0], W["rs"][0]
    entries_x = None
    zk.groth16_prove(xyzz, r1, z, r, s)
    entries_x = zk.last_accumulate_entries()
    proof = zk.groth16_prove(edw, r1, z, r, s)
    assert zk.last_prove_table_model() == 1 and zk.last_accumulate_entries() == entries_x
    assert (proof == serial[0]).all()
    primary = z[1:1 + n_prim]
    assert zk.groth16_verify(W["vk"], primary, proof) and fr_int(primary[1]) == 3
    app = zk.AggregatorApp(W["agg"], edw, W["nvk"])
    pr = zk.Prover(edw, W["desc"])
    try:
        zm = app.witness(*W["batches"][0])
        assert (zm == app.mask(z)).all()
        assert (app.prove(r1, zm, r, s) == proof).all() and zk.last_prove_table_model() == 1
        assert (pr.prove_app(app, zm, r, s) == proof).all() and pr.last_table_model() == 1
    finally:
        pr.free(); app.free()


def test_streaming_prover_chains_edwards_proofs_and_changes_models(zk):
    """zkhip_prover_set_streaming: from its second proof on the instance puts the upload and the QAP map on the G1 sequence's stream and
    B-G2's stream follows the upload through an event.  Four witnesses back to back, twice, each equal to its serial proof.  A prover
    instance belongs to one key, so the change of models on ONE set of contexts is the next test's (the plain entry point); here a
    streaming XYZZ instance proves between the Edwards instance's proofs, and streaming is switched off again."""
    W, xyzz, edw, r1, serial = _wrapping_keys(zk)
    p = zk.Prover(edw, W["desc"])
    q = zk.Prover(xyzz, W["desc"])
    try:
        p.set_streaming(True); q.set_streaming(True)
        for rep in range(2):
            for i in range(4):
                assert (p.prove(W["zs"][i], *W["rs"][i]) == serial[i]).all(), (rep, i)
                assert p.last_table_model() == 1
                assert p.timings()["chained"] == (rep > 0 or i > 0)
        assert (q.prove(W["zs"][1], *W["rs"][1]) == serial[1]).all() and q.last_table_model() == 0
        assert (p.prove(W["zs"][2], *W["rs"][2]) == serial[2]).all() and p.last_table_model() == 1
        p.set_streaming(False)
        assert (p.prove(W["zs"][3], *W["rs"][3]) == serial[3]).all() and not p.timings()["chained"]
    finally:
        p.free(); q.free()


def test_one_instance_serves_both_models_through_the_plain_entry_point(zk):
    """The plain entry point's contexts are shared by every key on the device: Edwards, XYZZ, Edwards again - the contexts are planned
    again for the other model (K = 4 and K = 1 against K = 5) and every proof is the serial one."""
    W, xyzz, edw, r1, serial = _wrapping_keys(zk)
    for crs, model, i in ((edw, 1, 0), (xyzz, 0, 1), (edw, 1, 2), (edw, 1, 3), (xyzz, 0, 0)):
        assert (zk.groth16_prove(crs, r1, W["zs"][i], *W["rs"][i]) == serial[i]).all()
        assert zk.last_prove_table_model() == model


def test_pipeline_with_an_edwards_key(zk):
    """Eight batches through zkhip_aggregator_pipeline_* (its slots only see the key's handle): every wrapping proof equals the serial
    XYZZ proof of its batch and verifies with its expected result bits - one batch has a bumped nested input (bits 1)."""
    W, xyzz, edw, r1, serial = _wrapping_keys(zk)
    agg, n_prim = W["agg"], W["agg"].num_primary_inputs()
    pipe = zk.AggregatorPipeline(agg, edw, gpu_slots=3, witness_workers=2)
    try:
        jobs = []
        for i in range(8):
            npr, nin = W["batches"][i % 4]
            bump = 1 if i == 5 else 0
            nin = nin.copy()
            if bump:
                nin[1] = fr_limbs(fr_int(nin[1]) + 1)
            r, s = fr_limbs(0xaaaa + i), fr_limbs(0xbbbb + 7 * i)
            jobs.append((npr, nin, r, s, 1 if bump else 3, pipe.submit(W["nvk"], npr, nin, r, s)))
        for npr, nin, r, s, bits, ticket in reversed(jobs):
            prim, proof = pipe.wait(ticket)
            z = agg.witness(W["nvk"], npr, nin)
            assert (prim == z[1:1 + n_prim]).all() and fr_int(prim[1]) == bits
            assert (proof == zk.groth16_prove(xyzz, r1, z, r, s)).all()
            assert zk.groth16_verify(W["vk"], prim, proof)
    finally:
        pipe.free()
