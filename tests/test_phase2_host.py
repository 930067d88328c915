"""Phase-2 contributions on the host alone (zkhip_keypair_contribute_host, zkhip_phase2_verify_host: no device): the contribution against
pyref's ec_mul, the verifier's report field by field against a Python model (tests/phase2_fixtures.py) on the honest contribution and
on every tampering, a chain of three contributions link by link, and the argument errors.  CPU only; everything is bit-exact."""
import ctypes

import numpy as np
import pytest

from oracle import pyref as R
from tests import key_check_fixtures as K
from tests import phase2_fixtures as F
from tests import point_check_fixtures as P
from tests.helpers import aff_limbs, aff_point

RM = R.R_MOD
N_CASES = 109      # len(F.host_cases()): asserted where the cases are built, so that collecting these tests multiplies no point


@pytest.fixture(scope="module")
def cases():
    out = F.host_cases()
    assert len(out) == N_CASES
    return out


@pytest.fixture(scope="module")
def zkl():
    from zecale_amd import zkhip
    zkhip.load()
    return zkhip


def arrays_of(kp):
    pk, m, l, d = kp.pk_arrays()
    return dict(pk, ABC=kp.vk()["ABC"]), (m, l, d)


def key_arrays(key):
    pk, abc = key.arrays()
    return dict(pk, ABC=abc), (key.n_vars, key.n_primary, key.domain_size)


def assert_same_key(got, want):
    assert got[1] == want[1]
    assert sorted(got[0]) == sorted(want[0])
    for name in want[0]:
        assert (np.asarray(got[0][name]).reshape(-1) == np.asarray(want[0][name]).reshape(-1)).all(), name


@pytest.mark.parametrize("infinite", [False, True], ids=["all finite", "variables at infinity"])
def test_contribute_host_equals_the_model(zkl, tmp_path, infinite):
    """H and L by s^-1 (pyref's ec_mul), delta by s in both groups, an entry at infinity stays there, every other element and the sizes
    byte-identical; the record and the digest are the ones Python computes; the key check still passes; verify_host accepts"""
    key = F.with_infinite_l(K.synthetic_key(infinity=(2, 5))) if infinite else K.synthetic_key()
    want, rec, digest = F.contribute_model(key, F.S1, F.K1, F.ZERO_DIGEST)
    kp = F.keypair_of(zkl, key, tmp_path)
    new, got_rec, got_digest = kp.contribute(F.scalar_limbs(F.S1), F.scalar_limbs(F.K1), F.ZERO_DIGEST, host=True)
    assert_same_key(arrays_of(new), key_arrays(want))
    assert got_rec.to_bytes() == rec.to_bytes() and got_digest == digest
    assert (new.vk()["delta"] == want.el["delta_g2"][0].limbs).all()
    assert_same_key(arrays_of(kp), key_arrays(key))                                  # the old key is untouched
    assert zkl.check_key(new, host=True).ok == 1
    rep, d2 = zkl.phase2_verify(kp, new, got_rec, F.ZERO_DIGEST, host=True)          # (scalars drawn from the OS)
    assert rep.ok == 1 and d2 == digest and rep.describe() == "phase 2: ok"
    out = tmp_path / "new.bin"
    new.write(out)
    assert out.read_bytes() == F.key_file_bytes(want)                                # write / read work on the new keypair unchanged
    kp.free(); new.free()


def test_contribute_host_on_the_golden_key(zkl, tmp_path):
    """a real key with its own system: the points have no known multiple, so pyref multiplies them; the structure check still passes"""
    key, cs = K.golden_small()
    kp = F.keypair_of(zkl, key, tmp_path)
    new, rec, digest = kp.contribute(F.scalar_limbs(F.S2), F.scalar_limbs(F.K2), F.ZERO_DIGEST, host=True)
    sinv = pow(F.S2, -1, RM)
    pk, _, _, _ = new.pk_arrays()
    for name, arr in (("h_query", pk["H"]), ("l_query", pk["L"])):
        for p, got in zip(key.el[name], arr):
            assert (got == aff_limbs(R.ec_mul(sinv, aff_point(p.limbs)))).all(), name
    for name in ("delta_g1", "delta_g2"):
        assert (pk[name] == aff_limbs(R.ec_mul(F.S2, aff_point(key.el[name][0].limbs)))).all()
    for name, k2 in (("alpha_g1", "alpha_g1"), ("beta_g1", "beta_g1"), ("beta_g2", "beta_g2"), ("a_query", "A"), ("b_g2_query", "B2"), ("b_g1_query", "B1")):
        assert (pk[k2].reshape(-1, 24) == np.array([p.limbs for p in key.el[name]])).all()
    assert zkl.check_key(new, r1cs=K.cs_desc(zkl, cs), host=True).ok == 1
    rep, d2 = zkl.phase2_verify(kp, new, rec, F.ZERO_DIGEST, host=True)
    assert rep.ok == 1 and d2 == digest
    kp.free(); new.free()


def test_three_contributions_verify_link_by_link(zkl, tmp_path):
    kp = F.keypair_of(zkl, K.synthetic_key(), tmp_path)
    chain, digest = [kp], F.ZERO_DIGEST
    links = []
    for s, k in ((F.S1, F.K1), (F.S2, F.K2), (F.S3, F.K3)):
        new, rec, nd = chain[-1].contribute(F.scalar_limbs(s), F.scalar_limbs(k), digest, host=True)
        links.append((chain[-1], new, rec, digest, nd))
        chain.append(new)
        digest = nd
    for before, after, rec, prev, nd in links:
        rep, got = zkl.phase2_verify(before, after, rec, prev, host=True)
        assert rep.ok == 1 and got == nd
    # a link does not verify out of its place: over the wrong predecessor, or under the wrong digest
    rep, got = zkl.phase2_verify(chain[0], chain[2], links[1][2], links[1][3], host=True)
    assert rep.ok == 0 and got is None
    rep, got = zkl.phase2_verify(chain[1], chain[2], links[1][2], F.ZERO_DIGEST, host=True)
    assert rep.ok == 0 and rep.relations == 4 and got is None
    # the three secrets multiply: delta is delta_0 s1 s2 s3
    d0 = K.synthetic_key().el["delta_g1"][0].k
    assert (chain[3].consts()["delta_g1"] == K.multiple(d0 * F.S1 * F.S2 * F.S3 % RM, False).limbs).all()
    for c in chain:
        c.free()


def test_drawn_secrets(zkl, tmp_path):
    """s = k = None: drawn from the OS - two contributions differ, and both verify"""
    kp = F.keypair_of(zkl, K.synthetic_key(), tmp_path)
    a, rec_a, da = kp.contribute(host=True)
    b, rec_b, db = kp.contribute(host=True)
    assert rec_a.to_bytes() != rec_b.to_bytes() and da != db
    for new, rec, d in ((a, rec_a, da), (b, rec_b, db)):
        rep, got = zkl.phase2_verify(kp, new, rec, F.ZERO_DIGEST, host=True)
        assert rep.ok == 1 and got == d
    kp.free(); a.free(); b.free()


@pytest.mark.parametrize("i", range(N_CASES))
def test_verify_host_report_equals_the_model(zkl, cases, i):
    label, before, after, rec, prev, rho = cases[i]
    want, want_digest = F.model_report(before, after, rec, prev, rho)
    got, digest = F.verify(zkl, before, after, rec, prev, list(rho), host=True)
    assert got == want, label
    assert digest == want_digest, label


def test_what_the_cases_must_show(cases):
    """the model itself says what is asked of these contributions (so that a model that agreed with a wrong library would not pass)"""
    CASES = cases
    rep = {c[0]: F.model_report(*c[1:])[0] for c in CASES}
    dig = {c[0]: F.model_report(*c[1:])[1] for c in CASES}
    for tag in ("", "inf: "):
        assert rep[tag + "honest"]["ok"] == 1 and rep[tag + "honest"]["relations_evaluated"] == 7 and dig[tag + "honest"] is not None
        assert all(r["ok"] == 0 and dig[label] is None for label, r in rep.items() if not label.endswith("honest"))
        for label, r in rep.items():
            if label.startswith(tag + "l'[") and label.endswith("another multiple") or label.startswith(tag + "h'[") and label.endswith("another scalar"):
                assert (r["changed"], r["relations"], r["relations_evaluated"]) == (0, 2, 7), label
        r = rep[tag + "delta_g2' another multiple"]
        assert (r["relations"], r["relations_evaluated"]) == (1 | 2, 7)
        r = rep[tag + "delta' another common multiple"]
        assert (r["relations"], r["relations_evaluated"]) == (2 | 4, 7)
        assert rep[tag + "the record's delta_g1 is not the key's"]["changed"] == 1 << 3
        assert rep[tag + "a_query[0] changed"]["changed"] == 1 << K.A and rep[tag + "beta_g2 changed"]["changed"] == 1 << 2
        assert rep[tag + "n_primary changed"]["changed"] == 1 << 31 and rep[tag + "n_primary changed"]["relations_evaluated"] == 0
        r = rep[tag + "an l' entry set to infinity"]
        assert r["infinity_mismatch"] == K.L and not r["relations_evaluated"] & 2
        assert rep[tag + "an h' entry set to infinity"]["infinity_mismatch"] == K.H
        r = rep[tag + "delta' at infinity"]
        assert r["elements"]["delta_g1"][1] == 1 and r["relations_evaluated"] == 0
        for label, r in rep.items():
            if label.startswith(tag) and any(label.endswith(e.name) for e in P.bad_points(False)) and (tag or not label.startswith("inf: ")):
                assert sum(sum(e[2]) for e in r["elements"].values()) == 1 and not r["relations_evaluated"] & 2 and r["ok"] == 0, label
        for name in ("pok_response + 1", "pok_response >= r", "another prev_digest", "replayed on another before"):
            assert (rep[tag + name]["changed"], rep[tag + name]["relations"], rep[tag + name]["relations_evaluated"]) == (0, 4, 7), name
    assert rep["inf: an infinite l' entry made finite"]["infinity_mismatch_first"] == 1
    # every kind of refused point meets H', L', delta_g1' and T
    for where in ("h'[", "l'[", "delta_g1': ", "T: "):
        codes = sorted(max(e[4] for e in r["elements"].values()) for label, r in rep.items()
                       if label.startswith(where) and any(label.endswith(e.name) for e in P.bad_points(False)))
        assert codes == [P.ENCODING] * 2 + [P.OFF_CURVE] * 2 + [P.NOT_ORDER_R] * 4, where


def test_describe_names_what_failed(zkl, cases):
    label, before, after, rec, prev, rho = next(c for c in cases if c[0] == "delta_g2' another multiple")
    desc = lambda key: (key.arrays()[0], key.n_vars, key.n_primary, key.domain_size)
    rep, _ = zkl.phase2_verify(desc(before), desc(after), rec.struct(zkl), prev, rho=list(rho), host=True)
    text = rep.describe()
    assert "delta_g1'/delta_g2': fails" in text and "ratio" in text and "proof of knowledge" not in text


def test_argument_errors(zkl, tmp_path):
    key = K.synthetic_key()
    after, rec, _ = F.contribute_model(key, F.S1, F.K1, F.ZERO_DIGEST)
    kp = F.keypair_of(zkl, key, tmp_path)
    zero = np.zeros(6, dtype=np.uint64)
    r_limbs = np.array(R.int_to_limbs(RM, 6), dtype=np.uint64)
    for s, k in ((zero, F.scalar_limbs(F.K1)), (F.scalar_limbs(F.S1), zero), (r_limbs, F.scalar_limbs(F.K1))):
        with pytest.raises(zkl.ZkhipError) as e:
            kp.contribute(s, k, F.ZERO_DIGEST, host=True)
        assert e.value.code == -1
    rho = F.rho_for(key)
    rho[len(rho) - 1] = 0
    with pytest.raises(zkl.ZkhipError) as e:
        F.verify(zkl, key, after, rec, F.ZERO_DIGEST, rho, host=True)
    assert e.value.code == -1
    # null pointers
    lib = zkl.load()
    db, keep = zkl.make_crs_desc(key.arrays()[0], key.n_vars, key.n_primary, key.domain_size)
    rs, out, dg = rec.struct(zkl), zkl.Phase2Report(), ctypes.create_string_buffer(32)
    assert lib.zkhip_phase2_verify_host(None, ctypes.byref(db), ctypes.byref(rs), F.ZERO_DIGEST, None, ctypes.byref(out), dg) == -1
    assert lib.zkhip_phase2_verify_host(ctypes.byref(db), ctypes.byref(db), None, F.ZERO_DIGEST, None, ctypes.byref(out), dg) == -1
    assert lib.zkhip_phase2_verify_host(ctypes.byref(db), ctypes.byref(db), ctypes.byref(rs), F.ZERO_DIGEST, None, None, dg) == -1
    h = ctypes.c_void_p()
    assert lib.zkhip_keypair_contribute_host(None, None, None, F.ZERO_DIGEST, ctypes.byref(h), ctypes.byref(rs), dg) == -1
    assert lib.zkhip_keypair_contribute_host(kp.handle, None, None, F.ZERO_DIGEST, None, ctypes.byref(rs), dg) == -1
    # without a device the device routes refuse to run; they do not fall back to the host
    import torch
    if not torch.cuda.is_available():      # (meaningful only where there is no GPU)
        with pytest.raises(zkl.ZkhipError) as e:
            kp.contribute(F.scalar_limbs(F.S1), F.scalar_limbs(F.K1), F.ZERO_DIGEST)
        assert e.value.code == -2
        with pytest.raises(zkl.ZkhipError) as e:
            F.verify(zkl, key, after, rec, F.ZERO_DIGEST, None, host=False)
        assert e.value.code == -2
    # vectors of different length between before and after: a report, not an error
    shorter = K.synthetic_key(n_vars=5)
    got, digest = F.verify(zkl, key, shorter, rec, F.ZERO_DIGEST, None, host=True)
    assert got["changed"] == 1 << 31 and got["ok"] == 0 and digest is None
    kp.free()
    del keep
