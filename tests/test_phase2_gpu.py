"""Phase-2 contributions on the device: zkhip_keypair_contribute (k_common_scalar_mul) against zkhip_keypair_contribute_host limb for
limb across the chunk seams, the closed form setup(delta s) = contribute(setup(delta), s), proofs under twice-contributed keys, and
zkhip_phase2_verify's report against zkhip_phase2_verify_host's and the Python model on the honest contribution and every tampering of
tests/phase2_fixtures.py.  Everything is bit-exact."""
import numpy as np
import pytest

from oracle import pyref as R
from tests import key_check_fixtures as K
from tests import phase2_fixtures as F
from tests.helpers import csr_from_rows, fr_array, fr_limbs, golden, h2i, make_r1cs
from tests.test_phase2_host import arrays_of, assert_same_key

pytestmark = pytest.mark.gpu

RM = R.R_MOD
TRAPDOOR = (0x1234567, 0x2345678, 0x3456789, 0x456789a)
SIZES = (3, 65, 130, 200)        # with the chunk at 64: H of 3 / 127 / 255 / 255 points, L of 1 / 63 / 128 / 198


@pytest.fixture(scope="module")
def zkc(zk):
    """the library with the chunk of the key check and of the contribution at 64 points"""
    zk.key_check_set_chunk(64)
    yield zk
    zk.key_check_set_chunk(0)


def with_infinities(key):
    """the point at infinity at the first, a middle and the last index of H and of L"""
    for name in ("h_query", "l_query"):
        n = len(key.el[name])
        for i in sorted({0, n // 2, n - 1}):
            key = key.replace(name, i, K.INFINITY)
    return key


@pytest.fixture(scope="module")
def long_keys(zkc):
    return {n: with_infinities(K.gpu_key(zkc, n)) for n in SIZES}


def both_routes(zk, key, tmp_path, s=F.S1, k=F.K1):
    kp = F.keypair_of(zk, key, tmp_path)
    host = kp.contribute(F.scalar_limbs(s), F.scalar_limbs(k), F.ZERO_DIGEST, host=True)
    dev = kp.contribute(F.scalar_limbs(s), F.scalar_limbs(k), F.ZERO_DIGEST, host=False)
    return kp, host, dev


@pytest.mark.parametrize("n", SIZES)
def test_device_contribution_equals_host_contribution(zkc, long_keys, tmp_path, n):
    """130 variables: H is three full chunks and one of 63, L two full chunks; 65: L is one chunk less a point, H a chunk and 63;
    3: one partial wave.  Infinities at both ends and in the middle of both vectors stay where they are."""
    key = long_keys[n]
    kp, (h_kp, h_rec, h_dig), (d_kp, d_rec, d_dig) = both_routes(zkc, key, tmp_path)
    try:
        assert_same_key(arrays_of(d_kp), arrays_of(h_kp))
        assert d_rec.to_bytes() == h_rec.to_bytes() and d_dig == h_dig
        pk = d_kp.pk_arrays()[0]
        for name, arr in (("h_query", pk["H"]), ("l_query", pk["L"])):
            inf = [i for i, p in enumerate(key.el[name]) if not p.limbs.any()]
            assert inf and [i for i in range(len(arr)) if not arr[i].any()] == inf
        assert zkc.phase2_last_ms()[0] > 0.0          # the longest launch of the device route was timed
    finally:
        kp.free(); h_kp.free(); d_kp.free()


def test_the_rule_chunk_gives_the_same_key(zk, long_keys, tmp_path):
    zk.key_check_set_chunk(0)
    try:
        kp, (h_kp, h_rec, h_dig), (d_kp, d_rec, d_dig) = both_routes(zk, long_keys[200], tmp_path, F.S2, F.K2)
        assert_same_key(arrays_of(d_kp), arrays_of(h_kp))
        assert d_rec.to_bytes() == h_rec.to_bytes() and d_dig == h_dig
        kp.free(); h_kp.free(); d_kp.free()
    finally:
        zk.key_check_set_chunk(64)


def test_scalars_at_the_edges_of_the_recoding(zkc, long_keys, tmp_path):
    """s = 1 (s^-1 = 1: one digit), s = r - 1 (every point negated), s = 2 (s^-1 = (r + 1) / 2) on the 65-variable key"""
    kp = F.keypair_of(zkc, long_keys[65], tmp_path)
    try:
        for s in (1, RM - 1, 2):
            h_kp, h_rec, _ = kp.contribute(F.scalar_limbs(s), F.scalar_limbs(F.K3), F.ZERO_DIGEST, host=True)
            d_kp, d_rec, _ = kp.contribute(F.scalar_limbs(s), F.scalar_limbs(F.K3), F.ZERO_DIGEST, host=False)
            assert_same_key(arrays_of(d_kp), arrays_of(h_kp))
            assert d_rec.to_bytes() == h_rec.to_bytes()
            if s == 1:
                assert_same_key(arrays_of(d_kp), arrays_of(kp))
            h_kp.free(); d_kp.free()
    finally:
        kp.free()


def test_scalars_whose_decomposition_has_an_empty_half(zkc, long_keys, tmp_path):
    """the device route runs the endomorphism form, s^-1 = k1 + k2 lambda: s^-1 = 5 and 2^188 (k2 = 0: phi(P) is never added),
    s^-1 = lambda and 7 lambda (k1 = 0: P is never added), -lambda (a negative half), against the host route"""
    from tools.gen_params import glv_params      # the generator of bw6_params.h: the lambda the kernel's constants belong to
    l = glv_params()["lam"]
    kp = F.keypair_of(zkc, long_keys[65], tmp_path)
    try:
        for sinv in (5, 1 << 188, l, 7 * l % RM, RM - l):
            s = pow(sinv, -1, RM)
            h_kp, h_rec, _ = kp.contribute(F.scalar_limbs(s), F.scalar_limbs(F.K2), F.ZERO_DIGEST, host=True)
            d_kp, d_rec, _ = kp.contribute(F.scalar_limbs(s), F.scalar_limbs(F.K2), F.ZERO_DIGEST, host=False)
            assert_same_key(arrays_of(d_kp), arrays_of(h_kp))
            assert d_rec.to_bytes() == h_rec.to_bytes()
            h_kp.free(); d_kp.free()
    finally:
        kp.free()


def test_the_baseline_form_is_identical_where_the_build_has_it(zkc, long_keys, tmp_path):
    """a normal build holds the endomorphism form only and says so; a build with both (tools/phase2_ab.py measures one) gives the same key"""
    kp = F.keypair_of(zkc, long_keys[130], tmp_path)
    try:
        zkc.phase2_set_form(2)
        endo = kp.contribute(F.scalar_limbs(F.S3), F.scalar_limbs(F.K3), F.ZERO_DIGEST)
        try:
            zkc.phase2_set_form(1)
        except zkc.ZkhipError as e:
            assert e.code == -4
        else:
            base = kp.contribute(F.scalar_limbs(F.S3), F.scalar_limbs(F.K3), F.ZERO_DIGEST)
            assert_same_key(arrays_of(base[0]), arrays_of(endo[0]))
            base[0].free()
        endo[0].free()
        with pytest.raises(zkc.ZkhipError):
            zkc.phase2_set_form(3)
    finally:
        zkc.phase2_set_form(0)
        kp.free()


def _systems():
    g = golden("groth16_small.json")
    small = (g["A"], g["B"], g["C"], [h2i(x) for x in g["z"]], g["n_primary"])
    A, B, C, z = make_r1cs(77, 100, 2, 60)
    return {"golden small": small, "a hundred constraints": (A, B, C, z, 2)}


@pytest.mark.parametrize("which", ("golden small", "a hundred constraints"))
def test_closed_form_and_proofs_after_two_contributions(zkc, which):
    """setup(tau, alpha, beta, delta).contribute(s) is setup(tau, alpha, beta, delta s) on every array and on vk(); a proof made with the
    twice-contributed key verifies under its vk() and not under the original's, a proof from the original key not under the new vk();
    the key check with the system's structure passes on the contributed key; and the prover's proof is the same before and after the
    contributions ran beside it (the call leaves no state)."""
    A, B, C, z, l = _systems()[which]
    desc, keep = zkc.make_r1cs_desc(*(csr_from_rows(x) for x in (A, B, C)), len(z), l)
    tau, alpha, beta, delta = TRAPDOOR
    setup = lambda d: zkc.Keypair(desc, fr_limbs(tau), fr_limbs(alpha), fr_limbs(beta), fr_limbs(d % RM))
    kp0 = setup(delta)
    zl, r, s = fr_array(z), fr_limbs(0x1111), fr_limbs(0x2222)
    crs0 = kp0.upload_crs()
    pr0 = zkc.Prover(crs0, desc)
    proof0 = pr0.prove(zl, r, s)
    kp1, rec1, d1 = kp0.contribute(F.scalar_limbs(F.S1), F.scalar_limbs(F.K1), F.ZERO_DIGEST)
    kp2, rec2, d2 = kp1.contribute(F.scalar_limbs(F.S2), F.scalar_limbs(F.K2), d1)
    closed1, closed2 = setup(delta * F.S1), setup(delta * F.S1 * F.S2)
    crs2 = kp2.upload_crs()
    pr2 = zkc.Prover(crs2, desc)
    try:
        assert_same_key(arrays_of(kp1), arrays_of(closed1))
        assert_same_key(arrays_of(kp2), arrays_of(closed2))
        for name, v in closed2.vk().items():
            assert (kp2.vk()[name] == v).all(), name
        assert (pr0.prove(zl, r, s) == proof0).all()                       # two handles, a prover and two contributions: no state left
        proof2 = pr2.prove(zl, r, s)
        inputs = zl[1:1 + l]
        assert zkc.groth16_verify(kp2.vk(), inputs, proof2)
        assert not zkc.groth16_verify(kp0.vk(), inputs, proof2)
        assert zkc.groth16_verify(kp0.vk(), inputs, proof0)
        assert not zkc.groth16_verify(kp2.vk(), inputs, proof0)
        assert zkc.check_key(kp2, r1cs=desc).ok == 1
        for before, after, rec, prev, nd in ((kp0, kp1, rec1, F.ZERO_DIGEST, d1), (kp1, kp2, rec2, d1, d2)):
            rep, got = zkc.phase2_verify(before, after, rec, prev)
            assert rep.ok == 1 and got == nd, rep.describe()
    finally:
        pr0.free(); pr2.free(); crs0.free(); crs2.free()
        for k in (kp0, kp1, kp2, closed1, closed2):
            k.free()
        del keep


@pytest.fixture(scope="module")
def device_cases(zkc):
    """the tamperings of the CPU list on the 130-variable key (chunk 64), its points from the library's fixed-base kernel"""
    mul = F.library_mul(zkc)
    out = []
    for tag, key in (("", K.gpu_key(zkc, 130)), ("inf: ", with_infinities(K.gpu_key(zkc, 130, seed=6)))):
        after, rec, _ = F.contribute_model(key, F.S1, F.K1, F.ZERO_DIGEST, mul)
        rho = F.rho_for(key)
        out += [(tag + label, b, a, r, p, rho) for label, b, a, r, p in F.tamperings(key, after, rec, F.ZERO_DIGEST, mul)]
    return out


from tests.test_phase2_host import N_CASES      # noqa: E402  (the same list of tamperings: the labels differ in their indices only)


@pytest.mark.parametrize("i", range(N_CASES))
def test_device_report_equals_host_report(zkc, device_cases, i):
    assert len(device_cases) == N_CASES
    label, before, after, rec, prev, rho = device_cases[i]
    host, host_digest = F.verify(zkc, before, after, rec, prev, rho, host=True)
    dev, dev_digest = F.verify(zkc, before, after, rec, prev, rho, host=False)
    want, want_digest = F.model_report(before, after, rec, prev, rho)
    assert dev == host == want, label
    assert dev_digest == host_digest == want_digest, label
    assert (want["ok"] == 1) == label.endswith("honest"), label


def test_the_model_contribution_is_the_library_s(zkc, device_cases, tmp_path):
    """the `after` the reports above are about is what contribute itself makes of `before`"""
    label, before, after, rec, prev, rho = device_cases[0]
    kp = F.keypair_of(zkc, before, tmp_path)
    new, got_rec, digest = kp.contribute(F.scalar_limbs(F.S1), F.scalar_limbs(F.K1), prev)
    try:
        pk, abc = after.arrays()
        assert_same_key(arrays_of(new), (dict(pk, ABC=abc), (after.n_vars, after.n_primary, after.domain_size)))
        assert got_rec.to_bytes() == rec.to_bytes() and digest == F.link(prev, rec)
    finally:
        kp.free(); new.free()


def test_drawn_scalars_on_the_device(zkc, device_cases):
    """rho = None: an honest contribution passes, a tampered one fails, whatever the OS draws"""
    honest = device_cases[0]
    tampered = next(c for c in device_cases if c[0].startswith("l'[0]"))
    rep, digest = F.verify(zkc, *honest[1:5], None, host=False)
    assert rep["ok"] == 1 and digest == F.link(honest[4], honest[3])
    rep, digest = F.verify(zkc, *tampered[1:5], None, host=False)
    assert rep["ok"] == 0 and rep["relations"] == 2 and rep["relations_evaluated"] == 7 and digest is None
