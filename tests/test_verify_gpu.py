"""Groth16 verification in batches on the GPU (zkhip_verifier: the BW6-761 pairing kernels of zecale_amd/csrc/pairing.hip) against
the host verifier it is pinned on (zkhip_groth16_verify) and pyref's big integers: the Fq6 lane bodies inside a real kernel, reduced
GT values limb for limb, the reference's own fixtures (client/test_commands/test_bw6_761_groth16_contract.py:66-79), the golden small
circuit, mixed batches of trapdoor statements, and handles running beside each other and beside a prover.
G = 8 verifications share a wave and WG = 16 a workgroup: the batch sizes sit on both sides of either."""
import random
import threading

import numpy as np
import pytest

from oracle import pyref as R
from tests import verify_fixtures as V
from tests.helpers import aff_limbs, aff_point, csr_from_rows, fr_array, fr_limbs, golden, h2i, pt_from_json

pytestmark = pytest.mark.gpu

G, WG = 8, 16


def test_group_sizes(zk):
    assert (zk.VERIFIER_GROUP, zk.VERIFIER_WORKGROUP) == (G, WG)


# ---------------------------------------------------------------- (a) the lane bodies in a kernel
@pytest.mark.parametrize("op", ["mul", "sqr", "mul_line"])
def test_fq6_lane_bodies_in_a_kernel(zk, op):
    cases = V.fq6_cases()
    want = [V.fq6_expected(op, a, b) for a, b in cases]
    for n in (1, G, G + 1, WG + 1):
        idx = [(i * 5 + n) % len(cases) for i in range(n)]          # every case appears at n = WG + 1; the sets of a group differ
        got = zk.fq6_selftest(op, np.array([V.fq6_limbs(cases[i][0]) for i in idx]), np.array([V.fq6_limbs(cases[i][1]) for i in idx]))
        for row, i in zip(got, idx):
            assert V.fq6_ints(row) == want[i], (op, n, i)


# ---------------------------------------------------------------- (b) reduced GT values
def _both_routes(zk, products):
    """products: list of lists of (P, Q) of one length -> (GPU values, host values), each count x 6 x 12 limbs"""
    g1 = np.array([[aff_limbs(P) for P, _ in pr] for pr in products])
    g2 = np.array([[aff_limbs(Q) for _, Q in pr] for pr in products])
    return zk.pairing_product("gpu", g1, g2), zk.pairing_product("host", g1, g2)


def test_pairing_of_the_generators_and_bilinearity(zk):
    e = V.gt_value([(R.G1_GEN, R.G2_GEN)])
    assert e != V.EXT.one()
    rng = random.Random(5)
    uv = [(1, 1), (2, 3), (7, 1), (rng.randrange(R.R_MOD), rng.randrange(R.R_MOD)), (R.R_MOD - 1, 5), (rng.randrange(R.R_MOD), R.R_MOD - 2)]
    for u, v in uv:
        gpu, host = _both_routes(zk, [[(V.g1mul(u), V.g2mul(v))]])
        assert (gpu == host).all(), (u, v)
        assert V.fq6_ints(gpu[0]) == V.EXT.pow(e, u * v % R.R_MOD), (u, v)       # e(uP, vQ) = e(P, Q)^(uv)


def _batch1_pairs():
    vk = golden("dummy_app/aggregator_vk.json")
    ep = golden("dummy_app/batch1.json")["ext_proof"]
    acc = pt_from_json(vk["ABC"][0])
    for x, P in zip(ep["inputs"], vk["ABC"][1:]):
        acc = R.ec_add(acc, R.ec_mul(h2i(x), pt_from_json(P)))
    pr = {k: pt_from_json(v) for k, v in ep["proof"].items()}
    return [(pr["a"], pr["b"]), (acc, R.ec_neg(R.G2_GEN)), (pt_from_json(vk["alpha"]), R.ec_neg(pt_from_json(vk["beta"]))),
            (pr["c"], R.ec_neg(pt_from_json(vk["delta"])))]


def test_pairing_products_of_the_reference_fixture_and_with_infinity(zk):
    four = _batch1_pairs()
    gpu, host = _both_routes(zk, [four])
    assert (gpu == host).all()
    assert V.fq6_ints(gpu[0]) == V.EXT.one() == V.gt_value(four)                # the valid proof's product is one
    # each pair on its own, then products in which P or Q of one pair is the point at infinity (it contributes 1)
    singles = [[p] for p in four]
    gpu, host = _both_routes(zk, singles)
    assert (gpu == host).all()
    vals = [V.fq6_ints(x) for x in gpu]
    assert vals == [V.gt_value(s) for s in singles]
    with_inf = [[four[0], (None, four[1][1]), four[2]], [four[0], four[1], (four[2][0], None)], [(None, None), four[1], four[3]]]
    gpu, host = _both_routes(zk, with_inf)
    assert (gpu == host).all()
    mul = V.EXT.mul
    assert [V.fq6_ints(x) for x in gpu] == [mul(vals[0], vals[2]), mul(vals[0], vals[1]), mul(vals[1], vals[3])]


@pytest.mark.parametrize("count", [1, G + 1, WG + 1])
def test_pairing_products_differ_per_position(zk, count):
    """two pairs per product, other points at every position: position i holds e(u_i G1, G2) e(G1, v_i G2) = e^(u_i + v_i)"""
    rng = random.Random(count)
    e = V.gt_value([(R.G1_GEN, R.G2_GEN)])
    uv = [(rng.randrange(1, R.R_MOD) if i % 3 else i + 2, rng.randrange(1, R.R_MOD) if i % 2 else 3 * i + 1) for i in range(count)]
    gpu, host = _both_routes(zk, [[(V.g1mul(u), R.G2_GEN), (R.G1_GEN, V.g2mul(v))] for u, v in uv])
    assert (gpu == host).all()
    for x, (u, v) in zip(gpu, uv):
        assert V.fq6_ints(x) == V.EXT.pow(e, (u + v) % R.R_MOD)


# ---------------------------------------------------------------- (c), (d) fixtures
def _vk(j):
    return dict(alpha=aff_limbs(pt_from_json(j["alpha"])), beta=aff_limbs(pt_from_json(j["beta"])),
                delta=aff_limbs(pt_from_json(j["delta"])), ABC=np.array([aff_limbs(pt_from_json(p)) for p in j["ABC"]]))


def _proof(j):
    return np.concatenate([aff_limbs(pt_from_json(j["a"])), aff_limbs(pt_from_json(j["b"])), aff_limbs(pt_from_json(j["c"]))])


def test_reference_fixtures_alone_and_together(zk):
    vk = _vk(golden("dummy_app/aggregator_vk.json"))
    st = {}
    for name in ("batch1.json", "batch1-invalid.json"):
        ep = golden("dummy_app/" + name)["ext_proof"]
        st[name] = (np.array([fr_limbs(h2i(x)) for x in ep["inputs"]]), _proof(ep["proof"]))
    v = zk.Verifier(vk)
    good, bad = st["batch1.json"], st["batch1-invalid.json"]
    assert list(v.verify_batch([good[0]], [good[1]])) == [True]
    assert list(v.verify_batch([bad[0]], [bad[1]])) == [False]
    assert list(v.verify_batch([good[0], bad[0]], [good[1], bad[1]])) == [True, False]
    assert list(v.verify_batch([bad[0], good[0]], [bad[1], good[1]])) == [False, True]
    assert list(v.verify_batch(np.zeros((0, v.n_inputs, 6), dtype=np.uint64), np.zeros((0, 72), dtype=np.uint64))) == []
    v.free()


def test_golden_small_proof_and_every_tampering(zk):
    g = golden("groth16_small.json")
    vk = _vk(g["vk"])
    z = [h2i(x) for x in g["z"]]
    inputs = np.array([fr_limbs(x) for x in z[1:1 + g["n_primary"]]])
    proof = _proof(g["proof"])
    cases, expect = [(inputs, proof)], [True]
    for i in range(g["n_primary"]):
        bad = inputs.copy(); bad[i] = fr_limbs((z[1 + i] + 1) % R.R_MOD)
        cases.append((bad, proof)); expect.append(False)
    badp = proof.copy(); badp[48:] = proof[:24]                                   # C := A
    cases.append((inputs, badp)); expect.append(False)
    for lo in (0, 24, 48):                                                         # A, B or C at infinity
        badp = proof.copy(); badp[lo:lo + 24] = 0
        cases.append((inputs, badp)); expect.append(False)
    v = zk.Verifier(vk)
    got = list(v.verify_batch([c[0] for c in cases], [c[1] for c in cases]))
    v.free()
    assert got == [zk.groth16_verify(vk, i, p) for i, p in cases]
    assert got == expect


# ---------------------------------------------------------------- (e), (f) mixed batches, several handles
_HOST = {}


def _host_verdict(zk, vkl, n_inputs, inp, prf):
    key = (n_inputs, inp.tobytes(), prf.tobytes())
    if key not in _HOST:
        _HOST[key] = zk.groth16_verify(vkl, inp, prf)
    return _HOST[key]


def _mixed_batch(n_inputs, count, seed):
    """count statements cycling through the eight valid ones of this key; invalid ones (an input bumped; without inputs C := A)
    at the first, the last and a few pseudo-random positions.  Returns (inputs, proofs, invalid positions)."""
    vk, proofs = V.statements(n_inputs)
    assert len(proofs) >= 8
    rng = random.Random(seed)
    invalid = {0, count - 1} | {rng.randrange(count) for _ in range(count // 4)}
    inputs, prfs = [], []
    for j in range(count):
        proof, xs = proofs[j % len(proofs)]
        xs, pl = list(xs), V.proof_limbs(proof)
        if j in invalid:
            if n_inputs:
                i = rng.randrange(n_inputs)
                xs[i] = (xs[i] + 1 + j) % R.R_MOD
            else:
                pl[48:] = pl[:24]
        inputs.append(V.input_limbs(xs)); prfs.append(pl)
    return np.array(inputs).reshape(count, n_inputs, 6), np.array(prfs), invalid


@pytest.mark.parametrize("count", [G + 1, WG + 1])
def test_mixed_batches_on_two_handles(zk, count):
    keys = {n: V.vk_limbs(V.statements(n)[0]) for n in (0, 5)}
    handles = {n: zk.Verifier(keys[n]) for n in (0, 5)}
    batches = {n: _mixed_batch(n, count, 100 * count + n) for n in (0, 5)}
    want = {}
    for n, (inp, prf, invalid) in batches.items():
        want[n] = [_host_verdict(zk, keys[n], n, inp[j], prf[j]) for j in range(count)]
        assert want[n] == [j not in invalid for j in range(count)]
    for n in (0, 5, 0, 5):                                     # the two handles interleaved, each batch twice on the same handle
        inp, prf, _ = batches[n]
        assert list(handles[n].verify_batch(inp, prf)) == want[n], n
    for h in handles.values():
        h.free()


def test_chunk_boundary_of_the_per_proof_route(zk):
    """VERIFIER_CHUNK + 1 proofs (a second chunk of one proof: its staging, inputs and verdict start at an offset), tampered at the
    first position and on both sides of the boundary: False at exactly those three, True everywhere else."""
    from tests import combine_fixtures as C
    n, chunk = 4, zk.VERIFIER_CHUNK
    inp, prf, ks = C.batch(n, chunk + 1, {0: 1, chunk - 1: 1, chunk: 1})
    v = zk.Verifier(V.vk_limbs(V.statements(n)[0]))
    try:
        got = np.asarray(v.verify_batch(inp, prf))
    finally:
        v.free()
    assert got.shape == (chunk + 1,) and got.dtype == np.bool_
    assert np.flatnonzero(~got).tolist() == [0, chunk - 1, chunk] == [j for j, k in enumerate(ks) if k]


def test_two_verifier_threads_beside_a_prover(zk):
    g = golden("groth16_small.json")
    pts = lambda L: np.array([aff_limbs(pt_from_json(p)) for p in L]).reshape(-1, 24)
    pk = {k: (aff_limbs(pt_from_json(v)) if k in ("alpha_g1", "beta_g1", "beta_g2", "delta_g1", "delta_g2") else pts(v))
          for k, v in g["pk"].items()}
    A, B, C = (csr_from_rows(g[k]) for k in "ABC")
    z = fr_array([h2i(x) for x in g["z"]])
    crs = zk.Crs(pk, len(g["z"]), g["n_primary"], 1 << g["log_d"])
    desc, keep = zk.make_r1cs_desc(A, B, C, len(g["z"]), g["n_primary"])      # (keep: the arrays the descriptor points into)
    prover = zk.Prover(crs, desc)
    count = G + 1
    keys = {n: V.vk_limbs(V.statements(n)[0]) for n in (0, 5)}
    batches = {n: _mixed_batch(n, count, 100 * count + n) for n in (0, 5)}
    out, errs = {}, []

    def verify(n):
        try:
            v = zk.Verifier(keys[n])
            out[n] = [list(v.verify_batch(batches[n][0], batches[n][1])) for _ in range(2)]
            v.free()
        except Exception as e:          # noqa: BLE001 - reported by the main thread
            errs.append(e)

    def prove():
        try:
            out["proof"] = [prover.prove(z, fr_limbs(h2i(g["r"])), fr_limbs(h2i(g["s"]))) for _ in range(3)]
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=verify, args=(0,)), threading.Thread(target=verify, args=(5,)), threading.Thread(target=prove)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for n in (0, 5):
        want = [j not in batches[n][2] for j in range(count)]
        assert out[n] == [want, want]
    for proof in out["proof"]:
        assert aff_point(proof[:24]) == pt_from_json(g["proof"]["a"])
        assert aff_point(proof[24:48]) == pt_from_json(g["proof"]["b"])
        assert aff_point(proof[48:]) == pt_from_json(g["proof"]["c"])
    prover.free(); crs.free()
