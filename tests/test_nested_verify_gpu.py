"""Nested (BLS12-377) Groth16 verification in batches on the GPU (zkhip_nested_verifier: the kernels of zecale_amd/csrc/pairing_bls.hip)
against the host verifier it is pinned on (zkhip_bls12_377_groth16_verify) and Python big integers: the Fq12 lane bodies inside a real
kernel, reduced GT values limb for limb, the reference's nested fixtures, mixed batches of trapdoor statements, the wrapping circuit's
result bits, off-curve and degenerate proofs, handles beside each other and beside a prover, and the screening server.
G = 4 verifications share a wave and WG = 8 a workgroup: the batch sizes sit on both sides of either."""
import random
import threading

import numpy as np
import pytest

from oracle import pyref as R
from tests import nested_verify_fixtures as N
from tests.helpers import aff_limbs, aff_point, csr_from_rows, fr_array, fr_int, fr_limbs, golden, h2i, pt_from_json

pytestmark = pytest.mark.gpu

G, WG, CHUNK = 4, 8, 8192
OPS = ["mul", "sqr", "mul_line"]


def test_group_sizes(zk):
    assert (zk.NESTED_VERIFIER_GROUP, zk.NESTED_VERIFIER_WORKGROUP, zk.NESTED_VERIFIER_CHUNK) == (G, WG, CHUNK)


# ---------------------------------------------------------------- 1. the lane bodies in a kernel
@pytest.mark.parametrize("op", OPS)
def test_fq12_lane_bodies_in_a_kernel(zk, op):
    cases = N.fq12_cases()
    want = [N.fq12_expected(op, a, b) for a, b in cases]
    for n in (1, G, G + 1, WG + 1):
        idx = [(i * 5 + n) % len(cases) for i in range(n)]          # every case but two appears at n = WG + 1; the sets of a group differ
        got = zk.fq12_selftest(op, np.array([N.fq12_limbs(cases[i][0]) for i in idx]), np.array([N.fq12_limbs(cases[i][1]) for i in idx]))
        for row, i in zip(got, idx):
            assert N.fq12_ints(row) == want[i], (op, n, i)
    idx = [4, 6, 10]                                                 # ... and the two it leaves out, with the all-(q - 1) case
    got = zk.fq12_selftest(op, np.array([N.fq12_limbs(cases[i][0]) for i in idx]), np.array([N.fq12_limbs(cases[i][1]) for i in idx]))
    assert [N.fq12_ints(row) for row in got] == [want[i] for i in idx]


# ---------------------------------------------------------------- 2. reduced GT values
def _both_routes(zk, products):
    """products: list of lists of (P, Q) of one length -> (GPU values, host values), each count x 12 x 6 limbs"""
    g1 = np.array([[N.g1_limbs(P) for P, _ in pr] for pr in products], dtype=np.uint64)
    g2 = np.array([[N.g2_limbs(Q) for _, Q in pr] for pr in products], dtype=np.uint64)
    return zk.nested_pairing_product("gpu", g1, g2), zk.nested_pairing_product("host", g1, g2)


@pytest.fixture(scope="module")
def gt_base(zk):
    g1, g2 = N.pair_limbs([(R.BLS_G1_GEN, R.BLS_G2_GEN)])
    e = N.fq12_ints(zk.nested_pairing_product("host", g1, g2)[0])
    assert e != N.EXT.one() and N.EXT.pow(e, R.BLS_R) == N.EXT.one()
    return e


def test_pairing_of_the_generators_and_bilinearity(zk, gt_base):
    rng = random.Random(5)
    for u, v in [(1, 1), (2, 3), (R.BLS_R - 1, 5), (rng.randrange(1, R.BLS_R), rng.randrange(1, R.BLS_R))]:
        gpu, host = _both_routes(zk, [[(N.g1mul(u), N.g2mul(v))]])
        assert (gpu == host).all(), (u, v)
        assert N.fq12_ints(gpu[0]) == N.EXT.pow(gt_base, u * v % R.BLS_R), (u, v)       # e(uP, vQ) = e(P, Q)^(uv)


def test_products_of_a_valid_statement(zk):
    vk, proofs = N.golden_statement(3)
    four = N.verification_pairs(vk, *proofs[0])
    gpu, host = _both_routes(zk, [four])
    assert (gpu == host).all() and N.fq12_ints(gpu[0]) == N.EXT.one()
    gpu, host = _both_routes(zk, [[pq] for pq in four])              # each of its pairs alone
    assert (gpu == host).all()
    assert all(N.fq12_ints(row) != N.EXT.one() for row in gpu)


@pytest.mark.parametrize("count", [G + 1, WG + 1])
def test_two_pair_products_differ_at_every_position(zk, gt_base, count):
    """product i = e(u_i P, Q) e(P, v_i Q) = e(P, Q)^(u_i + v_i): other points at every position of the groups and workgroups"""
    uv = [(i + 2, 3 * i + 1) for i in range(count)]
    gpu, host = _both_routes(zk, [[(N.g1mul(u), R.BLS_G2_GEN), (R.BLS_G1_GEN, N.g2mul(v))] for u, v in uv])
    assert (gpu == host).all()
    for row, (u, v) in zip(gpu, uv):
        assert N.fq12_ints(row) == N.EXT.pow(gt_base, u + v)


def test_off_curve_points_are_refused_on_both_routes(zk):
    g1, g2 = N.pair_limbs([(R.BLS_G1_GEN, R.BLS_G2_GEN)])
    bad1 = g1.copy(); bad1[0, 0, :6] = N.fl(N.fint(g1[0, 0, :6]) + 1)
    bad2 = g2.copy(); bad2[0, 0, 18:] = N.fl(N.fint(g2[0, 0, 18:]) + 1)
    for route in ("host", "gpu"):
        for a, b in ((bad1, g2), (g1, bad2)):
            with pytest.raises(zk.ZkhipError) as e:
                zk.nested_pairing_product(route, a, b)
            assert e.value.code == -1


# ---------------------------------------------------------------- 3. the reference's fixtures
def _bumped(xs, i=0):
    bad = list(xs)
    bad[i] = (bad[i] + 1) % R.BLS_R
    return bad


def _arrays(items):
    """[(proof, inputs)] -> (inputs limbs, proofs limbs)"""
    k = len(items[0][1])
    return (np.array([N.input_limbs(xs) for _, xs in items], dtype=np.uint64).reshape(len(items), k, 6),
            np.array([N.proof_limbs(pr) for pr, _ in items], dtype=np.uint64))


def _host_verdicts(zk, vkl, items):
    return [zk.bls12_377_groth16_verify(vkl, N.input_limbs(xs), N.proof_limbs(pr)) for pr, xs in items]


def test_reference_fixtures(zk):
    """extproof1..6.json under vk.json: accepted; rejected with the input bumped; good and bad interleaved in both orders; an empty batch."""
    vk, proofs = N.dummy_app()
    v = zk.NestedVerifier(N.vk_limbs(vk), 1)
    assert v.n_inputs == 1
    try:
        assert v.verify_batch(*_arrays(proofs)).all() and v.last_fallbacks() == 0
        bad = [(pr, _bumped(xs)) for pr, xs in proofs]
        assert not v.verify_batch(*_arrays(bad)).any() and v.last_fallbacks() == 0
        for first in (0, 1):
            mixed = [(proofs if (i + first) % 2 == 0 else bad)[i] for i in range(6)]
            assert list(v.verify_batch(*_arrays(mixed))) == [(i + first) % 2 == 0 for i in range(6)]
        empty = v.verify_batch(np.zeros((0, 1, 6), dtype=np.uint64), np.zeros((0, 48), dtype=np.uint64))
        assert empty.shape == (0,) and v.last_fallbacks() == 0
    finally:
        v.free()


# ---------------------------------------------------------------- 4. mixed batches of trapdoor statements
def _mixed_batch(k, count, seed):
    """count statements under the key of N.statements(k); invalid ones (an input bumped, or C := A where there are no inputs) at the first
    position, the last, and a quarter of the rest pseudo-randomly.  Returns (items, set of invalid positions)."""
    _, proofs = N.statements(k)
    rng = random.Random(seed)
    invalid = {0, count - 1} | {j for j in range(count) if rng.random() < 0.25}
    items = []
    for j in range(count):
        pr, xs = proofs[j % len(proofs)]
        if j in invalid:
            pr, xs = (pr, _bumped(xs, rng.randrange(k))) if k else (dict(pr, c=pr["a"]), xs)
        items.append((pr, xs))
    return items, invalid


@pytest.mark.parametrize("k", [0, 3])
def test_mixed_batches_twice_and_on_two_handles(zk, k):
    vkl = N.vk_limbs(N.statements(k)[0])
    batches = {count: _mixed_batch(k, count, 10 * count + k) for count in (G + 1, WG + 1)}
    for count, (items, invalid) in batches.items():
        want = [j not in invalid for j in range(count)]
        assert _host_verdicts(zk, vkl, items) == want                # the host function agrees with the construction
    v1, v2 = zk.NestedVerifier(vkl, k), zk.NestedVerifier(vkl, k)
    try:
        for rnd in range(2):                                         # the same batches twice, interleaved on two handles
            for count, (items, invalid) in batches.items():
                want = [j not in invalid for j in range(count)]
                for v in (v1, v2):
                    assert list(v.verify_batch(*_arrays(items))) == want, (k, count, rnd)
                    assert v.last_fallbacks() == 0                   # a batch that silently went through the host would pass the rest
    finally:
        v1.free(); v2.free()


def test_chunk_boundary(zk):
    """CHUNK + 1 proofs under the three-input key (a second chunk of one proof: its proof, inputs and both status bytes sit at the chunk's
    offset), the ten statements repeated by indexing their limb arrays; an input bumped at the first position and on both sides of the
    boundary.  False at exactly those three, and nothing went to the host."""
    vk, proofs = N.statements(3)
    base_in, base_pr = _arrays(proofs)
    bad_in, _ = _arrays([(pr, _bumped(xs)) for pr, xs in proofs])
    idx = np.arange(CHUNK + 1) % len(proofs)
    inp, prl = base_in[idx], base_pr[idx]
    invalid = [0, CHUNK - 1, CHUNK]
    inp[invalid] = bad_in[idx[invalid]]
    v = zk.NestedVerifier(N.vk_limbs(vk), 3)
    try:
        got = np.asarray(v.verify_batch(inp, prl))
        assert v.last_fallbacks() == 0
    finally:
        v.free()
    assert got.shape == (CHUNK + 1,) and np.flatnonzero(~got).tolist() == invalid


# ---------------------------------------------------------------- 5. nine inputs
def test_nine_inputs_once(zk):
    vk, proofs = N.golden_statement(9)
    pr, xs = proofs[0]
    items = [(pr, xs), (pr, _bumped(xs, 0)), (proofs[1][0], proofs[1][1]), (pr, _bumped(xs, 4)), (pr, _bumped(xs, 8)), (proofs[2][0], proofs[2][1])]
    v = zk.NestedVerifier(N.vk_limbs(vk), 9)
    try:
        assert list(v.verify_batch(*_arrays(items))) == [True, False, True, False, False, True] and v.last_fallbacks() == 0
    finally:
        v.free()


# ---------------------------------------------------------------- 6. agreement with the wrapping circuit
def test_verdicts_are_the_circuits_result_bits(zk):
    """For nested_k3.json, the verdicts of (proof 0, proof 1) under the four bump patterns equal the bits of the packed-result primary
    input of the wrapping circuit's assignment (host generator): 3, 2, 1, 0."""
    vk, proofs = N.golden_statement(3)
    vkl = N.vk_limbs(vk)
    agg = zk.AggregatorCircuit(2, 3)
    v = zk.NestedVerifier(vkl, 3)
    try:
        for packed, bump in ((3, ()), (2, (0,)), (1, (1,)), (0, (0, 1))):
            items = [(proofs[p][0], _bumped(proofs[p][1], 1) if p in bump else proofs[p][1]) for p in (0, 1)]
            inp, prl = _arrays(items)
            z = agg.witness(vkl, prl.reshape(-1), inp.reshape(-1, 6))
            assert fr_int(z[2]) == packed
            got = v.verify_batch(inp, prl)
            assert sum(int(b) << i for i, b in enumerate(got)) == packed and v.last_fallbacks() == 0
    finally:
        v.free(); agg.free()


# ---------------------------------------------------------------- 7. off-curve proof points
def test_off_curve_proof_points(zk):
    """A, B or C with one coordinate + 1: verdict 0 as on the host route, the neighbours unaffected, nothing handed to the host; so for
    the all-zero encoding (the nested format has no point at infinity)."""
    vk, proofs = N.statements(3)
    vkl = N.vk_limbs(vk)
    inp, prl = _arrays(proofs[:G + 1])
    bad = prl.copy()
    for j, at in ((0, 6), (2, 12), (2, 30), (4, 36)):                # A.y of proof 0, B.x.c0 and B.y.c1 of proof 2, C.x of proof 4
        bad[j, at:at + 6] = N.fl(N.fint(prl[j, at:at + 6]) + 1)
    bad[3, 12:36] = 0                                                # B of proof 3 all zero
    v = zk.NestedVerifier(vkl, 3)
    try:
        got = list(v.verify_batch(inp, bad))
        assert got == [False, True, False, False, False] and v.last_fallbacks() == 0
        assert got == [zk.bls12_377_groth16_verify(vkl, inp[j], bad[j]) for j in range(G + 1)]
    finally:
        v.free()


# ---------------------------------------------------------------- 8. the degenerate statement
@pytest.mark.parametrize("x,negated,host_accepts", [(4, False, False), (8, False, True), (8, True, False)])
def test_degenerate_statement_goes_to_the_host(zk, x, negated, host_accepts):
    """A statement, valid by the group law, on which the host's affine accumulator meets +-2^2 ABC_1 at step 2 - at a set bit (x = 4, the
    plan's statement: the host's chord of a point with itself is not its double, and it rejects) or at a clear one (x = 8: the same point, which the host happens to accept, and under the negated key the negative,
    which it rejects) - at position 0, the middle and the last of a batch of G + 1 among ordinary proofs of the same key, two of them
    valid and one with a wrong input: verdicts equal the host function's, the ordinary ones' the construction's, and last_fallbacks()
    is exactly the number placed."""
    vk, pr, xs = N.degenerate_statement(x, negated)
    vkl = N.vk_limbs(vk)
    ordinary = [N.degenerate_statement(3, negated)[1:], N.degenerate_statement(5, negated)[1:], (N.degenerate_statement(3, negated)[1], [6])]
    host = _host_verdicts(zk, vkl, [(pr, xs)] + ordinary)
    assert host[1:] == [True, True, False]
    assert host[0] == host_accepts
    v = zk.NestedVerifier(vkl, 1)
    try:
        for places in ((0,), (2,), (G,), (0, 2, G)):
            got = list(v.verify_batch(*_arrays([(pr, xs) if j in places else ordinary[j % 3] for j in range(G + 1)])))
            assert got == [host[0] if j in places else host[1 + j % 3] for j in range(G + 1)], places
            assert v.last_fallbacks() == len(places)
        assert list(v.verify_batch(*_arrays(ordinary))) == host[1:] and v.last_fallbacks() == 0
    finally:
        v.free()


# ---------------------------------------------------------------- 9. handles beside each other and beside a prover
def test_two_nested_verifier_threads_and_a_verifier_beside_a_prover(zk):
    from tests import verify_fixtures as V
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
    batches = {k: _mixed_batch(k, count, 100 * count + k) for k in (0, 3)}
    wvk, wproofs = V.statements(0)
    out, errs = {}, []

    def nested(k):
        try:
            v = zk.NestedVerifier(N.vk_limbs(N.statements(k)[0]), k)
            out[k] = [(list(v.verify_batch(*_arrays(batches[k][0]))), v.last_fallbacks()) for _ in range(2)]
            v.free()
        except Exception as e:          # noqa: BLE001 - reported by the main thread
            errs.append(e)

    def wrapping():
        try:
            v = zk.Verifier(V.vk_limbs(wvk))
            prl = np.array([V.proof_limbs(p) for p, _ in wproofs[:count]])
            out["w"] = list(v.verify_batch(np.zeros((count, 0, 6), dtype=np.uint64), prl))
            v.free()
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    def prove():
        try:
            out["proof"] = [prover.prove(z, fr_limbs(h2i(g["r"])), fr_limbs(h2i(g["s"]))) for _ in range(3)]
        except Exception as e:          # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=nested, args=(0,)), threading.Thread(target=nested, args=(3,)), threading.Thread(target=wrapping),
               threading.Thread(target=prove)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for k in (0, 3):
        want = [j not in batches[k][1] for j in range(count)]
        assert out[k] == [(want, 0), (want, 0)]
    assert out["w"] == [True] * count
    for proof in out["proof"]:
        assert aff_point(proof[:24]) == pt_from_json(g["proof"]["a"])
        assert aff_point(proof[24:48]) == pt_from_json(g["proof"]["b"])
        assert aff_point(proof[48:]) == pt_from_json(g["proof"]["c"])
    prover.free(); crs.free()


# ---------------------------------------------------------------- 10. the screening server
def test_screening_server_drops_the_invalid_transaction(zk, tmp_path):
    """A live serve(GpuProver(screen_nested=True)): one valid and one input-bumped dummy-app transaction plus enough valid ones to fill a
    batch.  The aggregated transaction carries only valid ones with both result bits set, and the drop counter is 1."""
    import json
    from zecale_amd import encoding as E
    from zecale_amd import server as S
    prover = S.GpuProver(str(tmp_path / "zecale_keypair.bin"), device=0, gpu_slots=2, witness_workers=2, screen_nested=True)
    server, port, service = S.serve(prover, "127.0.0.1:0", max_workers=4)
    try:
        client = S.AggregatorClient("127.0.0.1:%d" % port)
        vk = E.verification_key_from_json(client.get_verification_key())
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        txs = {k: golden("dummy_app/extproof%d.json" % k) for k in (1, 2, 3)}
        bad = json.loads(json.dumps(txs[1]))                          # the highest fee, its input 7 bumped to 8
        bad["extended_proof"]["inputs"] = txs[2]["extended_proof"]["inputs"]
        client.submit_nested_transaction(bad)
        client.submit_nested_transaction(txs[2])
        client.submit_nested_transaction(txs[3])
        batch = client.get_aggregated_transaction("dummy_app")
        _, proof, inputs, params = E.aggregated_transaction_from_json(batch)
        assert zk.groth16_verify(vk, inputs, proof)
        assert [fr_int(x) for x in inputs[1:]] == [3, 8, 9]          # both result bits set; the inputs of extproof2 and extproof3
        assert service.screen_dropped == 1 and service.pools["dummy_app"].tx_pool_size() == 0
    finally:
        server.stop(0)
        prover.close()
