"""Checked batches of the nested GPU verifier (zkhip_nested_verifier_new_checked / _verify_batch_checked: k_nested_point_check in front
of the pairing kernels of zecale_amd/csrc/pairing_bls.hip) against the host route they are pinned on
(zkhip_bls12_377_groth16_verify_checked) and the status bytes tests/nested_point_check_fixtures.py computes from Python integers: valid
statements, batches in which refused proofs sit at the first, the last and middle positions among valid and pairing-rejected ones,
agreement with the unchecked route, fallbacks, keys, two handles of two keys, the reference's own fixtures and the screening server.
G = 4 verifications share a wave of the pairing kernels and WG = 8 a workgroup; the check kernel puts one B point on a lane, so 65
proofs put one B lane into its second wave."""
import numpy as np
import pytest

from oracle import pyref as R
from tests import nested_point_check_fixtures as F
from tests import nested_verify_fixtures as N
from tests.helpers import fr_int, golden

pytestmark = pytest.mark.gpu

G, WG = 4, 8
COUNTS = (1, G + 1, WG + 1, 65)


@pytest.fixture(scope="module")
def handles(zk):
    """one checked and one unchecked handle per key (no inputs, three inputs), shared by the tests of this file"""
    keys = {n: N.vk_limbs(N.statements(n)[0]) for n in (0, 3)}
    h = {n: (zk.NestedVerifier(keys[n], n, checked=True), zk.NestedVerifier(keys[n], n)) for n in (0, 3)}
    yield keys, h
    for pair in h.values():
        for v in pair:
            v.free()


_HOST = {}


def _host_byte(zk, vkl, case):
    key = (vkl.tobytes(), case.inputs.tobytes(), case.proof.tobytes())
    if key not in _HOST:
        _HOST[key] = zk.bls12_377_groth16_verify_checked(vkl, case.inputs, case.proof)
    return _HOST[key]


def _arrays(v, cases):
    return np.array([c.inputs for c in cases]).reshape(len(cases), v.n_inputs, 6), np.array([c.proof for c in cases])


def _run(v, cases):
    codes, masks = v.verify_batch_checked(*_arrays(v, cases))
    assert codes.dtype == np.uint8 and masks.dtype == np.uint8 and codes.shape == masks.shape == (len(cases),)
    assert not (codes & 0xF0).any() and not (masks & 0x0F).any()
    return [int(c | m) for c, m in zip(codes, masks)]


def _compose(n_inputs, count, refused):
    """Batches of `count` proofs that use up `refused`: refused proofs at the first position, the last, the middle one and then every
    fourth in between, the valid statements of the key around them, every second of those in a batch with a bumped input (rejected by
    the pairing; G + 1 proofs with three refused ones leave two places: one accepted, one rejected)."""
    order = list(dict.fromkeys([0, count - 1, count // 2] + list(range(4, count - 1, 4))))
    refused, batches, k = list(refused), [], 0
    while refused:
        take = {pos: refused.pop(0) for pos in order[:len(refused)]}
        batch = []
        for pos in range(count):
            if pos in take:
                batch.append(take[pos])
            else:
                batch.append(F.make_case(n_inputs, k, bump=(pos - sum(1 for q in take if q < pos)) % 2 == 1))
                k += 1
        batches.append(batch)
    return batches


@pytest.mark.parametrize("n_inputs", [0, 3])
def test_valid_statements_are_accepted(zk, handles, n_inputs):
    checked = handles[1][n_inputs][0]
    for count in COUNTS:
        assert _run(checked, [F.make_case(n_inputs, j) for j in range(count)]) == [F.ACCEPT] * count, count
        assert checked.last_fallbacks() == 0
    codes, masks = checked.verify_batch_checked(np.zeros((0, n_inputs, 6), dtype=np.uint64), np.zeros((0, 48), dtype=np.uint64))
    assert len(codes) == 0 and len(masks) == 0


@pytest.mark.parametrize("group", ["a", "b", "c", "inputs", "mixed"])
@pytest.mark.parametrize("count", COUNTS)
def test_mixed_batches(zk, handles, count, group):
    """Every fixture in the slot `group` names (under "mixed": two failure classes in one proof, several elements of one class, a
    refused proof that is also a wrong statement), refused proofs first, last and in the middle of batches of valid and
    pairing-rejected ones: the status byte of every proof is the host route's and Python's, so a refused neighbour changes nothing for
    a valid proof; nothing goes to the host - not the cofactor B points either; and the proofs nothing refuses get the same verdict from
    the unchecked route."""
    n = 3
    keys, h = handles
    checked, unchecked = h[n]
    passed = []
    for batch in _compose(n, count, F.refused_cases(n)[group]):
        got = _run(checked, batch)
        assert checked.last_fallbacks() == 0
        for pos, (case, st) in enumerate(zip(batch, got)):
            assert st == _host_byte(zk, keys[n], case) == case.want, (count, pos, case.label, hex(st), hex(case.want))
        assert {F.ACCEPT, F.REJECT} <= set(got) or count == 1
        passed += [(case, st) for case, st in zip(batch, got) if st <= F.REJECT]
    if passed:                                                   # only these meet the unchecked route's preconditions
        ok = unchecked.verify_batch(*_arrays(unchecked, [c for c, _ in passed]))
        assert list(ok) == [st == F.ACCEPT for _, st in passed]


def test_chunk_boundary_of_the_checked_route(zk, handles):
    """NESTED_VERIFIER_CHUNK + 1 proofs under the three-input key, the ten statements repeated by indexing their limb arrays: a proof
    the pairing rejects is the last of the first chunk, a refused one (an input >= r) the only proof of the second, whose codes and
    status bytes are read at the chunk's offset.  REJECT and the refusal byte at exactly those positions, ACCEPT elsewhere, and
    nothing went to the host."""
    chunk = zk.NESTED_VERIFIER_CHUNK
    checked = handles[1][3][0]
    base_in, base_pr = _arrays(checked, [F.make_case(3, j) for j in range(10)])
    idx = np.arange(chunk + 1) % 10
    inp, prl = base_in[idx], base_pr[idx]
    rejected, refused = F.make_case(3, (chunk - 1) % 10, bump=True), F.refused_cases(3)["inputs"][0]
    inp[chunk - 1], prl[chunk - 1] = rejected.inputs, rejected.proof
    inp[chunk], prl[chunk] = refused.inputs, refused.proof
    codes, masks = checked.verify_batch_checked(inp, prl)
    assert checked.last_fallbacks() == 0
    want = np.full(chunk + 1, F.ACCEPT, dtype=np.uint8)
    want[chunk - 1], want[chunk] = F.REJECT, refused.want
    assert (rejected.want, refused.want) == (F.REJECT, F.ENCODING | F.MASK["inputs"])
    got = codes | masks
    assert got.shape == want.shape and np.flatnonzero(got != want).tolist() == []


def test_inputs_at_the_edge_of_the_scalar_field(zk, handles):
    """r - 1 and 0 are inputs like any other (the pairing rejects the statement); r, 2^253 - 1 and x + q on the limbs are refused"""
    keys, h = handles
    cases = F.fine_input_cases(3) + F.refused_cases(3)["inputs"]
    got = _run(h[3][0], cases)
    assert got == [c.want for c in cases] == [F.REJECT] * 2 + [F.ENCODING | 0x80] * 3
    assert got == [_host_byte(zk, keys[3], c) for c in cases]


def _deg_case(x, negated, proof=None, replace=None):
    vk, pr, xs = N.degenerate_statement(x, negated)
    pl = N.proof_limbs(proof or pr)
    for slot, e in (replace or {}).items():
        lo, hi = F.SLOT[slot]
        pl[lo:hi] = e.limbs
    return F.Case("degenerate key, x = %d" % xs[0], N.input_limbs(xs), pl, None)


@pytest.mark.parametrize("x,negated", [(4, False), (8, False), (8, True)])
def test_degenerate_statements_go_to_the_host_and_refused_ones_do_not(zk, x, negated):
    """Statements on which the host's affine accumulator meets a degenerate step, at positions 0, 2 and G among ordinary proofs of the
    key: the bytes are the host's, last_fallbacks() is the number placed; a refused proof at another position of the same batch - with
    the degenerate statement's own inputs, so that its accumulator lane meets the same step - is not counted."""
    vkl = N.vk_limbs(N.degenerate_statement(x, negated)[0])
    deg = _deg_case(x, negated)
    ordinary = [_deg_case(3, negated), _deg_case(5, negated)]
    refused = _deg_case(x, negated, replace={"a": F.bad_points(False)[3]})       # same inputs, A = generator + (-1, 0)
    host = {id(c): zk.bls12_377_groth16_verify_checked(vkl, c.inputs, c.proof) for c in [deg, refused] + ordinary}
    assert host[id(deg)] in (F.ACCEPT, F.REJECT) and host[id(refused)] == F.NOT_ORDER_R | 0x10
    assert [host[id(c)] for c in ordinary] == [F.ACCEPT, F.ACCEPT]
    v = zk.NestedVerifier(vkl, 1, checked=True)
    try:
        for places in ((0,), (2,), (G,), (0, 2, G)):
            batch = [deg if j in places else refused if j == 1 else ordinary[j % 2] for j in range(G + 1)]
            assert _run(v, batch) == [host[id(c)] for c in batch], places
            assert v.last_fallbacks() == len(places)
    finally:
        v.free()


def test_two_checked_handles_of_two_keys_interleaved(zk):
    """each batch twice on its handle, the handles taking turns: nothing of a flagged batch stays behind in a handle's work space"""
    keys = {n: N.vk_limbs(N.statements(n)[0]) for n in (0, 3)}
    hs = {n: zk.NestedVerifier(keys[n], n, checked=True) for n in (0, 3)}
    batches = {}
    for n in (0, 3):
        r = F.refused_cases(n)
        batches[n] = [_compose(n, WG + 1, r["mixed"][:3] + r["b"][:2])[0], _compose(n, G + 1, r["a"][:1] + r["c"][7:9])[0]]
    want = {n: [[c.want for c in b] for b in batches[n]] for n in (0, 3)}
    try:
        for n in (0, 3, 0, 3):
            for b, w in zip(batches[n], want[n]):
                assert _run(hs[n], b) == w, n
        # a batch of valid statements straight after flagged ones of the same size
        for n in (0, 3):
            assert _run(hs[n], [F.make_case(n, j) for j in range(G + 1)]) == [F.ACCEPT] * (G + 1)
    finally:
        for v in hs.values():
            v.free()


def test_keys(zk, handles):
    for name, code, vkl in F.bad_keys(1):
        with pytest.raises(zk.ZkhipError) as err:
            zk.NestedVerifier(vkl, 1, checked=True)
        assert err.value.code == -1                              # ZKHIP_ERR_ARG
        assert name + ":" in str(err.value) and "(%d)" % code in str(err.value), str(err.value)
        if code == F.NOT_ORDER_R:
            zk.NestedVerifier(vkl, 1).free()                     # the unchecked constructor is what it was: it takes this key
    good = zk.NestedVerifier(N.vk_limbs(N.statements(1)[0]), 1, checked=True)
    try:
        assert _run(good, [F.make_case(1, 0)]) == [F.ACCEPT]
        case = F.make_case(1, 0)                                 # a checked handle serves the unchecked call as well
        assert list(good.verify_batch(case.inputs.reshape(1, 1, 6), case.proof.reshape(1, 48))) == [True]
    finally:
        good.free()
    unchecked = handles[1][0][1]
    case = F.make_case(0, 0)
    with pytest.raises(zk.ZkhipError) as err:
        unchecked.verify_batch_checked(case.inputs.reshape(1, 0, 6), case.proof.reshape(1, 48))
    assert err.value.code == -4                                  # ZKHIP_ERR_STATE


def test_reference_fixtures(zk):
    """extproof1..6.json under vk.json: six ACCEPT; six REJECT with the input bumped"""
    vk, proofs = N.dummy_app()
    vkl = N.vk_limbs(vk)
    v = zk.NestedVerifier(vkl, 1, checked=True)
    try:
        good = [F.Case("extproof", N.input_limbs(xs), N.proof_limbs(pr), F.ACCEPT) for pr, xs in proofs]
        bad = [F.Case("bumped", N.input_limbs([(xs[0] + 1) % R.BLS_R]), N.proof_limbs(pr), F.REJECT) for pr, xs in proofs]
        assert _run(v, good) == [F.ACCEPT] * 6 and v.last_fallbacks() == 0
        assert _run(v, bad) == [F.REJECT] * 6 and v.last_fallbacks() == 0
        assert [_host_byte(zk, vkl, c) for c in good + bad] == [F.ACCEPT] * 6 + [F.REJECT] * 6
    finally:
        v.free()


def test_screening_server_counts_the_malformed_transaction(zk, tmp_path):
    """A live serve(GpuProver(screen_nested=True)): one dummy-app transaction whose A is a multiple of the generator plus (-1, 0) - on
    its curve, so the submission check lets it through; that is the point - one with a bumped input, and enough valid ones to fill a
    batch.  Both are dropped, one of them is counted as malformed and its entry carries NOT_ORDER_R | MASK_A."""
    import json
    from zecale_amd import encoding as E
    from zecale_amd import server as S
    prover = S.GpuProver(str(tmp_path / "zecale_keypair.bin"), device=0, gpu_slots=2, witness_workers=2, screen_nested=True)
    server, port, service = S.serve(prover, "127.0.0.1:0", max_workers=4)
    try:
        client = S.AggregatorClient("127.0.0.1:%d" % port)
        vk = E.verification_key_from_json(client.get_verification_key())
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        txs = {k: golden("dummy_app/extproof%d.json" % k) for k in (1, 2, 3, 4)}
        bumped = json.loads(json.dumps(txs[1]))                       # the highest fee, its input 7 bumped to 8
        bumped["extended_proof"]["inputs"] = txs[2]["extended_proof"]["inputs"]
        malformed = json.loads(json.dumps(txs[2]))
        not_in_g1 = R.ec_add(N.g1mul(12345), (R.BLS_Q - 1, 0), R.BLS_Q)
        assert R.on_curve(not_in_g1, R.BLS_G1_B, R.BLS_Q) and R.ec_mul(R.BLS_R, not_in_g1, R.BLS_Q) is not None
        malformed["extended_proof"]["proof"]["a"] = E.nested_g1_to_json(np.array(N.g1_limbs(not_in_g1), dtype=np.uint64))
        client.submit_nested_transaction(bumped)
        client.submit_nested_transaction(malformed)
        client.submit_nested_transaction(txs[3])
        client.submit_nested_transaction(txs[4])
        batch = client.get_aggregated_transaction("dummy_app")
        _, proof, inputs, params = E.aggregated_transaction_from_json(batch)
        assert zk.groth16_verify(vk, inputs, proof)
        assert [fr_int(x) for x in inputs[1:]] == [3, 9, 10]         # both result bits set; the inputs of extproof3 and extproof4
        assert service.screen_dropped == 2 and service.screen_malformed == 1 and service.pools["dummy_app"].tx_pool_size() == 0
        refused = service.pools["dummy_app"].screen_refused
        assert sorted(t["screen_status"] for t in refused) == [F.REJECT, F.NOT_ORDER_R | F.MASK["a"]]
    finally:
        server.stop(0)
        prover.close()
