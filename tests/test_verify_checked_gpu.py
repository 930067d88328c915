"""Checked batches of the GPU verifier (zkhip_verifier_new_checked / _verify_batch_checked: k_point_check in front of the pairing kernels
of zecale_amd/csrc/pairing.hip) against the host route they are pinned on (zkhip_groth16_verify_checked) and the status bytes
tests/point_check_fixtures.py computes from pyref: valid statements, batches in which refused proofs sit at the first, the last and
middle positions among valid and pairing-rejected ones, agreement with the unchecked route, key validation on the device, two handles
of two keys, and the reference's own fixtures.  G = 8 verifications share a wave and WG = 16 a workgroup: the batch sizes 1, G + 1 and
WG + 1 sit on both sides of either."""
import numpy as np
import pytest

from tests import point_check_fixtures as F
from tests import verify_fixtures as V
from tests.helpers import aff_limbs, fr_limbs, golden, h2i, pt_from_json

pytestmark = pytest.mark.gpu

G, WG = 8, 16
COUNTS = (1, G + 1, WG + 1)


@pytest.fixture(scope="module")
def handles(zk):
    """one checked and one unchecked handle per key (no inputs, five inputs), shared by the tests of this file"""
    keys = {n: V.vk_limbs(V.statements(n)[0]) for n in (0, 5)}
    h = {n: (zk.Verifier(keys[n], checked=True), zk.Verifier(keys[n])) for n in (0, 5)}
    yield keys, h
    for pair in h.values():
        for v in pair:
            v.free()


_HOST = {}


def _host_byte(zk, vkl, n_inputs, case):
    key = (n_inputs, case.inputs.tobytes(), case.proof.tobytes())
    if key not in _HOST:
        _HOST[key] = zk.groth16_verify_checked(vkl, case.inputs, case.proof)
    return _HOST[key]


def _run(v, cases):
    codes, masks = v.verify_batch_checked(np.array([c.inputs for c in cases]).reshape(len(cases), v.n_inputs, 6), np.array([c.proof for c in cases]))
    assert codes.dtype == np.uint8 and masks.dtype == np.uint8 and codes.shape == masks.shape == (len(cases),)
    assert not (codes & 0xF0).any() and not (masks & 0x0F).any()
    return [int(c | m) for c, m in zip(codes, masks)]


def _compose(n_inputs, count, refused):
    """Batches of `count` proofs that use up `refused`: refused proofs at the first position, the last, the middle one and then every
    fourth in between, the valid statements of the key around them, every third of those with a bumped input (rejected by the pairing)."""
    order = list(dict.fromkeys([0, count - 1, count // 2] + list(range(4, count - 1, 4))))
    refused, batches, k = list(refused), [], 0
    while refused:
        take = {pos: refused.pop(0) for pos in order[:len(refused)]}
        batch = []
        for pos in range(count):
            if pos in take:
                batch.append(take[pos])
            else:
                batch.append(F.make_case(n_inputs, k, bump=k % 3 == 1))
                k += 1
        batches.append(batch)
    return batches


@pytest.mark.parametrize("n_inputs", [0, 5])
def test_valid_statements_are_accepted(zk, handles, n_inputs):
    checked = handles[1][n_inputs][0]
    for count in COUNTS:
        assert _run(checked, [F.make_case(n_inputs, j) for j in range(count)]) == [F.ACCEPT] * count, count
    codes, masks = checked.verify_batch_checked(np.zeros((0, n_inputs, 6), dtype=np.uint64), np.zeros((0, 72), dtype=np.uint64))
    assert len(codes) == 0 and len(masks) == 0


@pytest.mark.parametrize("group", ["a", "b", "c", "inputs", "mixed"])
@pytest.mark.parametrize("count", COUNTS)
def test_mixed_batches(zk, handles, count, group):
    """Every fixture in the slot `group` names (under "mixed": two failure classes in one proof, several elements of one class), refused
    proofs first, last and in the middle of batches of valid and pairing-rejected ones: the status byte of every proof is the host
    route's and pyref's, so a refused neighbour changes nothing for a valid proof; and the proofs nothing refuses get the same
    verdict from the unchecked route."""
    n = 5
    keys, h = handles
    checked, unchecked = h[n]
    passed = []
    for batch in _compose(n, count, F.refused_cases(n)[group]):
        got = _run(checked, batch)
        for pos, (case, st) in enumerate(zip(batch, got)):
            assert st == _host_byte(zk, keys[n], n, case) == case.want, (count, pos, case.label, hex(st), hex(case.want))
        assert {F.ACCEPT, F.REJECT} <= set(got) or count == 1
        passed += [(case, st) for case, st in zip(batch, got) if st <= F.REJECT]
    if passed:                                                   # only these meet the unchecked route's preconditions
        ok = unchecked.verify_batch(np.array([c.inputs for c, _ in passed]), np.array([c.proof for c, _ in passed]))
        assert list(ok) == [st == F.ACCEPT for _, st in passed]


def test_a_point_at_infinity_passes_the_checks(zk, handles):
    """the all-zero point is in the group: the pairing decides, as on the host"""
    keys, h = handles
    for n in (0, 5):
        cases = [F.make_case(n, 1, {"a": F.point_elem("infinity", None, False)}, label="A at infinity"),
                 F.make_case(n, 2), F.make_case(n, 3, {"b": F.point_elem("infinity", None, True)}, label="B at infinity")]
        got = _run(h[n][0], cases)
        assert got == [_host_byte(zk, keys[n], n, c) for c in cases] == [F.REJECT, F.ACCEPT, F.REJECT]


def test_chunk_boundary_of_the_checked_route(zk, handles):
    """VERIFIER_CHUNK + 1 proofs on the checked five-input handle: a tampered but well-formed proof is the last of the first chunk, a
    refused one (an input >= r) the only proof of the second - its inputs and its codes are read at the chunk's offset.  REJECT and
    the refusal byte at exactly those positions, ACCEPT for every other proof."""
    from tests import combine_fixtures as C
    chunk = zk.VERIFIER_CHUNK
    refused = F.refused_cases(5)["inputs"][0]
    inp, prf, _ = C.batch(5, chunk + 1, {chunk - 1: 1})
    inp[chunk], prf[chunk] = refused.inputs, refused.proof
    codes, masks = handles[1][5][0].verify_batch_checked(inp, prf)
    got = codes | masks
    want = np.full(chunk + 1, F.ACCEPT, dtype=np.uint8)
    want[chunk - 1], want[chunk] = F.REJECT, refused.want
    assert refused.want == F.ENCODING | F.MASK["inputs"]
    assert got.shape == want.shape and np.flatnonzero(got != want).tolist() == []


def test_two_checked_handles_of_two_keys_interleaved(zk):
    """each batch twice on its handle, the handles taking turns: nothing of a flagged batch stays behind in a handle's work space"""
    keys = {n: V.vk_limbs(V.statements(n)[0]) for n in (0, 5)}
    hs = {n: zk.Verifier(keys[n], checked=True) for n in (0, 5)}
    batches = {}
    for n in (0, 5):
        r = F.refused_cases(n)
        batches[n] = [_compose(n, WG + 1, r["mixed"][:3] + r["b"][:2])[0], _compose(n, G + 1, r["a"][:1] + r["c"][5:7])[0]]
    want = {n: [[c.want for c in b] for b in batches[n]] for n in (0, 5)}
    for n in (0, 5, 0, 5):
        for b, w in zip(batches[n], want[n]):
            assert _run(hs[n], b) == w, n
    # a batch of valid statements straight after flagged ones of the same size
    for n in (0, 5):
        assert _run(hs[n], [F.make_case(n, j) for j in range(G + 1)]) == [F.ACCEPT] * (G + 1)
        hs[n].free()


def test_keys_are_validated_on_the_device(zk, handles):
    for name, code, vkl in F.bad_keys(1):
        with pytest.raises(zk.ZkhipError) as err:
            zk.Verifier(vkl, checked=True)
        assert err.value.code == -1                              # ZKHIP_ERR_ARG
        assert name + ":" in str(err.value) and "(%d)" % code in str(err.value), str(err.value)
        zk.Verifier(vkl).free()                                  # the unchecked constructor is what it was (nothing is run on this key)
    good = zk.Verifier(V.vk_limbs(V.statements(1)[0]), checked=True)
    assert _run(good, [F.make_case(1, 0)]) == [F.ACCEPT]
    good.free()
    unchecked = handles[1][0][1]
    case = F.make_case(0, 0)
    with pytest.raises(zk.ZkhipError) as err:
        unchecked.verify_batch_checked([case.inputs], [case.proof])
    assert err.value.code == -4                                  # ZKHIP_ERR_STATE


def test_reference_fixtures(zk):
    j = golden("dummy_app/aggregator_vk.json")
    vk = dict(alpha=aff_limbs(pt_from_json(j["alpha"])), beta=aff_limbs(pt_from_json(j["beta"])), delta=aff_limbs(pt_from_json(j["delta"])),
              ABC=np.array([aff_limbs(pt_from_json(p)) for p in j["ABC"]]))
    st = {}
    for name in ("batch1.json", "batch1-invalid.json"):
        ep = golden("dummy_app/" + name)["ext_proof"]
        st[name] = (np.array([fr_limbs(h2i(x)) for x in ep["inputs"]]),
                    np.concatenate([aff_limbs(pt_from_json(ep["proof"][k])) for k in "abc"]))
    v = zk.Verifier(vk, checked=True)
    good, bad = st["batch1.json"], st["batch1-invalid.json"]
    for inputs, proofs, want in (([good[0]], [good[1]], [0]), ([bad[0]], [bad[1]], [1]), ([bad[0], good[0]], [bad[1], good[1]], [1, 0])):
        codes, masks = v.verify_batch_checked(inputs, proofs)
        assert list(codes) == want and not masks.any()
        assert [zk.groth16_verify_checked(vk, i, p) for i, p in zip(inputs, proofs)] == want
    v.free()
