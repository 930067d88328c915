"""zkhip_crs_check on the device against zkhip_crs_check_host (and the Python model) field by field: the cases of
tests/test_key_check_host.py, vectors of 1, 63, 64, 65 and 200 points with the chunk set to 64 through the hook - a refused point at
the last index of a chunk, the first index of the next and the last index of the vector: the tail lanes of a wave and the chunk seam -
and keys from zkhip_groth16_setup with the structure check against their own and against another system."""
import pytest

from tests import key_check_fixtures as K
from tests import point_check_fixtures as P
from tests.helpers import fr_limbs

pytestmark = pytest.mark.gpu

CASES = K.report_cases()
TRAPDOOR = (0x1234567, 0x2345678, 0x3456789, 0x456789a)


@pytest.fixture(scope="module")
def zkc(zk):
    """the library with the key check's chunk at 64 points"""
    zk.key_check_set_chunk(64)
    yield zk
    zk.key_check_set_chunk(0)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_device_report_equals_host_report(zkc, i):
    label, key, rho = CASES[i]
    host = K.check(zkc, key, list(rho), host=True)
    dev = K.check(zkc, key, list(rho), host=False)
    assert dev == host == K.model_report(key, rho), label


@pytest.fixture(scope="module")
def long_keys(zkc):
    return {n: K.gpu_key(zkc, n, n_primary=0 if n == 1 else 1) for n in (1, 63, 64, 65, 200)}


@pytest.mark.parametrize("n", (1, 63, 64, 65, 200))
def test_vector_lengths_around_the_chunk(zkc, long_keys, n):
    key = long_keys[n]
    rho = K.rho_for(n, seed=n)
    want = K.model_report(key, rho)
    assert want["ok"] == 1
    assert K.check(zkc, key, rho, host=False) == want == K.check(zkc, key, rho, host=True)
    # B-G2 of the last variable is another multiple: one term of n, in the last (partial) chunk
    wrong = key.replace("b_g2_query", n - 1, K.multiple(77, True))
    got = K.check(zkc, wrong, rho, host=False)
    assert got == K.model_report(wrong, rho) and got["pairs"] == 4


@pytest.mark.parametrize("n,index", ((65, 63), (65, 64), (200, 63), (200, 64), (200, 127), (200, 128), (200, 199), (64, 63), (63, 62), (1, 0)))
@pytest.mark.parametrize("name", ("a_query", "b_g2_query"))
def test_refused_point_at_the_chunk_seam(zkc, long_keys, n, index, name):
    key = long_keys[n]
    rho = K.rho_for(n, seed=n)
    bad = [K.refused(e) for e in P.bad_points(name in K.G2_ELEMENTS)]
    k = key.replace(name, index, bad[(n + index) % 8])
    got = K.check(zkc, k, rho, host=False)
    assert got == K.model_report(k, rho) and got["elements"][name][3] == index
    if index >= 64:          # a second refusal in an earlier chunk: the smaller index and ITS code are reported
        k2 = k.replace(name, 5, bad[(n + index + 3) % 8])
        got = K.check(zkc, k2, rho, host=False)
        assert got == K.model_report(k2, rho) and got["elements"][name][3:] == (5, bad[(n + index + 3) % 8].code)


def test_the_rule_chunk_gives_the_same_report(zk, long_keys):
    zk.key_check_set_chunk(0)
    try:
        key = long_keys[200].replace("h_query", 130, K.refused(P.bad_points(False)[3]))
        rho = K.rho_for(200, seed=200)
        assert K.check(zk, key, rho, host=False) == K.model_report(key, rho)
    finally:
        zk.key_check_set_chunk(64)


def _setup(zk, desc):
    return zk.Keypair(desc, *(fr_limbs(x) for x in TRAPDOOR))


def test_setup_key_of_the_small_golden_system_passes_with_its_system(zkc):
    key, cs = K.golden_small()
    desc = K.cs_desc(zkc, cs)
    kp = _setup(zkc, desc[0])
    try:
        rep = zkc.check_key(kp, r1cs=desc)
        f = rep.fields()
        assert f["ok"] == 1 and f["structure"] == 0 and f["pairs_evaluated"] == 7, rep.describe()
        assert f["elements"]["vk_abc"][0] == cs["n_primary"] + 1 and f["elements"]["a_query"][1] == 1
        assert f == zkc.check_key(kp, r1cs=desc, host=True).fields()
    finally:
        kp.free()


def test_wrapping_key_passes_with_its_circuit_and_not_with_the_nine_input_one(zkc):
    """(with the chunk of the rule: at 64 points per launch the key's 270 k points are four thousand launches of one wave each)"""
    zkc.key_check_set_chunk(0)
    agg = zkc.AggregatorCircuit(2, 1)
    desc = zkc.r1cs_desc_from_aggregator(agg)
    kp = _setup(zkc, desc)
    other = zkc.AggregatorCircuit(2, 9)
    try:
        rep = zkc.check_key(kp, r1cs=desc)
        f = rep.fields()
        assert f["ok"] == 1 and f["structure"] == 0 and f["pairs"] == 0 and f["pairs_evaluated"] == 7, rep.describe()
        assert f["elements"]["a_query"][0] == desc.n_vars and f["elements"]["h_query"][0] == kp.domain_size - 1
        assert all(v[3] is None for v in f["elements"].values())
        rep9 = zkc.check_key(kp, r1cs=zkc.r1cs_desc_from_aggregator(other))
        f9 = rep9.fields()
        assert f9["ok"] == 0 and f9["structure"] == K.A and f9["structure_first"] is None, rep9.describe()
        assert f9["pairs"] == 0 and all(v[3] is None for v in f9["elements"].values())      # the key itself is still a good key
    finally:
        zkc.key_check_set_chunk(64)
        kp.free(); agg.free(); other.free()


def test_server_check_key_refuses_the_key_of_another_circuit(zk, tmp_path):
    """--check-key: a keypair file that holds a healthy key of ANOTHER system with as many primary inputs (so that the server's own
    "invalid VK" look at the ABC length passes) is refused before anything is uploaded, naming the element.  (The server's own key
    passing the same call - check_key(keypair, r1cs) - is test_wrapping_key_passes_with_its_circuit_and_not_with_the_nine_input_one.)"""
    from tests.helpers import csr_from_rows, make_r1cs
    from zecale_amd import server as S
    assert S.main(["--check-key"], parse_only=True).check_key is True and S.main([], parse_only=True).check_key is False
    agg = zk.AggregatorCircuit(S.BATCH_SIZE, S.NUM_INPUTS_PER_NESTED_PROOF)
    l = agg.num_primary_inputs()
    agg.free()
    A, B, C, z = make_r1cs(5, 20, l, 10)
    desc, keep = zk.make_r1cs_desc(*(csr_from_rows(x) for x in (A, B, C)), len(z), l)
    other = _setup(zk, desc)
    path = str(tmp_path / "other_keypair.bin")
    other.write(path)
    other.free()
    with pytest.raises(ValueError, match="refused.*a_query.*its length"):
        S.GpuProver(path, device=0, gpu_slots=1, witness_workers=1, check_key=True)


def test_edwards_fallback_points_at_the_key_check(zk, long_keys):
    """A key with one L point not of order r asked onto the Edwards model: the upload succeeds on XYZZ as before, and
    zkhip_last_error() now says where to look; the key check names the point."""
    key = long_keys[200].replace("l_query", 17, K.refused(P.bad_points(False)[1]))
    assert key.el["l_query"][17].code == P.NOT_ORDER_R
    pk, abc = key.arrays()
    crs = zk.Crs(pk, key.n_vars, key.n_primary, key.domain_size, opts=zk.key_opts(table_model=1))
    try:
        assert crs.table_model == 0
        assert "zkhip_crs_check" in zk.load().zkhip_last_error().decode()
    finally:
        crs.free()
    f = zk.check_key((pk, key.n_vars, key.n_primary, key.domain_size)).fields()
    assert f["elements"]["l_query"][2:] == ((0, 0, 1), 17, P.NOT_ORDER_R) and f["ok"] == 0
