"""Screening with status bytes (zecale_amd/server.py AggregatorService._screen over a prover's `screen_status`) on a live loopback
server with stubbed provers: refused entries carry their byte, malformed ones (code >= 2) are counted beside the dropped ones, and a
prover that has only `screen` is served as before.  The GPU prover's own screen_status through the host checked function, for a key
whose handle is refused as degenerate, runs here as well (host code).  CPU only."""
from tests.helpers import golden
from tests.test_server_cpu import StubProver
from tests.test_server_screen_cpu import ScreeningProver, _inputs, _live
from zecale_amd import encoding as E
from zecale_amd import server as S

NOT_ORDER_R_A, ENCODING_INPUT, REJECT = 0x14, 0x82, 1


class StatusProver(StubProver):
    """`screen_status` gives the transactions whose (one) input is a key of `status` that byte and records every call; it has no
    `screen`"""

    def __init__(self, status):
        super().__init__()
        self.status, self.screened = dict(status), []

    def screen_status(self, nested_vk_limbs, proofs, inputs):
        xs = [int(E.fr_to_json(i.reshape(6)), 16) for i in inputs]
        self.screened.append(xs)
        assert len(proofs) == len(inputs) and all(p.shape == (48,) for p in proofs)
        return [self.status.get(x, 0) for x in xs]


def test_status_bytes_are_kept_and_malformed_entries_counted():
    """extproof1..6 carry the inputs 7 .. 12 and the fees 12 .. 7.  8 is a wrong statement, 9 has an A outside G1, 11 an input that is
    not reduced: the batches are (7, 10) and then (12 alone is too few); three are dropped, two of them malformed."""
    prover = StatusProver({8: REJECT, 9: NOT_ORDER_R_A, 11: ENCODING_INPUT})
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (3, 1, 4, 2, 6, 5):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [7, 10]
        assert prover.screened == [[7, 8, 9, 10, 11, 12]]
        assert service.screen_dropped == 3 and service.screen_malformed == 2
        pool = service.pools["dummy_app"]
        assert pool.tx_pool_size() == 1
        got = {int(E.fr_to_json(t["inputs"].reshape(6)), 16): t["screen_status"] for t in pool.screen_refused}
        assert got == {8: REJECT, 9: NOT_ORDER_R_A, 11: ENCODING_INPUT}
        assert [len(c[1]) for c in prover.calls] == [2]
    finally:
        server.stop(0)


def test_a_prover_with_only_screen_works_as_before():
    prover = ScreeningProver(bad={8})
    assert not hasattr(prover, "screen_status")
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (3, 1, 4, 2):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [7, 9]
        assert prover.screened == [[7, 8, 9, 10]]
        assert service.screen_dropped == 1 and service.screen_malformed == 0
        assert all("screen_status" not in t for t in service.pools["dummy_app"].screen_refused)
    finally:
        server.stop(0)


def test_gpu_prover_screen_is_status_zero_and_the_host_route_gives_bytes():
    """GpuProver.screen / screen_status on an instance that was never constructed (no device): a key without a handle - (None, lock),
    as for a degenerate key - goes through zkhip_bls12_377_groth16_verify_checked."""
    import threading

    import numpy as np

    from oracle import pyref as R
    from tests import nested_verify_fixtures as N
    from zecale_amd import zkhip
    vk, proofs = N.dummy_app()
    vkl = N.vk_limbs(vk)
    p = S.GpuProver.__new__(S.GpuProver)
    p.zk = zkhip
    p._screens, p._screen_mu = {np.ascontiguousarray(vkl, dtype=np.uint64).tobytes(): (None, threading.Lock())}, threading.Lock()
    prl = [N.proof_limbs(pr) for pr, _ in proofs[:3]]
    inp = [N.input_limbs(xs) for _, xs in proofs[:3]]
    inp[1] = N.input_limbs([proofs[1][1][0] + 1])                                 # a wrong statement
    prl[2] = prl[2].copy(); prl[2][0:12] = N.g1_limbs((R.BLS_Q - 1, 0))           # A of order 2
    assert p.screen_status(vkl, prl, inp) == [0, REJECT, NOT_ORDER_R_A]
    assert p.screen(vkl, prl, inp) == [True, False, False]
