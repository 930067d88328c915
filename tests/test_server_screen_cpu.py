"""Screening of the pool before a batch is popped (zecale_amd/server.py AggregatorService._screen) on a live loopback server with a
stubbed prover that has a `screen` method: failed entries are dropped and counted, the fee order of the rest is kept, an entry is
screened once, the service's lock is not held during the call, and a prover without `screen` sees the service it always saw.  CPU only."""
import grpc
import pytest

from tests.helpers import golden
from tests.test_server_cpu import StubProver
from zecale_amd import encoding as E
from zecale_amd import server as S


class ScreeningProver(StubProver):
    """`screen` refuses the transactions whose (one) input is in `bad` and records every call; `inside` runs in the middle of it."""

    def __init__(self, bad=()):
        super().__init__()
        self.bad, self.screened, self.inside = set(bad), [], None

    def screen(self, nested_vk_limbs, proofs, inputs):
        xs = [int(E.fr_to_json(i.reshape(6)), 16) for i in inputs]
        self.screened.append(xs)
        assert len(proofs) == len(inputs) and all(p.shape == (48,) for p in proofs)
        if self.inside is not None:
            fn, self.inside = self.inside, None
            fn()
        return [x not in self.bad for x in xs]


def _live(prover):
    server, port, service = S.serve(prover, "127.0.0.1:0", max_workers=4)
    return server, S.AggregatorClient("127.0.0.1:%d" % port), service


def _inputs(batch):
    return [int(x, 16) for x in batch["ext_proof"]["inputs"][2:]]


def test_failed_entries_are_dropped_and_the_rest_keep_their_fee_order():
    """extproof1..6 carry the inputs 7 .. 12 and the fees 12 .. 7.  With 8 and 11 refused, the batches are (7, 9) and (10, 12): the
    order of the fees that are left.  Every entry is screened exactly once, in one call per request that finds new entries."""
    prover = ScreeningProver(bad={8, 11})
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (3, 1, 4, 2):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [7, 9]
        assert prover.screened == [[7, 8, 9, 10]] and service.screen_dropped == 1
        assert service.pools["dummy_app"].tx_pool_size() == 1
        with pytest.raises(grpc.RpcError) as e:                       # one entry left: no batch, and nothing new to screen
            client.get_aggregated_transaction("dummy_app")
        assert e.value.details() == "insufficient entries in pool"
        assert prover.screened == [[7, 8, 9, 10]]
        for k in (6, 5):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [10, 12]
        assert prover.screened == [[7, 8, 9, 10], [11, 12]]            # the entry that had passed is not screened again
        assert service.screen_dropped == 2 and service.pools["dummy_app"].tx_pool_size() == 0
        assert [len(c[1]) for c in prover.calls] == [2, 2]
        assert sorted(int(E.fr_to_json(t["inputs"].reshape(6)), 16) for t in service.pools["dummy_app"].screen_refused) == [8, 11]
    finally:
        server.stop(0)


def test_the_lock_is_not_held_during_screen():
    """The stub submits a transaction from inside `screen`: with the service's lock held the submission would never return.  The
    entry that arrives meanwhile has the highest fee but no verdict: it is not popped, and goes through the next request's screening -
    where it is refused."""
    prover = ScreeningProver(bad={7})
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (2, 3):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        prover.inside = lambda: client.submit_nested_transaction(golden("dummy_app/extproof1.json"))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [8, 9]
        assert prover.screened == [[8, 9]] and service.pools["dummy_app"].tx_pool_size() == 1
        for k in (4, 5):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [10, 11]
        assert prover.screened == [[8, 9], [7, 10, 11]] and service.screen_dropped == 1
    finally:
        server.stop(0)


def test_a_request_during_a_screening_waits_for_its_entries():
    """Four transactions are queued and the first request's screening has all of them out of the pool when a second request for the
    application arrives (the stub starts it from inside `screen`).  It must not see an empty pool: it waits for the first request to put
    the entries back and pop, and gets the second batch."""
    import threading
    asked = threading.Event()                                         # set whenever a request asks the prover whether it screens

    class Watched(ScreeningProver):
        screen_nested = property(lambda self: asked.set() or True)
    prover = Watched()
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (1, 2, 3, 4):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        second = {}

        def request():
            try:
                second["inputs"] = _inputs(client.get_aggregated_transaction("dummy_app"))
            except grpc.RpcError as e:
                second["error"] = e.details()
        t = threading.Thread(target=request)

        def inside():                                                 # the screening goes on only once the second request is being handled
            asked.clear()
            t.start()
            assert asked.wait(30)
        prover.inside = inside
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [7, 8]
        t.join()
        assert second == {"inputs": [9, 10]}
        assert prover.screened == [[7, 8, 9, 10]] and service.screen_dropped == 0
    finally:
        server.stop(0)


def test_a_failing_screen_loses_nothing():
    prover = ScreeningProver()
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (1, 2):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))

        def boom():
            raise RuntimeError("screen broke")
        prover.inside = boom
        with pytest.raises(grpc.RpcError) as e:
            client.get_aggregated_transaction("dummy_app")
        assert e.value.details() == "screen broke" and service.pools["dummy_app"].tx_pool_size() == 2
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [7, 8] and service.screen_dropped == 0
    finally:
        server.stop(0)


def test_a_prover_without_screen_behaves_as_before():
    prover = StubProver()
    server, client, service = _live(prover)
    try:
        client.register_application(golden("dummy_app/vk.json"), "dummy_app")
        for k in (3, 1, 4, 2):
            client.submit_nested_transaction(golden("dummy_app/extproof%d.json" % k))
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [7, 8]
        assert _inputs(client.get_aggregated_transaction("dummy_app")) == [9, 10]
        assert service.screen_dropped == 0
        assert not hasattr(service.pools["dummy_app"], "screen_refused")
    finally:
        server.stop(0)
