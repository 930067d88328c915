"""GpuProver.screen_status with screen_combined (zecale_amd/server.py): the checked handle's combined check is asked first and the
checked per-proof batch runs only when it fails; with the option off the combined check is never asked.  A GpuProver made by __new__
with a stub handle, as tests/test_server_screen_checked_cpu.py makes one: CPU only, no device."""
import threading

import numpy as np

from zecale_amd import server as S

KEY = np.arange(84, dtype=np.uint64)


class StubHandle:
    """a checked NestedVerifier: verify_all(status=True) answers `passes`, verify_batch_checked the bytes of `status`; both are recorded"""

    def __init__(self, passes, status):
        self.passes, self.status, self.calls = passes, list(status), []

    def verify_all(self, inputs, proofs, rho=None, status=False):
        assert status is True and rho is None and inputs.shape[0] == proofs.shape[0] == len(self.status)
        self.calls.append("verify_all")
        return self.passes, bytes(len(self.status))

    def verify_batch_checked(self, inputs, proofs):
        assert inputs.shape[0] == proofs.shape[0] == len(self.status)
        self.calls.append("verify_batch_checked")
        st = np.array(self.status, dtype=np.uint8)
        return st & np.uint8(0x0F), st & np.uint8(0xF0)


def _prover(handle, **attrs):
    p = S.GpuProver.__new__(S.GpuProver)
    p.zk = None
    p._screens, p._screen_mu = {KEY.tobytes(): (handle, threading.Lock())}, threading.Lock()
    for k, v in attrs.items():
        setattr(p, k, v)
    return p


def _batch(n):
    return [np.zeros(48, dtype=np.uint64) for _ in range(n)], [np.zeros((1, 6), dtype=np.uint64) for _ in range(n)]


def test_a_passing_combined_check_returns_zeros_and_skips_the_per_proof_batch():
    h = StubHandle(True, [0, 0, 0, 0])
    p = _prover(h, screen_combined=True)
    proofs, inputs = _batch(4)
    assert p.screen_status(KEY, proofs, inputs) == [0, 0, 0, 0]
    assert p.screen(KEY, proofs, inputs) == [True] * 4
    assert h.calls == ["verify_all", "verify_all"]


def test_a_failing_combined_check_returns_the_checked_batchs_bytes():
    status = [0, 1, 0x14, 0x82, 0]
    h = StubHandle(False, status)
    p = _prover(h, screen_combined=True)
    proofs, inputs = _batch(5)
    assert p.screen_status(KEY, proofs, inputs) == status
    assert h.calls == ["verify_all", "verify_batch_checked"]
    assert p.screen(KEY, proofs, inputs) == [True, False, False, False, True]


def test_with_the_option_off_the_combined_check_is_never_asked():
    status = [0, 1, 0x14]
    proofs, inputs = _batch(3)
    for attrs in ({"screen_combined": False}, {}):          # the second: a prover made before the option existed
        h = StubHandle(True, status)
        p = _prover(h, **attrs)
        assert p.screen_status(KEY, proofs, inputs) == status
        assert h.calls == ["verify_batch_checked"]


def test_the_constructor_and_the_command_line_take_the_option():
    import inspect
    sig = inspect.signature(S.GpuProver.__init__)
    assert sig.parameters["screen_combined"].default is False
    assert "--screen-combined" in inspect.getsource(S.main)
