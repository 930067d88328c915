"""The library's own SHA-256 (zecale_amd/csrc/sha256.hpp, what the phase-2 transcript hashes with) against hashlib, through the g++
shim of tests/phase2_host_shim.cpp.  CPU only."""
import ctypes
import hashlib

import pytest

from tests.test_phase2_lane_model import build_shim

LENGTHS = (0, 55, 56, 63, 64, 65, 119, 120, 1000)      # around the padding's two boundaries (55 / 56 and 63 / 64), in both blocks


@pytest.fixture(scope="module")
def shim():
    return build_shim()


def message(n):
    return bytes((7 * i + n) & 0xFF for i in range(n))


@pytest.mark.parametrize("n", LENGTHS)
def test_one_shot_equals_hashlib(shim, n):
    out = ctypes.create_string_buffer(32)
    shim.sha256_shim(message(n), n, out)
    assert out.raw == hashlib.sha256(message(n)).digest()


@pytest.mark.parametrize("piece", (1, 7, 64, 100))
def test_incremental_equals_hashlib(shim, piece):
    for n in LENGTHS:
        out = ctypes.create_string_buffer(32)
        shim.sha256_pieces_shim(message(n), n, piece, out)
        assert out.raw == hashlib.sha256(message(n)).digest(), n
