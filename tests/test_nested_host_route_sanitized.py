"""The host code the nested verifier leans on - the key check and preparation of a handle (zecale_amd/csrc/nested_key.hpp: doubling
chains against Python's, refused keys by name), zkhip_bls12_377_groth16_verify (the fallback of proofs the device does not decide)
and the computation of route 0 of zkhip_internal_nested_pairing_product - as a stand-alone program (tests/nested_host_route_main.cpp with
zecale_amd/csrc/aggregator.cpp) built with the address and undefined-behaviour sanitizers and run on the CPU: its verdicts are the
construction's and its GT values the library's, on a key without inputs, the reference's fixtures, and the degenerate statements
(the rejecting one leaves the circuit DSL through an exception).  CPU only."""
import functools
import os
import subprocess

import numpy as np

from oracle import pyref as R
from tests import nested_verify_fixtures as N

HERE = os.path.dirname(os.path.abspath(__file__))


def _line(vk, pr, xs):
    limbs = np.concatenate([N.vk_limbs(vk), N.input_limbs(xs).reshape(-1), N.proof_limbs(pr)])
    return "%d %s" % (len(xs), " ".join("%x" % int(x) for x in limbs))


def test_host_verifier_and_route_0_stand_alone_under_sanitizers(tmp_path):
    from zecale_amd import zkhip
    exe = tmp_path / "nested_host_route_sanitized"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                           os.path.join(HERE, "nested_host_route_main.cpp"), os.path.join(HERE, "..", "zecale_amd", "csrc", "aggregator.cpp")])
    vk0, proofs0 = N.statements(0)
    vk1, proofs1 = N.dummy_app()
    bumped = [(proofs1[0][1][0] + 1) % R.BLS_R]
    cases = [(vk0, proofs0[0][0], [], True),                                         # a key without inputs: nothing to invert
             (vk0, dict(proofs0[0][0], c=proofs0[0][0]["a"]), [], False),
             (vk1, proofs1[0][0], proofs1[0][1], True),
             (vk1, proofs1[0][0], bumped, False),
             N.degenerate_statement(8) + (True,),                                    # the chain point at a clear bit: 0 / 0 goes through
             N.degenerate_statement(8, negated=True) + (False,)]                     # its negative: the slope's product check throws
    # the chain point at a SET bit: slope 0 / 0 passes the product check as 0, the chord's result is not 2 acc, the product is not one
    cases.append(N.degenerate_statement() + (False,))
    off = dict(vk1, ABC=[vk1["ABC"][0], (vk1["ABC"][1][0], (vk1["ABC"][1][1] + 1) % N.Q)])
    two = dict(vk1, ABC=[vk1["ABC"][0], (N.Q - 1, 0)])                               # on the curve, of order two
    refused = [(off, proofs1[0][0], proofs1[0][1]), (two, proofs1[0][0], proofs1[0][1])]
    out = subprocess.run([str(exe)], input="\n".join(_line(vk, pr, xs) for vk, pr, xs in [c[:3] for c in cases] + refused) + "\n",
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [r.split() for r in out.stdout.strip().splitlines()]
    assert len(rows) == len(cases) + 2
    assert rows[-2][:2] == ["refused", "nested"] and "ABC[1]:" in rows[-2] and "off" in rows[-2]
    assert rows[-1][:2] == ["refused", "nested"] and "ABC[1]:" in rows[-1] and "degenerate" in rows[-1]
    xor = lambda limbs: functools.reduce(lambda a, b: a ^ b, (int(x) for x in limbs), 0)
    for (vk, pr, xs, want), (n_lines, n_chain, chain, ok, acc) in zip(cases, rows):
        assert (int(n_lines), int(n_chain)) == (3 * 69 * 4 * 6, len(xs) * 253 * 12)
        assert int(chain, 16) == xor(l for B in vk["ABC"][1:] for P in N.doubling_chain(B) for l in N.g1_limbs(P))
        lib = zkhip.bls12_377_groth16_verify(N.vk_limbs(vk), N.input_limbs(xs), N.proof_limbs(pr))
        assert bool(int(ok)) == lib and lib == want
        g1, g2 = N.pair_limbs([(pr["a"], pr["b"])])
        e = zkhip.nested_pairing_product("host", g1, g2)[0]
        assert int(acc, 16) == xor(np.asarray(e).reshape(-1))
