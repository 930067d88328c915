"""A plain `bench.py` run (no --full) on the GPU: the line carries the headline and nothing measured beyond it, `--steps` sets the
timed steps, and `--dump-outputs` writes the last timed MSM's sum - checked against its closed form (the bases are k_i G with known
k_i, so sum_i s_i (k_i G) = (sum_i s_i k_i mod r) G)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_msm(zk, tmp_path):
    log_n, steps, warmup = 16, 3, 1
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-n", str(log_n), "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    n = 1 << log_n
    assert line["steps"] == steps and line["unit"] == "Mscalar/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert abs(line["value"] * line["ms_per_step"] * 1e3 - n) < 0.01 * n          # value and ms_per_step describe the same timed steps
    for extra in ("roofline", "cpu_baseline", "prover_2_20", "wrapping_prover"):
        assert extra not in line, extra
    words = np.load(tmp_path / "out" / "msm_result_affine.npy")
    assert words.dtype == np.float64 and words.shape == (48,)
    w = words.astype(np.uint64)
    got = w[0::2] | (w[1::2] << np.uint64(32))
    # the last timed step used scalar vector (warmup + steps - 1) mod n_sets, drawn as bench.py draws it (Montgomery residues)
    n_sets = min(steps + warmup, 4)
    rinv = pow(1 << 384, -1, bench.R_MOD)
    to_int = lambda a: [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(a)]
    ks = to_int(bench.random_fr_canonical(0x5EED, n))
    sc = [v * rinv % bench.R_MOD for v in to_int(bench.random_fr_uniform(0xABC0 + 17 * ((warmup + steps - 1) % n_sets), n))]
    dot = sum(a * b for a, b in zip(sc, ks)) % bench.R_MOD
    lim = np.array([[(dot >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]], dtype=np.uint64)
    expect = zk.fixed_base_mul(bench.g1_generator_limbs(), lim, montgomery=False)[0]
    assert (got == expect).all()
