#!/usr/bin/env python3
"""Nested (BLS12-377) Groth16 verification of the dummy application's proofs (one input): the GPU kernels (zkhip.NestedVerifier)
against the host route (zkhip.bls12_377_groth16_verify) on 16 threads, on the same batches, both routes in the same run taking
turns, the median of three at every count; and the wrapping stream's rate with and without a NestedVerifier screening batches of
64 beside it.  Writes profiles/nested_verify_gpu.txt (or --out).  The first GPU call (work space) is not timed.
GATE: at 1,024 proofs the GPU batch is no slower than the sixteen host threads on the same batch.  last_fallbacks must be zero
everywhere: a batch that went through the host would make the comparison meaningless.
Usage: python tools/nested_verify_ab.py [--out FILE] [--stream N] [--gpu-slots K]"""
import argparse
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOST_THREADS = 16
ROUNDS = 3
COUNTS = (1, 64, 1024, 16384)
EXTRA = (4, 16, 256)                # more points for the count at which the GPU overtakes the host
SCREEN_BATCH = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_verify_gpu.txt"))
    ap.add_argument("--stream", type=int, default=1024, help="proofs per block of the stream measurement (0: skip)")
    ap.add_argument("--gpu-slots", type=int, default=24)
    args = ap.parse_args()
    import bench
    from tests.helpers import golden
    from zecale_amd import encoding as E
    from zecale_amd import zkhip
    zkhip.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    vk = E.nested_verification_key_from_json(golden("dummy_app/vk.json"))
    pool, pool_in = [], []
    for k in range(1, 7):
        pr, inp = E.nested_extended_proof_from_json(golden("dummy_app/extproof%d.json" % k)["extended_proof"])
        pool.append(pr); pool_in.append(inp.reshape(1, 6))
    pool, pool_in = np.array(pool), np.array(pool_in)
    pool_in[-1] = pool_in[0]                                 # one invalid statement in the pool: proof 6 with proof 1's input
    n_pool = len(pool)
    say("# nested Groth16 verification, dummy-application key (1 input): GPU kernels vs the host route on %d threads, medians of %d alternating runs"
        % (HOST_THREADS, ROUNDS))

    ver = zkhip.NestedVerifier(vk, 1)
    ver.verify_batch(pool_in[:1], pool[:1])
    fallbacks = ver.last_fallbacks()
    host_one = lambda i: zkhip.bls12_377_groth16_verify(vk, pool_in[i], pool[i])
    say("%8s %12s %16s %14s %16s %-10s" % ("count", "GPU ms", "GPU verif./s", "host ms (16 t)", "host verif./s", "GPU faster"))
    gpu_ms, host_ms = {}, {}
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(host_one, [i % n_pool for i in range(HOST_THREADS)]))          # threads up
        for count in sorted(COUNTS + EXTRA):
            idx = [i % n_pool for i in range(count)]
            inp, prf = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
            want = [i != n_pool - 1 for i in idx]
            g, h = [], []
            for _ in range(ROUNDS):                              # the two routes take turns on the same batch
                t = time.perf_counter()
                ok = ver.verify_batch(inp, prf)
                g.append(time.perf_counter() - t)
                fallbacks += ver.last_fallbacks()
                assert list(ok) == want, "GPU verdicts at count %d" % count
                t = time.perf_counter()
                hok = list(ex.map(host_one, idx))
                h.append(time.perf_counter() - t)
                assert hok == want, "host verdicts at count %d" % count
            dg, dh = sorted(g)[ROUNDS // 2], sorted(h)[ROUNDS // 2]
            gpu_ms[count], host_ms[count] = dg * 1e3, dh * 1e3
            say("%8d %12.2f %16.1f %14.2f %16.1f %-10s%s" % (count, dg * 1e3, count / dg, dh * 1e3, count / dh, "yes" if dg <= dh else "no",
                                                          "" if count in COUNTS else "   (crossover probe)"))
    over = [c for c in sorted(gpu_ms) if gpu_ms[c] <= host_ms[c]]
    say("the GPU overtakes the %d host threads at count %s (smallest measured count at which its batch is no slower)" % (HOST_THREADS, over[0] if over else "none measured"))
    gate = gpu_ms[1024] <= host_ms[1024]
    say("GATE (GPU no slower than %d host threads at 1,024 proofs): %s  (%.1fx)" % (HOST_THREADS, "met" if gate else "MISSED", host_ms[1024] / gpu_ms[1024]))

    # ---- the wrapping stream with and without a NestedVerifier screening beside it (interleaved: without, with, without, with)
    if args.stream:
        nvk_l, npr, nin, trapdoor = bench.aggregator_inputs(1)
        agg = zkhip.AggregatorCircuit(2, 1)
        desc = zkhip.r1cs_desc_from_aggregator(agg)
        kp = zkhip.Keypair(desc, *trapdoor)
        crs = kp.upload_crs()
        z = agg.witness(nvk_l, npr, nin)
        rs = bench.random_fr_uniform(9, 2)
        provers = [zkhip.Prover(crs, desc) for _ in range(args.gpu_slots)]
        for p_ in provers:
            p_.set_streaming(True)
            p_.prove(z, rs[0], rs[1])
        idx = [i % n_pool for i in range(SCREEN_BATCH)]
        s_in, s_pr = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
        s_want = [i != n_pool - 1 for i in idx]
        screened = [0]

        def block(with_screen):
            counter, lock, stop = [args.stream], threading.Lock(), threading.Event()
            n0 = screened[0]

            def worker(p_):
                while True:
                    with lock:
                        if counter[0] <= 0:
                            return
                        counter[0] -= 1
                    p_.prove(z, rs[0], rs[1])

            def screener():
                nonlocal fallbacks
                while not stop.is_set():
                    assert list(ver.verify_batch(s_in, s_pr)) == s_want
                    fallbacks += ver.last_fallbacks()
                    screened[0] += 1
            ths = [threading.Thread(target=worker, args=(p_,)) for p_ in provers]
            sc = threading.Thread(target=screener) if with_screen else None
            t = time.perf_counter()
            if sc:
                sc.start()
            [x.start() for x in ths]; [x.join() for x in ths]
            dt = time.perf_counter() - t
            stop.set()
            if sc:
                sc.join()
            return args.stream / dt, (screened[0] - n0) * SCREEN_BATCH / dt
        rates = [(w, block(w)) for w in (False, True, False, True)]
        say("wrapping stream, %d proofs per block on %d prover instances, proofs/s (a NestedVerifier screens batches of %d back to back beside it where it runs):"
            % (args.stream, args.gpu_slots, SCREEN_BATCH))
        for w, (r, s) in rates:
            say("  %-24s %8.1f%s" % ("with NestedVerifier" if w else "without NestedVerifier", r, "   (%.0f nested verifications/s beside it)" % s if w else ""))
        for p_ in provers:
            p_.free()
        crs.free(); kp.free(); agg.free()
    say("last_fallbacks summed over every GPU batch of this run: %d" % fallbacks)
    ver.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if gate and fallbacks == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
