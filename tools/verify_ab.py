#!/usr/bin/env python3
"""Groth16 verification of the batch-2 wrapping key's proofs: the GPU pairing kernels (zkhip.Verifier) against the host route
(zkhip.groth16_verify) on 16 threads, measured in the same run, and the wrapping stream's rate with and without a Verifier checking
every proof beside it.  Writes profiles/verify_gpu.txt (or --out).  Each block runs once; the first GPU call (work space) is not timed.
The checked route (Verifier(vk, checked=True).verify_batch_checked: every proof point validated on the device first) is timed beside
the unchecked one on the same batches, no proof refused so that every point walks all 377 bits of r: unchecked, checked, three
times over at every count, the median of each.  GATE 2: checked <= 1.25 x unchecked at 1,024 proofs.
profiles/verify_checked.txt is a run with --out profiles/verify_checked.txt (profiles/verify_gpu.txt is the run before this column).
--combined writes profiles/verify_combined.txt instead: ONE random-combination check per batch (Verifier.verify_all, scalars drawn from
the OS) against the per-proof route (verify_batch) of this build and - with --parent-lib - of a library built from the parent commit,
on all-valid batches of 1 .. 65,536 proofs, the routes taking turns in one run, medians of five; the host finish's share of the
combined time; and the host route (groth16_verify_all, 16 threads) once per batch.  CONDITIONS: the per-proof route equals the parent's
within the spread of its own repeats (no kernel of it changed); the combined batch at 16,384 proofs takes at most half the per-proof
batch's time.
--located writes profiles/verify_locate.txt: per-proof verdicts by way of the combined check (Verifier.verify_batch_located) beside
Verifier.verify_all, the per-proof route and today's fallback (verify_batch_combined: combined, then per-proof) on batches of 1,024 /
16,384 / 65,536 proofs with 0, 1, 2, 16 and 1 % invalid statements at seeded positions, the routes taking turns, medians of five with
their spreads, the parent build's verify_all and per-proof route beside them with --parent-lib; and the cost rule's constants.
Usage: python tools/verify_ab.py [--out FILE] [--stream N] [--gpu-slots K] [--combined | --located] [--parent-lib libzkhip.so]"""
import argparse
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HOST_THREADS = 16
CHECKED_GATE = 1.25                 # checked ms / unchecked ms at 1,024 proofs
ROUNDS = 3
COUNTS = (1, 64, 1024, 16384)
EXTRA = (16, 32, 128, 256)          # more points for the count at which the GPU overtakes the host
BATCH = 256
COMBINED_COUNTS = (1, 64, 1024, 16384, 65536)
COMBINED_ROUNDS = 5
COMBINED_GATE = 0.5                 # combined ms / per-proof ms at 16,384 proofs


class ParentVerifier:
    """zkhip_verifier_* of ANOTHER build of the library (the parent commit's), loaded beside this one: its per-proof route"""

    def __init__(self, path, vk):
        import ctypes
        self.lib = ctypes.CDLL(path)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        self.lib.zkhip_verifier_new.argtypes = [u64p, u64p, u64p, u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        self.lib.zkhip_verifier_verify_batch.argtypes = [ctypes.c_void_p, u64p, u64p, ctypes.c_size_t, ctypes.c_void_p]
        self.lib.zkhip_verifier_free.argtypes = [ctypes.c_void_p]
        self.p = lambda a: np.ascontiguousarray(a, dtype=np.uint64).ctypes.data_as(u64p)
        assert self.lib.zkhip_init(0) == 0
        self.handle = ctypes.c_void_p()
        abc = np.ascontiguousarray(vk["ABC"], dtype=np.uint64).reshape(-1, 24)
        assert self.lib.zkhip_verifier_new(self.p(vk["alpha"]), self.p(vk["beta"]), self.p(vk["delta"]), self.p(abc), abc.shape[0] - 1,
                                           ctypes.byref(self.handle)) == 0

    def verify_batch(self, inp, prf):
        ok = np.zeros(prf.shape[0], dtype=np.uint8)
        assert self.lib.zkhip_verifier_verify_batch(self.handle, self.p(inp), self.p(prf), prf.shape[0], ok.ctypes.data) == 0
        return ok.astype(bool)

    def verify_all(self, inp, prf):
        import ctypes
        ok = ctypes.c_int(0)
        self.lib.zkhip_verifier_verify_all.argtypes = [ctypes.c_void_p, type(self.p(inp)), type(self.p(inp)), ctypes.c_size_t, ctypes.c_void_p,
                                                       ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
        assert self.lib.zkhip_verifier_verify_all(self.handle, self.p(inp), self.p(prf), prf.shape[0], None, ctypes.byref(ok), None) == 0
        return bool(ok.value)

    def free(self):
        self.lib.zkhip_verifier_free(self.handle)


def combined_table(say, zkhip, vk, pool, pool_in, parent_lib):
    """the combined check against the per-proof route (and the parent build's), taking turns on the same all-valid batches"""
    n_pool = len(pool)
    ver = zkhip.Verifier(vk)
    parent = ParentVerifier(parent_lib, vk) if parent_lib else None
    finish = []

    def combined(i, p):
        ok = ver.verify_all(i, p)
        finish.append(ver.last_finish_ms())
        return [ok] * len(p)
    routes = [("combined", combined), ("per-proof", lambda i, p: list(ver.verify_batch(i, p)))]
    if parent:
        routes.append(("parent", lambda i, p: list(parent.verify_batch(i, p))))
    for _, fn in routes:
        fn(pool_in[:1], pool[:1])                            # work space
    say("%8s %-10s %10s %10s %10s %14s" % ("count", "route", "median ms", "min ms", "max ms", "verif./s"))
    med_all, same = {}, True
    for count in COMBINED_COUNTS:
        idx = np.arange(count) % n_pool
        inp, prf = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
        for _, fn in routes:
            fn(inp, prf)                                      # the work space of this size
        ms = {name: [] for name, _ in routes}
        del finish[:]
        for _ in range(COMBINED_ROUNDS):
            for name, fn in routes:
                t = time.perf_counter()
                ok = fn(inp, prf)
                ms[name].append((time.perf_counter() - t) * 1e3)
                assert all(ok) and len(ok) == count, "%s verdicts at count %d" % (name, count)
        med = {name: sorted(v)[COMBINED_ROUNDS // 2] for name, v in ms.items()}
        med_all[count] = med
        for name, _ in routes:
            say("%8d %-10s %10.2f %10.2f %10.2f %14.1f" % (count, name, med[name], min(ms[name]), max(ms[name]), count / med[name] * 1e3))
        fin = sorted(finish)[len(finish) // 2]
        t = time.perf_counter()
        assert zkhip.groth16_verify_all(vk, inp, prf)
        host_ms = (time.perf_counter() - t) * 1e3
        line = "%8d combined / per-proof = %.3f; host finish %.1f ms = %.0f %% of the combined batch; host route on %d threads (one run): %.0f ms" % (
            count, med["combined"] / med["per-proof"], fin, 100 * fin / med["combined"], HOST_THREADS, host_ms)
        if parent:
            spread = max(ms["per-proof"]) - min(ms["per-proof"])
            agree = abs(med["per-proof"] - med["parent"]) <= spread
            same = same and agree
            line += "; per-proof - parent's = %+.2f ms, spread of the per-proof repeats %.2f ms: %s" % (med["per-proof"] - med["parent"], spread,
                                                                                                       "within" if agree else "OUTSIDE")
        say(line)
    pays = [c for c in COMBINED_COUNTS if med_all[c]["combined"] < med_all[c]["per-proof"]]
    say("the combined check is the cheaper one from count %s on (smallest measured count at which its batch is faster)" % (pays[0] if pays else "none measured"))
    ratio = med_all[16384]["combined"] / med_all[16384]["per-proof"]
    gate = ratio <= COMBINED_GATE
    say("CONDITION speed (combined <= %.1f x per-proof at 16,384 proofs, medians of %d alternating runs): %s  (%.3f, %.1fx faster)"
        % (COMBINED_GATE, COMBINED_ROUNDS, "met" if gate else "MISSED", ratio, 1 / ratio))
    if parent:
        say("CONDITION no regression (per-proof route within the spread of its own repeats of the parent build's, at every count): %s" % ("met" if same else "MISSED"))
        parent.free()
    ver.free()
    return gate and same


LOCATED_COUNTS = (1024, 16384, 65536)
LOCATED_BAD = (0, 1, 2, 16, "1 %")
LOCATED_ROUNDS = 5


def located_table(say, zkhip, vk, pool, pool_in, bad_proof, bad_in, parent_lib, counts=LOCATED_COUNTS):
    """the located route beside the combined check, the per-proof route and today's fallback (combined, then per-proof), taking turns
    on the same batches with 0, 1, 2, 16 and 1 % invalid statements at seeded positions; the parent build's two routes beside them"""
    n_pool = len(pool)
    ver = zkhip.Verifier(vk)
    parent = ParentVerifier(parent_lib, vk) if parent_lib else None
    routes = [("located", lambda i, p: list(ver.verify_batch_located(i, p))),
              ("combined", lambda i, p: ver.verify_all(i, p)),
              ("per-proof", lambda i, p: list(ver.verify_batch(i, p))),
              ("fallback", lambda i, p: list(ver.verify_batch_combined(i, p)))]
    if parent:
        routes += [("parent-combined", lambda i, p: parent.verify_all(i, p)), ("parent-per-proof", lambda i, p: list(parent.verify_batch(i, p)))]
    for _, fn in routes:
        fn(pool_in[:1], pool[:1])                            # work space
    # the per-proof route by count: what the cost rule takes for handing proofs over (its time rises in steps of 4,096 proofs)
    steps = {}
    for count in (1024, 2048, 4096, 4097, 6144, 8192, 8193, 12288, 12289, 16384):
        idx = np.arange(count) % n_pool
        inp, prf = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
        ver.verify_batch(inp, prf)
        ms = []
        for _ in range(LOCATED_ROUNDS):
            t = time.perf_counter()
            assert ver.verify_batch(inp, prf).all()
            ms.append((time.perf_counter() - t) * 1e3)
        steps[count] = sorted(ms)[LOCATED_ROUNDS // 2]
        say("per-proof route, %6d proofs: median %.1f ms (%.1f .. %.1f)" % (count, steps[count], min(ms), max(ms)))
    say("%8s %8s %-16s %10s %10s %10s   %s" % ("count", "invalid", "route", "median ms", "min ms", "max ms", "the located route's last run"))
    ok_all, cases, rounds_ms = True, {}, {}
    for count in counts:
        for spec in LOCATED_BAD:
            nbad = max(1, count // 100) if spec == "1 %" else spec
            where = np.random.RandomState(count + nbad).choice(count, nbad, replace=False)
            idx = np.arange(count) % n_pool
            inp, prf = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
            inp[where], prf[where] = bad_in, bad_proof
            want = np.ones(count, dtype=bool)
            want[where] = False
            for _, fn in routes:
                fn(inp, prf)                                  # the work space of this size
            ms = {name: [] for name, _ in routes}
            for _ in range(LOCATED_ROUNDS):
                for name, fn in routes:
                    t = time.perf_counter()
                    got = fn(inp, prf)
                    ms[name].append((time.perf_counter() - t) * 1e3)
                    if name.endswith("combined"):
                        assert got is (nbad == 0), "%s verdict at count %d, %s invalid" % (name, count, spec)
                    else:
                        assert (np.array(got) == want).all(), "%s verdicts at count %d, %s invalid" % (name, count, spec)
                    if name == "located":
                        st = ver.last_locate_stats()
            med = {name: sorted(v)[LOCATED_ROUNDS // 2] for name, v in ms.items()}
            spread = {name: max(v) - min(v) for name, v in ms.items()}
            for name, _ in routes:
                note = ""
                if name == "located":
                    note = "chunks failed %d, rounds %d, node tests %d, to the per-proof route %d, descent %.1f ms, per-proof route %.1f ms" % (
                        st["chunks_failed"], st["rounds"], st["node_tests"], st["finish_proofs"], st["descent_ms"], st["finish_ms"])
                say("%8d %8s %-16s %10.2f %10.2f %10.2f   %s" % (count, spec, name, med[name], min(ms[name]), max(ms[name]), note))
            if nbad == 0:
                inside = abs(med["located"] - med["combined"]) <= spread["combined"]
                say("%8d all valid: located - combined = %+.2f ms, spread of the combined repeats %.2f ms: %s" % (
                    count, med["located"] - med["combined"], spread["combined"], "inside" if inside else "OUTSIDE"))
                if parent:
                    for a, b in (("combined", "parent-combined"), ("per-proof", "parent-per-proof")):
                        agree = abs(med[a] - med[b]) <= spread[a]
                        ok_all = ok_all and agree
                        say("%8d no regression: %s - parent's = %+.2f ms, spread of its repeats %.2f ms: %s" % (count, a, med[a] - med[b], spread[a],
                                                                                                              "within" if agree else "OUTSIDE"))
            else:
                say("%8d %s invalid: located / fallback = %.3f (%.1f ms below; spreads %.1f and %.1f ms)" % (
                    count, spec, med["located"] / med["fallback"], med["fallback"] - med["located"], spread["located"], spread["fallback"]))
                cases[(count, spec)] = (med["located"], med["fallback"], spread["located"], spread["fallback"], dict(st))
    # the conditions, once every count has its one-proof descent: a node round of a count is that descent over its paid rounds (every
    # round of a one-proof descent is one load of the threads; a batch of one chunk knows its root already)
    for count in counts:
        if (count, 1) not in cases:
            continue
        loc, fall, s_loc, s_fall, st = cases[(count, 1)]
        paid = st["rounds"] - (1 if count <= 16384 else 0)
        rounds_ms[count] = st["descent_ms"] / paid
        line = "%8d one node round = %.1f ms (the one-proof descent, %.1f ms / %d paid rounds)" % (count, rounds_ms[count], st["descent_ms"], paid)
        if count >= 16384:
            gate = fall - loc > s_loc + s_fall
            ok_all = ok_all and gate
            line += "; CONDITION one invalid: below the fallback by more than both spreads (%.1f > %.1f + %.1f ms): %s" % (
                fall - loc, s_loc, s_fall, "met" if gate else "MISSED")
        say(line)
        if (count, "1 %") in cases:
            loc, fall, _, _, st = cases[(count, "1 %")]
            gate = loc <= fall + rounds_ms[count]
            ok_all = ok_all and gate
            say("%8d CONDITION 1 %% invalid: within one node round of the fallback (%+.1f ms against %.1f ms; its descent took %.1f ms): %s" % (
                count, loc - fall, rounds_ms[count], st["descent_ms"], "met" if gate else "MISSED"))
    node_round = rounds_ms.get(16384)
    if node_round is not None:
        say("the cost rule's constants from this run (csrc/pairing_locate.hpp LOCATE_COST): node test %.1f ms; per-proof route on up to 4,096 / 8,192 / "
            "12,288 / 16,384 proofs %.1f / %.1f / %.1f / %.1f ms" % (node_round, steps[4096], steps[8192], steps[12288], steps[16384]))
    if parent:
        parent.free()
    ver.free()
    return ok_all


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "verify_gpu.txt"))
    ap.add_argument("--stream", type=int, default=2048, help="proofs per block of the stream measurement (0: skip)")
    ap.add_argument("--gpu-slots", type=int, default=24)
    ap.add_argument("--pool", type=int, default=16, help="distinct proofs (the batches repeat them; the last one gets a bumped input)")
    ap.add_argument("--combined", action="store_true", help="the combined check against the per-proof route; writes profiles/verify_combined.txt")
    ap.add_argument("--parent-lib", default=None, help="with --combined or --located: a libzkhip.so built from the parent commit, for its routes in the same turns")
    ap.add_argument("--located", action="store_true", help="the located route against the combined check, the per-proof route and the fallback; writes profiles/verify_locate.txt")
    ap.add_argument("--located-counts", default=None, help="with --located: batch sizes, comma separated (default 1024,16384,65536)")
    args = ap.parse_args()
    if args.combined and args.out.endswith("verify_gpu.txt"):
        args.out = os.path.join(os.path.dirname(args.out), "verify_combined.txt")
    if args.located and args.out.endswith("verify_gpu.txt"):
        args.out = os.path.join(os.path.dirname(args.out), "verify_locate.txt")
    import bench
    from zecale_amd import zkhip
    zkhip.init(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nvk_l, npr, nin, trapdoor = bench.aggregator_inputs(1)
    agg = zkhip.AggregatorCircuit(2, 1)
    desc = zkhip.r1cs_desc_from_aggregator(agg)
    kp = zkhip.Keypair(desc, *trapdoor)
    vk, crs = kp.vk(), kp.upload_crs()
    z = agg.witness(nvk_l, npr, nin)
    n_in = agg.num_primary_inputs()
    prim = np.ascontiguousarray(z[1:1 + n_in])
    rs = bench.random_fr_uniform(9, 2 * args.pool)
    prover = zkhip.Prover(crs, desc)
    pool = np.array([prover.prove(z, rs[2 * i], rs[2 * i + 1]) for i in range(args.pool)])
    prover.free()
    pool_in = np.tile(prim, (args.pool, 1, 1))
    pool_in[-1, 0, 0] ^= np.uint64(1)                       # one invalid statement in the pool
    if args.located:
        say("# Groth16 verification, batch-2 wrapping key (%d primary inputs): per-proof verdicts by way of the combined check (located) vs the combined "
            "check alone, the per-proof route and today's fallback; medians of %d alternating runs" % (n_in, LOCATED_ROUNDS))
        counts = tuple(int(c) for c in args.located_counts.split(",")) if args.located_counts else LOCATED_COUNTS
        ok = located_table(say, zkhip, vk, pool[:-1], pool_in[:-1], pool[-1], pool_in[-1], args.parent_lib, counts)
        crs.free(); kp.free(); agg.free()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return 0 if ok else 1
    if args.combined:
        say("# Groth16 verification, batch-2 wrapping key (%d primary inputs): one combined check per batch vs the per-proof route, all-valid batches" % n_in)
        ok = combined_table(say, zkhip, vk, pool[:-1], pool_in[:-1], args.parent_lib)
        crs.free(); kp.free(); agg.free()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return 0 if ok else 1
    say("# Groth16 verification, batch-2 wrapping key (%d primary inputs): GPU pairing kernels vs the host route on %d threads" % (n_in, HOST_THREADS))

    # ---- host route, 16 threads (ctypes releases the GIL)
    n_host = 256
    idx = [i % args.pool for i in range(n_host)]
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(lambda i: zkhip.groth16_verify(vk, pool_in[i], pool[i]), idx[:HOST_THREADS]))      # threads up
        t = time.perf_counter()
        host_ok = list(ex.map(lambda i: zkhip.groth16_verify(vk, pool_in[i], pool[i]), idx))
        host_dt = time.perf_counter() - t
    host_rate = n_host / host_dt
    assert host_ok == [i != args.pool - 1 for i in idx], "host verdicts"
    t = time.perf_counter()
    zkhip.groth16_verify(vk, pool_in[0], pool[0])
    say("host: %d proofs on %d threads in %.2f s = %.1f verifications/s (one proof on one thread: %.1f ms)" % (n_host, HOST_THREADS, host_dt, host_rate, (time.perf_counter() - t) * 1e3))

    # ---- GPU route
    ver = zkhip.Verifier(vk)
    ver.verify_batch(pool_in[:1], pool[:1])
    chk = zkhip.Verifier(vk, checked=True)
    chk.verify_batch_checked(pool_in[:1], pool[:1])
    say("%8s %12s %16s %14s %-10s %12s %8s" % ("count", "ms/batch", "verifications/s", "host ms (16 t)", "GPU faster", "checked ms", "ratio"))
    gpu_ms, chk_ms = {}, {}
    for count in sorted(COUNTS + EXTRA):
        idx = np.arange(count) % args.pool
        inp, prf = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
        want = [i != args.pool - 1 for i in idx]
        plain, checked = [], []
        for _ in range(ROUNDS):                                  # the two routes take turns on the same batch
            t = time.perf_counter()
            ok = ver.verify_batch(inp, prf)
            plain.append(time.perf_counter() - t)
            assert list(ok) == want, "GPU verdicts at count %d" % count
            t = time.perf_counter()
            codes, masks = chk.verify_batch_checked(inp, prf)
            checked.append(time.perf_counter() - t)
            assert list(codes) == [0 if w else 1 for w in want] and not masks.any(), "checked statuses at count %d" % count
        dt, dc = sorted(plain)[ROUNDS // 2], sorted(checked)[ROUNDS // 2]
        gpu_ms[count], chk_ms[count] = dt * 1e3, dc * 1e3
        host_ms = count / host_rate * 1e3 if count >= HOST_THREADS else 1e3 / (host_rate / HOST_THREADS)
        say("%8d %12.1f %16.1f %14.1f %-10s %12.1f %8.3f%s" % (count, dt * 1e3, count / dt, host_ms, "yes" if dt * 1e3 < host_ms else "no", dc * 1e3, dc / dt,
                                                             "" if count in COUNTS else "   (crossover probe)"))
    over = [c for c in sorted(gpu_ms) if gpu_ms[c] < (c / host_rate * 1e3 if c >= HOST_THREADS else 1e3 / (host_rate / HOST_THREADS))]
    say("the GPU overtakes the %d host threads at count %s (smallest measured count at which its batch is faster)" % (HOST_THREADS, over[0] if over else "none measured"))
    gate = gpu_ms[1024] < 1024 / host_rate * 1e3
    say("GATE (GPU faster than %d host threads at 1,024 proofs): %s  (%.1fx)" % (HOST_THREADS, "met" if gate else "MISSED", (1024 / host_rate * 1e3) / gpu_ms[1024]))
    ratio = chk_ms[1024] / gpu_ms[1024]
    gate2 = ratio <= CHECKED_GATE
    say("GATE 2 (checked batch <= %.2f x unchecked at 1,024 proofs, medians of %d alternating runs): %s  (%.3fx: %.1f ms of checks on %.1f ms)"
        % (CHECKED_GATE, ROUNDS, "met" if gate2 else "MISSED", ratio, chk_ms[1024] - gpu_ms[1024], gpu_ms[1024]))

    # ---- the wrapping stream with and without a Verifier beside it (interleaved: without, with, without, with)
    if args.stream:
        provers = [zkhip.Prover(crs, desc) for _ in range(args.gpu_slots)]
        for p_ in provers:
            p_.set_streaming(True)
            p_.prove(z, rs[0], rs[1])

        def block(with_verifier):
            counter, lock, done = [args.stream], threading.Lock(), []
            cv = threading.Condition()
            verdicts = []

            def worker(p_):
                while True:
                    with lock:
                        if counter[0] <= 0:
                            return
                        counter[0] -= 1
                    pr = p_.prove(z, rs[0], rs[1])
                    with cv:
                        done.append(pr)
                        cv.notify()

            def checker():
                seen = 0
                while seen < args.stream:
                    with cv:
                        cv.wait_for(lambda: len(done) - seen >= min(BATCH, args.stream - seen))
                        take = done[seen:seen + BATCH]
                    verdicts.extend(ver.verify_batch(np.tile(prim, (len(take), 1, 1)), np.array(take)))
                    seen += len(take)
            ths = [threading.Thread(target=worker, args=(p_,)) for p_ in provers] + ([threading.Thread(target=checker)] if with_verifier else [])
            t = time.perf_counter()
            [x.start() for x in ths]; [x.join() for x in ths]
            dt = time.perf_counter() - t
            assert all(verdicts) and len(verdicts) == (args.stream if with_verifier else 0)
            return args.stream / dt
        rates = [(w, block(w)) for w in (False, True, False, True)]
        say("wrapping stream, %d proofs per block on %d prover instances, proofs/s (every proof verified in batches of %d where a Verifier runs beside it):" % (args.stream, args.gpu_slots, BATCH))
        for w, r in rates:
            say("  %-18s %8.1f" % ("with Verifier" if w else "without Verifier", r))
        for p_ in provers:
            p_.free()
    ver.free(); chk.free(); crs.free(); kp.free(); agg.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if gate and gate2 else 1


if __name__ == "__main__":
    sys.exit(main())
