#!/usr/bin/env python3
"""Nested (BLS12-377) Groth16 verification of the dummy application's proofs (one input): the GPU kernels (zkhip.NestedVerifier)
against the host route (zkhip.bls12_377_groth16_verify) on 16 threads, on the same batches, both routes in the same run taking
turns, the median of three at every count; and the wrapping stream's rate with and without a NestedVerifier screening batches of
64 beside it.  Writes profiles/nested_verify_gpu.txt (or --out).  The first GPU call (work space) is not timed.
GATE: at 1,024 proofs the GPU batch is no slower than the sixteen host threads on the same batch.  last_fallbacks must be zero
everywhere: a batch that went through the host would make the comparison meaningless.
--checked measures the CHECKED route instead of the host comparison (profiles/nested_verify_checked.txt): at 64, 1,024 and 16,384 proofs
per batch the unchecked and the checked call on ONE checked handle and the same batches taking turns, with --parent-lib the unchecked call
of a library built from the parent commit in the same turns (nothing was added to that route: the two must agree within the spread of
the repeats), and the wrapping stream without a screener, with an unchecked and with a checked one.  No gate: the ratio is the number on
file.
--combined measures the COMBINED route (profiles/nested_verify_combined.txt): all-valid batches at 1, 64, 1,024 and 16,384 proofs, scalars
drawn from the OS; verify_all on an unchecked handle, verify_all with status on a checked one, the two per-proof routes and, with
--parent-lib, the parent build's two per-proof routes take turns in one run, medians of five.  CONDITION 1: this build's per-proof
routes differ from the parent build's by no more than the spread (max - min) of their five repeats, the larger of the two builds'.
CONDITION 2: at 16,384 proofs each combined route is faster than its per-proof route by more than both routes' spreads.  The ratio is
recorded, not gated.  Then a batch WITH an invalid proof through verify_batch_combined (both routes run) against the checked batch, and
the wrapping stream with a checked and with a combined screener on all-valid batches of 64.
Usage: python tools/nested_verify_ab.py [--out FILE] [--stream N] [--gpu-slots K] [--checked | --combined] [--parent-lib libzkhip.so]"""
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
CHECKED_COUNTS = (64, 1024, 16384)
CHECKED_ROUNDS = 5
ROUNDS = 3
COUNTS = (1, 64, 1024, 16384)
EXTRA = (4, 16, 256)                # more points for the count at which the GPU overtakes the host
SCREEN_BATCH = 64


class ParentVerifier:
    """zkhip_nested_verifier_* of ANOTHER build of the library (the parent commit's), loaded beside this one: its unchecked route"""

    def __init__(self, path, vk, k, checked=False):
        import ctypes
        self.ct, self.lib = ctypes, ctypes.CDLL(path)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        self.lib.zkhip_nested_verifier_new.argtypes = [u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        self.lib.zkhip_nested_verifier_new_checked.argtypes = [u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        self.lib.zkhip_nested_verifier_verify_batch.argtypes = [ctypes.c_void_p, u64p, u64p, ctypes.c_size_t, ctypes.c_void_p]
        self.lib.zkhip_nested_verifier_verify_batch_checked.argtypes = [ctypes.c_void_p, u64p, u64p, ctypes.c_size_t, ctypes.c_void_p]
        self.lib.zkhip_nested_verifier_free.argtypes = [ctypes.c_void_p]
        self.p = lambda a: a.ctypes.data_as(u64p)
        assert self.lib.zkhip_init(0) == 0
        self.handle = ctypes.c_void_p()
        self.vk = np.ascontiguousarray(vk, dtype=np.uint64)
        new = self.lib.zkhip_nested_verifier_new_checked if checked else self.lib.zkhip_nested_verifier_new
        assert new(self.p(self.vk), k, ctypes.byref(self.handle)) == 0

    def verify_batch_checked(self, inp, prf):
        st = np.zeros(prf.shape[0], dtype=np.uint8)
        assert self.lib.zkhip_nested_verifier_verify_batch_checked(self.handle, self.p(inp), self.p(prf), prf.shape[0], st.ctypes.data) == 0
        return st

    def verify_batch(self, inp, prf):
        ok = np.zeros(prf.shape[0], dtype=np.uint8)
        assert self.lib.zkhip_nested_verifier_verify_batch(self.handle, self.p(inp), self.p(prf), prf.shape[0], ok.ctypes.data) == 0
        return ok.astype(bool)

    def free(self):
        self.lib.zkhip_nested_verifier_free(self.handle)


def checked_table(say, zkhip, vk, pool, pool_in, parent_lib):
    """unchecked vs checked on one checked handle (and the parent build's unchecked route), the routes taking turns on the same batch"""
    n_pool = len(pool)
    ver = zkhip.NestedVerifier(vk, 1, checked=True)
    parent = ParentVerifier(parent_lib, vk, 1) if parent_lib else None
    routes = [("unchecked", lambda i, p: list(ver.verify_batch(i, p)))]
    if parent:
        routes.append(("parent", lambda i, p: list(parent.verify_batch(i, p))))
    routes.append(("checked", lambda i, p: [int(c | m) == 0 for c, m in zip(*ver.verify_batch_checked(i, p))]))
    for _, fn in routes:
        fn(pool_in[:1], pool[:1])                            # work space
    fallbacks = 0
    say("%8s %-10s %10s %10s %10s %14s" % ("count", "route", "median ms", "min ms", "max ms", "verif./s"))
    ratios = {}
    for count in CHECKED_COUNTS:
        idx = [i % n_pool for i in range(count)]
        inp, prf = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
        want = [i != n_pool - 1 for i in idx]
        ms = {name: [] for name, _ in routes}
        for _ in range(CHECKED_ROUNDS):
            for name, fn in routes:
                t = time.perf_counter()
                ok = fn(inp, prf)
                ms[name].append((time.perf_counter() - t) * 1e3)
                assert ok == want, "%s verdicts at count %d" % (name, count)
                if name != "parent":
                    fallbacks += ver.last_fallbacks()
        med = {name: sorted(v)[CHECKED_ROUNDS // 2] for name, v in ms.items()}
        for name, _ in routes:
            say("%8d %-10s %10.2f %10.2f %10.2f %14.1f" % (count, name, med[name], min(ms[name]), max(ms[name]), count / med[name] * 1e3))
        ratios[count] = med["checked"] / med["unchecked"]
        line = "%8d checked / unchecked = %.3f" % (count, ratios[count])
        if parent:
            spread = (max(ms["unchecked"]) - min(ms["unchecked"])) / med["unchecked"]
            line += "; unchecked / parent's unchecked = %.3f (spread of the unchecked repeats: %.1f %% of their median)" % (med["unchecked"] / med["parent"], spread * 100)
        say(line)
    if parent:
        parent.free()
    return ver, fallbacks


def combined_table(say, zkhip, vk, pool, pool_in, parent_lib):
    """the combined routes, the per-proof routes and the parent build's per-proof routes taking turns on the same all-valid batches"""
    valid, valid_in = pool[:-1], pool_in[:-1]                # (the pool's last statement is the invalid one)
    n_valid = len(valid)
    ver, plain = zkhip.NestedVerifier(vk, 1, checked=True), zkhip.NestedVerifier(vk, 1)
    parent = ParentVerifier(parent_lib, vk, 1, checked=True) if parent_lib else None
    finish, degenerate, fallbacks = {}, [0], [0]

    def combined(i, p):
        ok = plain.verify_all(i, p)
        finish.setdefault(len(p), []).append(plain.last_finish_ms())
        degenerate[0] += plain.last_degenerate()
        return ok

    def combined_status(i, p):
        ok, st = ver.verify_all(i, p, status=True)
        degenerate[0] += ver.last_degenerate()
        return ok and not any(st)

    def per_proof(i, p):
        ok = plain.verify_batch(i, p).all()
        fallbacks[0] += plain.last_fallbacks()
        return ok

    def checked(i, p):
        codes, masks = ver.verify_batch_checked(i, p)
        fallbacks[0] += ver.last_fallbacks()
        return not (codes | masks).any()
    routes = [("combined", combined), ("comb+status", combined_status), ("per-proof", per_proof), ("checked", checked)]
    if parent:
        routes += [("parent", lambda i, p: parent.verify_batch(i, p).all()), ("parent chk", lambda i, p: not parent.verify_batch_checked(i, p).any())]
    for _, fn in routes:
        fn(valid_in[:1], valid[:1])                          # work space
    finish.clear()
    spread = lambda v: max(v) - min(v)
    say("%8s %-12s %10s %10s %10s %14s" % ("count", "route", "median ms", "min ms", "max ms", "verif./s"))
    ahead, cond1, cond2, ratios = None, True, True, {}
    for count in COUNTS:
        idx = [i % n_valid for i in range(count)]
        inp, prf = np.ascontiguousarray(valid_in[idx]), np.ascontiguousarray(valid[idx])
        ms = {name: [] for name, _ in routes}
        for _ in range(CHECKED_ROUNDS):
            for name, fn in routes:
                t = time.perf_counter()
                ok = fn(inp, prf)
                ms[name].append((time.perf_counter() - t) * 1e3)
                assert ok, "%s on an all-valid batch of %d" % (name, count)
        med = {name: sorted(v)[CHECKED_ROUNDS // 2] for name, v in ms.items()}
        for name, _ in routes:
            say("%8d %-12s %10.2f %10.2f %10.2f %14.1f" % (count, name, med[name], min(ms[name]), max(ms[name]), count / med[name] * 1e3))
        fin = sorted(finish[count])[len(finish[count]) // 2]
        ratios[count] = (med["combined"] / med["per-proof"], med["comb+status"] / med["checked"])
        line = "%8d combined / per-proof = %.3f; combined with status / checked = %.3f; host finish %.2f ms = %.0f %% of the combined batch" % (
            count, ratios[count][0], ratios[count][1], fin, fin / med["combined"] * 100)
        if parent:
            for mine, theirs in (("per-proof", "parent"), ("checked", "parent chk")):
                d, sp = med[mine] - med[theirs], max(spread(ms[mine]), spread(ms[theirs]))
                cond1 = cond1 and abs(d) <= sp
                line += "; %s - parent's = %+.2f ms, spread %.2f ms: %s" % (mine, d, sp, "within" if abs(d) <= sp else "BEYOND")
        say(line)
        if ahead is None and med["combined"] < med["per-proof"]:
            ahead = count
        if count == 16384:
            for comb, pp in (("combined", "per-proof"), ("comb+status", "checked")):
                gap, sp = med[pp] - med[comb], max(spread(ms[comb]), spread(ms[pp]))
                cond2 = cond2 and gap > sp
                say("%8d %s is %.2f ms faster than %s; the larger spread of the two is %.2f ms" % (count, comb, gap, pp, sp))
    say("the combined check is ahead of the per-proof batch from count %s on (smallest measured count at which its batch is faster)" % (ahead or "none measured"))
    if parent:
        say("CONDITION 1, no regression (both per-proof routes within the spread of the five repeats of the parent build's, at every count): %s" % ("met" if cond1 else "MISSED"))
    say("CONDITION 2, speed (at 16,384 proofs each combined route faster than its per-proof route by more than both spreads): %s  (%.3f, %.3f; recorded, not gated)"
        % ("met" if cond2 else "MISSED", ratios[16384][0], ratios[16384][1]))
    # a batch WITH an invalid proof: verify_batch_combined runs the combined check, then the checked batch
    say("a batch with ONE invalid proof on the checked handle: verify_batch_combined (both routes run) against verify_batch_checked")
    for count in (64, 1024, 16384):
        idx = [i % n_valid for i in range(count)]
        inp, prf = np.ascontiguousarray(valid_in[idx]), np.ascontiguousarray(valid[idx])
        inp[count // 2], prf[count // 2] = pool_in[-1], pool[-1]
        both, one = [], []
        for _ in range(CHECKED_ROUNDS):
            t = time.perf_counter(); a = ver.verify_batch_combined(inp, prf); both.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); b = ver.verify_batch_checked(inp, prf); one.append((time.perf_counter() - t) * 1e3)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and int(b[0].sum()) == 1
        mb, mo = sorted(both)[CHECKED_ROUNDS // 2], sorted(one)[CHECKED_ROUNDS // 2]
        say("%8d both routes %10.2f ms, checked alone %10.2f ms: %.3f" % (count, mb, mo, mb / mo))
    say("proofs with a degenerate line schedule (last_degenerate) summed over every combined batch of this run: %d" % degenerate[0])
    if parent:
        parent.free()
    plain.free()
    return ver, fallbacks[0], cond1 and cond2 and degenerate[0] == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--checked", action="store_true", help="measure the checked route against the unchecked one instead of the GPU against the host")
    ap.add_argument("--combined", action="store_true", help="measure the combined (random-combination) route against the per-proof routes on all-valid batches")
    ap.add_argument("--parent-lib", default=None, help="with --checked or --combined: a libzkhip.so built from the parent commit, for its per-proof routes in the same turns")
    ap.add_argument("--stream", type=int, default=1024, help="proofs per block of the stream measurement (0: skip)")
    ap.add_argument("--gpu-slots", type=int, default=24)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "nested_verify_combined.txt" if args.combined else "nested_verify_checked.txt" if args.checked else "nested_verify_gpu.txt")
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
    if args.combined:
        say("# nested Groth16 verification, dummy-application key (1 input): ONE combined check per batch vs the per-proof routes, all-valid batches,"
            " scalars drawn from the OS, %d alternating runs" % CHECKED_ROUNDS)
        ver, fallbacks, gate = combined_table(say, zkhip, vk, pool, pool_in, args.parent_lib)
    elif args.checked:
        say("# nested Groth16 verification, dummy-application key (1 input): the checked route (every point's encoding, curve and order, every input's range,"
            " on the device) vs the unchecked one, %d alternating runs" % CHECKED_ROUNDS)
        ver, fallbacks = checked_table(say, zkhip, vk, pool, pool_in, args.parent_lib)
        gate = True
    else:
        ver, fallbacks, gate = host_table(say, zkhip, vk, pool, pool_in)
    if args.stream:
        fallbacks += stream_section(say, args, bench, zkhip, ver, pool, pool_in)
    say("last_fallbacks summed over every GPU batch of this run: %d" % fallbacks)
    ver.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if gate and fallbacks == 0 else 1


def host_table(say, zkhip, vk, pool, pool_in):
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
    return ver, fallbacks, gate


def stream_section(say, args, bench, zkhip, ver, pool, pool_in):
    """The wrapping stream's rate without a screener and with a NestedVerifier screening batches of 64 back to back beside it, the
    blocks interleaved, each kind twice; with --checked the handle screens through its unchecked and through its checked route.
    Returns the fallbacks of the screening batches."""
    n_pool, fallbacks = len(pool), [0]
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
    if args.combined:
        n_pool -= 1                                              # all-valid screening batches: the case --screen-combined is for
    idx = [i % n_pool for i in range(SCREEN_BATCH)]
    s_in, s_pr = np.ascontiguousarray(pool_in[idx]), np.ascontiguousarray(pool[idx])
    s_want = [i != len(pool) - 1 for i in idx]
    screened = [0]

    def screen_combined():                                       # GpuProver.screen_status with screen_combined
        ok, st = ver.verify_all(s_in, s_pr, status=True)
        return [True] * SCREEN_BATCH if ok else [int(c | m) == 0 for c, m in zip(*ver.verify_batch_checked(s_in, s_pr))]
    screen = {"unchecked": lambda: list(ver.verify_batch(s_in, s_pr)),
              "checked": lambda: [int(c | m) == 0 for c, m in zip(*ver.verify_batch_checked(s_in, s_pr))],
              "combined": screen_combined}

    def block(kind):
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
            while not stop.is_set():
                assert screen[kind]() == s_want
                fallbacks[0] += ver.last_fallbacks()
                screened[0] += 1
        ths = [threading.Thread(target=worker, args=(p_,)) for p_ in provers]
        sc = threading.Thread(target=screener) if kind else None
        t = time.perf_counter()
        if sc:
            sc.start()
        [x.start() for x in ths]; [x.join() for x in ths]
        dt = time.perf_counter() - t
        stop.set()
        if sc:
            sc.join()
        return args.stream / dt, (screened[0] - n0) * SCREEN_BATCH / dt
    kinds = (None, "checked", "combined") if args.combined else (None, "unchecked", "checked") if args.checked else (None, "unchecked")
    rates = [(k, block(k)) for k in kinds + kinds]
    say("wrapping stream, %d proofs per block on %d prover instances, proofs/s (a NestedVerifier screens batches of %d back to back beside it where it runs):"
        % (args.stream, args.gpu_slots, SCREEN_BATCH))
    name = {None: "without NestedVerifier", "unchecked": "with NestedVerifier", "checked": "with NestedVerifier, checked",
            "combined": "with NestedVerifier, combined"}
    for k, (r, s_) in rates:
        say("  %-30s %8.1f%s" % (name[k], r, "   (%.0f nested verifications/s beside it)" % s_ if k else ""))
    mean = {k: sum(r for kk, (r, _) in rates if kk == k) / 2 for k in kinds}
    for k in kinds[1:]:
        say("  loss of the wrapping stream %s: %.1f %%" % (name[k], (1 - mean[k] / mean[None]) * 100))
    for p_ in provers:
        p_.free()
    crs.free(); kp.free(); agg.free()
    return fallbacks[0]


if __name__ == "__main__":
    sys.exit(main())
