#!/usr/bin/env python3
"""Witness generation for batches of 32 nested proofs: the narrow kernel (one wave per witness) against k_witness_wide at 2, 4, 8 and
16 waves per witness, in ONE process, interleaved, three times over.  For (32, 1) and (32, 9):
  * one witness alone at every width, and four witnesses in one launch: the kernels' own time (HIP events, zkhip_gpu_witness_last_ms);
  * the host generator on the job's cores (wall clock);
  * one whole wrapping proof alone: GPU witness at the width this run picked, then zkhip_prover_timings (QAP, MSMs, host tail).
Every device assignment is compared with the host generator's before its time counts.  The comparison for the default width is the
narrow kernel IN THE SAME RUN: a width becomes the default for wide programs if its median beats the narrow kernel's by more than the
spread of the three repeats; otherwise auto stays narrow.  The static counts (zkhip_gpu_witness_plan) say what the widths would
give if a chunk cost the same at every width and a barrier nothing; the measured ratio against that is what a level barrier costs.

  python tools/batch32_witness_ab.py [--out profiles/batch32_witness.txt] [--no-proof]"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

WIDTHS = (1, 2, 4, 8, 16)
REPEATS = 3
TRAPDOOR = (0x1234567, 0x2345678, 0x3456789, 0x456789a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch32_witness.txt"))
    ap.add_argument("--no-proof", action="store_true", help="skip the whole wrapping proofs (two trusted setups)")
    ap.add_argument("--shapes", default="32x1,32x9")
    ap.add_argument("--commit", default="", help="the commit and state of the tree, where the run has no git checkout to ask")
    args = ap.parse_args()
    from zecale_amd import zkhip as zk
    from tests.helpers import fr_limbs, random_fr_uniform
    from tests.batch32_fixtures import big_batch, bumped_proofs
    zk.init(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    head = args.commit
    if not head:
        try:
            git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], capture_output=True, text=True).stdout.strip()
            head = git("rev-parse", "--short", "HEAD")
            if head:
                head += ", tree dirty" if git("status", "--porcelain", "--untracked-files=no") else ", tree clean"
        except OSError:
            pass
    say("command: python tools/batch32_witness_ab.py " + " ".join(sys.argv[1:]))
    say("commit: %s" % (head or "not a git checkout"))
    say("all times in ms; kernels' own time from HIP events; three interleaved repeats: median [min .. max]")
    fmt = lambda v: "%8.2f [%8.2f .. %8.2f]" % (statistics.median(v), min(v), max(v))
    for shape in args.shapes.split(","):
        n, k = (int(x) for x in shape.split("x"))
        agg = zk.AggregatorCircuit(n, k)
        plans = {w: agg.gpu_witness_plan(w) for w in WIDTHS}
        auto = agg.gpu_witness_plan(0)
        say()
        say("== (%d, %d): %d constraints, %d chunks in %d levels (%.2f per level), %.0f MB of values per witness; auto as built = %d waves" % (
            n, k, agg.num_constraints, auto["chunks"], auto["levels"], auto["chunks"] / auto["levels"], auto["value_bytes"] / 1e6, auto["waves"]))
        vk, pr, inp, _ = big_batch(n, k)
        _, _, inp_b, _ = big_batch(n, k, bumped_proofs(n))
        four = [(vk, pr, inp), (vk, pr, inp_b), (vk, pr, inp), (vk, pr, inp_b)]
        z_host = [agg.witness(vk, pr, inp), agg.witness(vk, pr, inp_b)]
        gw = zk.GpuWitness(agg, 4)
        one, many, host = {w: [] for w in WIDTHS}, {w: [] for w in WIDTHS}, []
        for w in WIDTHS:                                  # warm-up, and the check: the same assignment at every width
            gw.set_waves(w)
            _, deg, _ = gw.run(four)
            assert not deg.any()
            for i in range(4):
                assert (gw.copy_out(i) == z_host[i % 2]).all(), "(%d, %d) at %d waves: batch %d differs from the host generator" % (n, k, w, i)
        for rep in range(REPEATS):
            for w in WIDTHS:
                gw.set_waves(w)
                gw.run(four[:1]); one[w].append(gw.last_ms())
                gw.run(four); many[w].append(gw.last_ms())
            t = time.perf_counter(); agg.witness(vk, pr, inp); host.append((time.perf_counter() - t) * 1e3)
        say("%5s %10s %8s  %-32s %-8s %-32s" % ("waves", "steps", "static", "one witness alone", "measured", "four witnesses in one launch"))
        base = statistics.median(one[1])
        for w in WIDTHS:
            say("%5d %10d %7.2fx  %-32s %7.2fx %-32s" % (w, plans[w]["steps"], plans[1]["steps"] / plans[w]["steps"], fmt(one[w]), base / statistics.median(one[w]), fmt(many[w])))
        say("host generator on the job's cores (at most 16 section threads): %s" % fmt(host))
        spread = max(max(one[w]) - min(one[w]) for w in WIDTHS)
        best = min(WIDTHS, key=lambda w: statistics.median(one[w]))
        gain = base - statistics.median(one[best])
        say("fastest: %d waves, %.2f ms under the narrow kernel's median; largest spread of three repeats %.2f ms -> %s" % (
            best, gain, spread, ("%d waves beats the narrow kernel beyond the spread" % best) if best != 1 and gain > spread else "no width beats the narrow kernel beyond the spread: auto stays at 1"))
        for w in WIDTHS[1:]:
            static, meas = plans[1]["steps"] / plans[w]["steps"], base / statistics.median(one[w])
            per_step_1 = base / plans[1]["steps"] * 1e3
            per_step_w = statistics.median(one[w]) / plans[w]["steps"] * 1e3
            say("  %2d waves: measured %.2fx of the %.2fx the static counts predict; %.2f us per chunk-step against %.2f us narrow: %.2f us per level for the barrier and what it exposes" % (
                w, meas, static, per_step_w, per_step_1, (statistics.median(one[w]) - plans[w]["steps"] * per_step_1 / 1e3) / plans[w]["levels"] * 1e3))
        if not args.no_proof:
            desc = zk.r1cs_desc_from_aggregator(agg)
            t = time.perf_counter()
            kp = zk.Keypair(desc, *(fr_limbs(x) for x in TRAPDOOR))
            say("trusted setup on the 2^%d domain: %.1f s" % (kp.domain_size.bit_length() - 1, time.perf_counter() - t))
            crs = kp.upload_crs()
            pv = zk.Prover(crs, desc)
            rs = random_fr_uniform(77, 2)
            picked = best if best != 1 and gain > spread else 1
            gw.set_waves(picked)
            rows = []
            for rep in range(REPEATS + 1):                # the first is the warm-up
                t = time.perf_counter()
                d_z, deg, prim = gw.run(four[:1])
                t_w = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                proof = pv.prove_dev(d_z[0], rs[0], rs[1])
                t_p = (time.perf_counter() - t) * 1e3
                if rep == 0:
                    assert zk.groth16_verify(kp.vk(), prim[0], proof)
                else:
                    rows.append((t_w, gw.last_ms(), t_p, pv.timings()))
            say("one wrapping proof alone (GPU witness at %d waves, assignment proved where it lies):" % picked)
            for t_w, k_ms, t_p, tm in rows:
                say("  witness %.1f wall (%.1f kernels) | proof %.1f wall: qap %.1f, msm A %.1f B2 %.1f B1 %.1f H %.1f L %.1f, host tail %.1f%s" % (
                    t_w, k_ms, t_p, tm["qap"], tm["msm_A"], tm["msm_B2"], tm["msm_B1"], tm["msm_H"], tm["msm_L"], tm["host_tail"], " (chained)" if tm["chained"] else ""))
            pv.free(); crs.free(); kp.free()
        gw.free(); agg.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
