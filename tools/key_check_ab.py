#!/usr/bin/env python3
"""The measurements of the key check and of the checked prover, one process on one GPU (the no-regression leg starts one child
process per run).

Legs (--legs, comma list):
  key      zkhip_crs_check on the key of the 2^20 - 8 constraint system (the `prover_2_20` key of bench.py, from zkhip_groth16_setup),
           with its constraint system: per element and in total, the longest single launch; then the device and the host route (16
           threads) on the SAME points - a 2^14-point slice of every query vector, the host's time also scaled to the whole key and
           labelled as scaled.
  prover   a checked prover against the SAME prover with checking off, taking turns, medians of five: prover_2_20 and a
           wrapping-circuit prover (proofs must be identical).
  parent   with both features off: the headline (python bench.py) and one 2^20 proof alone against ANOTHER build of the library
           (--parent-lib: the parent commit's libzkhip.so), the two builds taking turns, child processes.  The difference must lie
           inside the parent's own spread of repeats.

Written to --out (profiles/key_check.txt holds the run this repository's figures come from)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(vals, unit="ms"):
    return "median %.2f  min %.2f  max %.2f %s (n = %d)" % (statistics.median(vals), min(vals), max(vals), unit, len(vals))


def key_leg(zk, bench, out):
    fs = bench.FullSizeProver(zk, 20)
    pk, m, l, d = fs.kp.pk_arrays()
    points = 5 + 3 * m + (d - 1) + (m - l - 1) + (l + 1)
    out.append("key of the 2^20 - 8 constraint system: n_vars %d, n_primary %d, domain %d: %d points" % (m, l, d, points))
    walls = []
    for rep in range(3):
        t0 = time.time()
        report = zk.check_key(fs.kp, r1cs=fs.desc)
        walls.append((time.time() - t0) * 1e3)
        assert report.ok, report.describe()
        ms = zk.key_check_last_ms()
    out.append("  zkhip_crs_check with the constraint system, whole call: %s" % spread(walls))
    out.append("  last call: point checks %.1f ms, the two MSMs of the B relation %.1f ms, the three pairing products on the host %.1f ms; "
               "rest (structure loop, descriptor) %.1f ms" % (ms[1], ms[2], ms[3], walls[-1] - ms[1] - ms[2] - ms[3]))
    out.append("  LONGEST SINGLE LAUNCH of k_key_point_check (chunk 2^17 points, device time): %.2f ms" % ms[0])
    for k, name in enumerate(zk.KEY_ELEMENTS):
        n = report.e[k].points
        if n > 1:
            out.append("    %-11s %8d points  %8.1f ms  (%.0f ns / point, staging included)" % (name, n, ms[4 + k], ms[4 + k] * 1e6 / n))
    # the same points on both routes: a 2^14-point slice of every query vector
    s = 1 << 14
    sl = dict(pk, A=pk["A"][:s], B2=pk["B2"][:s], B1=pk["B1"][:s], H=pk["H"][:s - 1], L=pk["L"][:s - 1])
    key = (sl, s, 0, s)
    sl_points = 5 + 3 * s + 2 * (s - 1)
    rho = [i + 1 for i in range(s)]
    dev, host = [], []
    for rep in range(3):
        t0 = time.time(); rd = zk.check_key(key, rho=rho); dev.append((time.time() - t0) * 1e3)
        dev_pts = zk.key_check_last_ms()[1]
        t0 = time.time(); rh = zk.check_key(key, rho=rho, host=True); host.append((time.time() - t0) * 1e3)
        host_pts = zk.key_check_last_ms()[1]
        assert rd.fields() == rh.fields() and rd.ok
    out.append("  the SAME %d points (a 2^14 slice of every vector) on both routes, whole call:" % sl_points)
    out.append("    device: %s;  host, %d threads: %s" % (spread(dev), min(16, os.cpu_count() or 1), spread(host)))
    out.append("    point checks alone (last repeat): device %.1f ms, host %.1f ms: ratio %.1f" % (dev_pts, host_pts, host_pts / dev_pts))
    out.append("    whole call: ratio %.1f.  Host route SCALED to the whole key's %d points (x %.1f): %.1f s against the device's %.2f s measured" %
               (statistics.median(host) / statistics.median(dev), points, points / sl_points, statistics.median(host) * points / sl_points / 1e3,
                statistics.median(walls) / 1e3))
    return fs


def checked_turns(zk, prover, z, r, s, name, out, repeats=5):
    ref = prover.prove(z, r, s)
    t = {False: [], True: []}
    for rep in range(repeats):
        for on in (False, True):                       # the two take turns
            prover.set_checked(on)
            prover.prove(z, r, s)
            t0 = time.time()
            proof = prover.prove(z, r, s)
            t[on].append((time.time() - t0) * 1e3)
            assert (proof == ref).all()
    prover.set_checked(False)
    a, b = statistics.median(t[False]), statistics.median(t[True])
    out.append("  %s, one proof alone: unchecked %s; checked %s; ratio checked / unchecked %.4f" % (name, spread(t[False]), spread(t[True]), b / a))


def prover_leg(zk, bench, fs, out):
    pr = zk.Prover(fs.crs, fs.desc)
    checked_turns(zk, pr, fs.z, fs.rr, fs.ss, "prover_2_20", out)
    pr.free()
    nvk_l, npr, nin, trapdoor = bench.aggregator_inputs(1)
    agg = zk.AggregatorCircuit(2, 1)
    desc = zk.r1cs_desc_from_aggregator(agg)
    kp = zk.Keypair(desc, *trapdoor)
    crs = kp.upload_crs()
    pr = zk.Prover(crs, desc)
    z = agg.witness(nvk_l, npr, nin)
    checked_turns(zk, pr, z, fs.rr, fs.ss, "wrapping circuit (batch 2)", out)
    pr.free(); crs.free(); kp.free(); agg.free()


CHILD = r"""
import json, sys, time
sys.path.insert(0, %r)
import bench
from zecale_amd import zkhip as zk
zk.init(0)
fs = bench.FullSizeProver(zk, 20)
r1 = fs.r1
zk.groth16_prove(fs.crs, r1, fs.z, fs.rr, fs.ss)
ts = []
for _ in range(5):
    t0 = time.time(); zk.groth16_prove(fs.crs, r1, fs.z, fs.rr, fs.ss); ts.append((time.time() - t0) * 1e3)
print("RESULT " + json.dumps(ts))
"""


def parent_leg(parent_lib, repeats, steps, warmup, out):
    libs = {"parent": parent_lib, "this": os.path.join(ROOT, "zecale_amd", "libzkhip.so")}
    head = {k: [] for k in libs}
    alone = {k: [] for k in libs}
    for rep in range(repeats):
        for k, lib in libs.items():                    # the two builds take turns
            env = dict(os.environ, ZKHIP_LIB=lib)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               env=env, capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            head[k].append(float(json.loads(line)["value"]))
            p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=900)
            ts = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            alone[k].append(statistics.median(ts))
    for name, vals, unit in (("headline (bench.py --steps %d --warmup %d), value" % (steps, warmup), head, "per s"), ("one 2^20 proof alone", alone, "ms")):
        out.append("  %s:" % name)
        for k in libs:
            out.append("    %-6s %s" % (k, spread(vals[k], unit)))
        diff = statistics.median(vals["this"]) - statistics.median(vals["parent"])
        sp = max(vals["parent"]) - min(vals["parent"])
        out.append("    difference of the medians %+.3f %s, the parent's own spread %.3f: %s" % (diff, unit, sp, "INSIDE" if abs(diff) <= sp else "OUTSIDE"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--legs", default="key,prover")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=3, help="runs per build of the parent leg")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_check.txt"))
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    out = ["Key check and checked prover (tools/key_check_ab.py): one process, one GPU", ""]
    if legs & {"key", "prover"}:
        import bench
        from zecale_amd import zkhip as zk
        zk.init(0)
        fs = None
        if "key" in legs:
            out.append("KEY CHECK")
            fs = key_leg(zk, bench, out)
            out.append("")
        if "prover" in legs:
            out.append("CHECKED PROVER (same build, checking off and on take turns)")
            fs = fs or bench.FullSizeProver(zk, 20)
            prover_leg(zk, bench, fs, out)
            out.append("")
        if fs:
            fs.free()
    if "parent" in legs:
        if not a.parent_lib:
            ap.error("--parent-lib: the parent build's libzkhip.so")
        out.append("NO REGRESSION (both features off; this build against the parent's, child processes taking turns)")
        parent_leg(a.parent_lib, a.repeats, a.steps, a.warmup, out)
        out.append("")
    text = "\n".join(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
