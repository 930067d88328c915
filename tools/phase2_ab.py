#!/usr/bin/env python3
"""The measurements of phase-2 contributions, one process on one GPU (the no-regression leg starts one child process per run).

Legs (--legs, comma list):
  contribute  zkhip_keypair_contribute on the key of the 2^20 - 8 constraint system (the `prover_2_20` key of bench.py): whole call, per
              vector with staging, the longest single launch, five repeats; in the same run k_key_point_check on the same H vector
              (the chain the new kernel is compared with: 377 doublings + 135 additions, medians of five); then the device and the host route (16 threads) on the SAME 2^14-point slices of H and L, the host's
              time also scaled to the whole key and labelled as scaled.
  forms       the two forms of the kernel - the signed-binary baseline over all of s^-1 and the endomorphism form - taking turns on
              the same key, medians of five: needs a library built with -DZKHIP_PHASE2_BOTH_FORMS (ZKHIP_LIB names it; a normal
              build holds the faster form only).  Outputs must be identical.
  verify      zkhip_phase2_verify of that contribution: whole call, point checks / sums / host relations, the longest launch.
  parent      with the feature unused: the headline (python bench.py) and one 2^20 proof alone against ANOTHER build of the library
              (--parent-lib: the parent commit's libzkhip.so), the two builds taking turns, child processes (tools/key_check_ab.py's
              leg).  The difference must lie inside the parent's own spread of repeats.

Written to --out (profiles/phase2.txt holds the run this repository's figures come from)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.key_check_ab import parent_leg, spread      # noqa: E402


def forms_leg(zk, fs, out):
    import hashlib
    from tests import phase2_fixtures as F
    pk, m, l, d = fs.kp.pk_arrays()
    nh, nl = d - 1, m - l - 1
    sk, kk = F.scalar_limbs(F.S1), F.scalar_limbs(F.K1)
    names = {1: "baseline (signed binary over s^-1)", 2: "endomorphism (k1 + k2 lambda)"}
    walls, vec, longest, launches, digest = ({f: [] for f in names} for _ in range(5))
    for rep in range(5):
        for f in names:                                # the two forms take turns
            zk.phase2_set_form(f)
            t0 = time.time()
            new = fs.kp.contribute(sk, kk)
            walls[f].append((time.time() - t0) * 1e3)
            ms = zk.phase2_last_ms()
            vec[f].append(ms[1] + ms[2]); longest[f].append(ms[0]); launches[f].append(ms[7])
            a = new[0].pk_arrays()[0]
            digest[f].append(hashlib.sha256(a["H"].tobytes() + a["L"].tobytes() + new[1].to_bytes()).hexdigest())
            new[0].free()
    zk.phase2_set_form(0)
    assert len({x for f in names for x in digest[f]}) == 1, "the two forms disagree"
    out.append("  the same contribution (fixed s, k) by both forms, taking turns, five repeats each; H, L and the record identical in all ten (SHA-256 of the arrays)")
    for f, name in names.items():
        out.append("    %-36s h_query + l_query %s" % (name, spread(vec[f])))
        out.append("    %-36s   longest launch %s; all launches %s; whole call %s" % ("", spread(longest[f]), spread(launches[f]), spread(walls[f])))
    r = lambda v: statistics.median(v[2]) / statistics.median(v[1])
    out.append("    endomorphism / baseline: longest launch %.3f, all launches %.3f, the two vectors with staging %.3f, whole call %.3f" %
               (r(longest), r(launches), r(vec), r(walls)))
    out.append("    (products per point: 377 doublings + ~126 additions = 5.0 k against ~190 doublings + 2 x ~63 additions + 2 x 63 products by omega = 3.3 k: 0.66)")
    out.append("    what copies overlapped with kernels could hide, endomorphism form: vectors with staging %.1f ms - all launches %.1f ms = %.1f ms of %d points' copies in and out" %
               (statistics.median(vec[2]), statistics.median(launches[2]), statistics.median(vec[2]) - statistics.median(launches[2]), nh + nl))


def contribute_leg(zk, fs, out):
    import numpy as np
    pk, m, l, d = fs.kp.pk_arrays()
    nh, nl = d - 1, m - l - 1
    out.append("key of the 2^20 - 8 constraint system: n_vars %d, n_primary %d, domain %d: H %d + L %d = %d points to multiply" % (m, l, d, nh, nl, nh + nl))
    walls, last, new = [], None, None
    for rep in range(5):
        if new:
            new[0].free()
        t0 = time.time()
        new = fs.kp.contribute()
        walls.append((time.time() - t0) * 1e3)
        last = zk.phase2_last_ms()
    out.append("  zkhip_keypair_contribute, whole call (the new keypair's host copy included): %s" % spread(walls))
    out.append("  last call: h_query %.1f ms (%.0f ns / point, staging included), l_query %.1f ms (%.0f ns / point); all launches of the kernel %.1f ms; "
               "the copy of the key %.1f ms, delta' in both groups %.1f ms, commitment, response and hashes %.1f ms; the Python wrapper and the rest %.1f ms" %
               (last[1], last[1] * 1e6 / nh, last[2], last[2] * 1e6 / nl, last[7], last[4], last[5], last[6], walls[-1] - sum(last[k] for k in (1, 2, 4, 5, 6))))
    out.append("  LONGEST SINGLE LAUNCH of k_common_scalar_mul (chunk 2^17 points, device time): %.2f ms = %.0f ns / point" % (last[0], last[0] * 1e6 / (1 << 17)))
    # the point check's kernel on the same H vector, in the same run
    h_only = (dict(pk, A=pk["A"][:1], B2=pk["B2"][:1], B1=pk["B1"][:1], L=pk["L"][:0]), 1, 0, d)
    kcs = []
    for _ in range(5):
        rep = zk.check_key(h_only, rho=[1])
        kcs.append(zk.key_check_last_ms())
    kc = [statistics.median(c[k] for c in kcs) for k in range(len(kcs[0]))]      # medians of five
    out.append("  k_key_point_check on the same h_query, medians of five: %.1f ms with staging (%.0f ns / point), its longest launch %.2f ms = %.0f ns / point" %
               (kc[4 + 8], kc[4 + 8] * 1e6 / nh, kc[0], kc[0] * 1e6 / (1 << 17)))
    out.append("  ratio of the longest launches, k_common_scalar_mul / k_key_point_check: %.3f (the chains: ~190 doublings + ~126 additions + 126 products by "
               "omega + one inversion + 24 limbs written, against 377 doublings + 135 additions + one byte written: 3.3 k against 5.1 k products, 0.65)" % (last[0] / kc[0]))
    assert rep.e[8].first_refused == zk.NONE_INDEX
    # the same points on both routes: 2^14-point slices of H and L
    s = 1 << 14
    import tempfile
    from tests import key_check_fixtures as K
    from tests import phase2_fixtures as F
    pts = lambda a: [K.Pt(p, 0, None) for p in a]
    sl = K.Key(s, 0, s, dict(alpha_g1=pts([pk["alpha_g1"]]), beta_g1=pts([pk["beta_g1"]]), beta_g2=pts([pk["beta_g2"]]), delta_g1=pts([pk["delta_g1"]]),
                             delta_g2=pts([pk["delta_g2"]]), a_query=pts(pk["A"][:s]), b_g2_query=pts(pk["B2"][:s]), b_g1_query=pts(pk["B1"][:s]),
                             h_query=pts(pk["H"][:s - 1]), l_query=pts(pk["L"][:s - 1]), vk_abc=pts(pk["A"][:1])))
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        kp = F.keypair_of(zk, sl, pathlib.Path(tmp))
    sk, kk = F.scalar_limbs(F.S1), F.scalar_limbs(F.K1)
    dev, host = [], []
    for rep in range(3):
        t0 = time.time(); a = kp.contribute(sk, kk); dev.append((time.time() - t0) * 1e3)
        dm = zk.phase2_last_ms()
        t0 = time.time(); b = kp.contribute(sk, kk, host=True); host.append((time.time() - t0) * 1e3)
        hm = zk.phase2_last_ms()
        assert all((a[0].pk_arrays()[0][k] == b[0].pk_arrays()[0][k]).all() for k in ("H", "L")) and a[1].to_bytes() == b[1].to_bytes()
        a[0].free(); b[0].free()
    n_sl = 2 * (s - 1)
    out.append("  the SAME %d points (2^14 - 1 of H and of L) on both routes, whole call:" % n_sl)
    out.append("    device: %s;  host, %d threads: %s" % (spread(dev), min(16, os.cpu_count() or 1), spread(host)))
    out.append("    the two vectors alone (last repeat): device %.1f ms, host %.1f ms: ratio %.1f" % (dm[1] + dm[2], hm[1] + hm[2], (hm[1] + hm[2]) / (dm[1] + dm[2])))
    out.append("    host route SCALED to the whole key's %d points (x %.1f): %.1f s against the device's %.2f s measured (h_query + l_query)" %
               (nh + nl, (nh + nl) / n_sl, (hm[1] + hm[2]) * (nh + nl) / n_sl / 1e3, (last[1] + last[2]) / 1e3))
    kp.free()
    return new


def verify_leg(zk, fs, new, out):
    walls = []
    for rep in range(5):
        t0 = time.time()
        report, digest = zk.phase2_verify(fs.kp, new[0], new[1], b"\0" * 32)
        walls.append((time.time() - t0) * 1e3)
        assert report.ok and digest == new[2], report.describe()
        ms = zk.phase2_last_ms()
    out.append("  zkhip_phase2_verify of that contribution, whole call: %s" % spread(walls))
    out.append("  last call: byte comparison of the unchanged elements %.1f ms, point checks of the new points %.1f ms, infinity patterns %.1f ms, the four sums "
               "(MSM engine, H and L of both keys) %.1f ms, the two pairing products and the proof of knowledge on the host %.1f ms; rest (the scalars from "
               "the OS and their six-word form, descriptors, the Python wrapper) %.1f ms" %
               (ms[1], ms[4], ms[2], ms[5], ms[6], walls[-1] - ms[1] - ms[2] - ms[4] - ms[5] - ms[6]))
    out.append("  LONGEST SINGLE LAUNCH of k_key_point_check in it (device time): %.2f ms" % ms[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--legs", default="contribute,verify")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=3, help="runs per build of the parent leg")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase2.txt"))
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    out = ["Phase-2 contributions (tools/phase2_ab.py): one process, one GPU", ""]
    if legs & {"contribute", "verify", "forms"}:
        import bench
        from zecale_amd import zkhip as zk
        zk.init(0)
        fs = bench.FullSizeProver(zk, 20)
        if "forms" in legs:
            out.append("THE TWO FORMS OF THE KERNEL (a build with both)")
            forms_leg(zk, fs, out)
            out.append("")
        if legs & {"contribute", "verify"}:
            out.append("CONTRIBUTE (the build's own form)")
            new = contribute_leg(zk, fs, out)
            out.append("")
            if "verify" in legs:
                out.append("VERIFY")
                verify_leg(zk, fs, new, out)
                out.append("")
            new[0].free()
        fs.free()
    if "parent" in legs:
        if not a.parent_lib:
            ap.error("--parent-lib: the parent build's libzkhip.so")
        out.append("NO REGRESSION (the feature unused; this build against the parent's, child processes taking turns)")
        parent_leg(a.parent_lib, a.repeats, a.steps, a.warmup, out)
        out.append("")
    text = "\n".join(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
