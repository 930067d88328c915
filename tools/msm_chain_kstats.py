#!/usr/bin/env python3
"""The launches behind the bucket accumulation, per MSM, from a rocprofv3 --kernel-trace --stats directory of `bench.py --serial`
(one MSM at a time).  usage: msm_chain_kstats.py <dir> [label]
Behind the accumulation: the stitching (k_fixup_fold, k_fixup) and the bucket reduction (k_sum_lds, k_sum, k_place_hilo and the tail:
k_seg / k_window_combine / k_hilo_combine before the plane form, k_plane_sum / k_plane_combine after it)."""
import csv
import glob
import sys

BEHIND = ("k_fixup", "k_sum", "k_seg", "k_place_hilo", "k_window_combine", "k_hilo_combine", "k_plane_")
FRONT = ("k_digit_pass", "k_bucket_sort", "k_scan_", "k_slice_weights", "k_bucket_order", "k_slots_clear")


def main():
    d = sys.argv[1]
    label = sys.argv[2] if len(sys.argv) > 2 else d
    f = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    short = lambda r: r["Name"].split("(")[0].replace("void ", "").replace("zkhip::", "")
    n = sum(int(r["Calls"]) for r in rows if "k_accumulate_edw_lock" in r["Name"]) or 1
    print("== %s (%d MSMs)\n# kernel, dispatches, mean ms, total ms" % (label, n))
    tot = {"behind": [0, 0.0], "front": [0, 0.0], "acc": [0, 0.0]}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        nm = short(r)
        if nm in ("k_table_build", "k_half_bases", "k_fixed_base_mul", "k_table_edw", "k_bases_to_dev"):
            continue
        print("%-40s %6s %9.3f %9.2f" % (nm, r["Calls"], float(r["AverageNs"]) / 1e6, float(r["TotalDurationNs"]) / 1e6))
        kind = "behind" if nm.startswith(BEHIND) else "front" if nm.startswith(FRONT) else "acc" if nm.startswith("k_accumulate") else None
        if kind:
            tot[kind][0] += int(r["Calls"])
            tot[kind][1] += float(r["TotalDurationNs"]) / 1e6
    print("# per MSM: accumulation kernels %.3f ms; stitching + reduction behind them %.3f ms in %.1f launches; sort, scans and slot clear in front %.3f ms in %.1f launches"
          % (tot["acc"][1] / n, tot["behind"][1] / n, tot["behind"][0] / n, tot["front"][1] / n, tot["front"][0] / n))


if __name__ == "__main__":
    main()
