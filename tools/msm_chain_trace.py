#!/usr/bin/env python3
"""The launch chains around the bucket accumulation, read from ONE rocprofv3 --kernel-trace of the MSM stream
(python bench.py --steps S --warmup W).  usage: msm_chain_trace.py <dir with *kernel_trace.csv> [timed MSMs, default 20]

Prints, for the last `timed` accumulations of the run (the timed region; the warm-up and the set-up launches come before them):
  * per MSM the time from its first digit pass to the start of its accumulation (front chain) and from the end of its accumulation
    to the end of its last kernel (back chain; the copy of the window results to the host follows and is not a kernel);
  * how many accumulations are in flight at each instant: the share of the region with 0 / 1 / 2 / 3+;
  * the launches between two accumulations of one stream.
A launch sequence is one stream's (Stream_Id column) when the trace has it, one hardware queue's (Queue_Id) otherwise - contexts
that share a queue are then told apart by order only, and the chain figures are upper bounds."""
import csv
import glob
import sys
from collections import defaultdict


def is_acc(name):
    """the Edwards accumulation launch that does the work on the lockstep route"""
    return "k_accumulate_edw_lock" in name


def queue_table(rows, t0, t1):
    """per hardware queue: the timed accumulations (primary streams) and the k_sum_edw launches of the region (both streams of a
    context launch them: the column tree's are the secondary stream's only kernels) with the distinct streams they came from"""
    if "Queue_Id" not in rows[0]:
        print("the trace has no Queue_Id column: no per-queue table")
        return
    has_stream = "Stream_Id" in rows[0]
    for title, pick in (("accumulations", is_acc), ("k_sum_edw launches", lambda nm: "k_sum_edw" in nm)):
        per = defaultdict(lambda: [0, set()])
        for r in rows:
            if pick(r["Kernel_Name"]) and t0 <= int(r["Start_Timestamp"]) <= t1:
                per[r["Queue_Id"]][0] += 1
                per[r["Queue_Id"]][1].add(r["Stream_Id"] if has_stream else "?")
        print("%s of the region per Queue_Id: launches, distinct Stream_Ids" % title)
        for q in sorted(per, key=lambda x: (len(x), x)):
            print("  queue %-6s %5d  %3d  streams %s" % (q, per[q][0], len(per[q][1]), " ".join(sorted(per[q][1], key=lambda x: (len(x), x)))))
    allq = sorted({r["Queue_Id"] for r in rows}, key=lambda x: (len(x), x))
    print("queues in the whole trace: %s" % " ".join(allq))


def main():
    d = sys.argv[1]
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no kernel_trace.csv under " + d)
    rows = list(csv.DictReader(open(files[0])))
    key = "Stream_Id" if "Stream_Id" in rows[0] and len({r["Stream_Id"] for r in rows}) > 2 else "Queue_Id"
    ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r[key]) for r in rows]
    ev.sort()
    acc = [e for e in ev if is_acc(e[2])]
    if len(acc) < timed:
        sys.exit("only %d accumulations in the trace" % len(acc))
    acc = acc[-timed:]
    t0, t1 = acc[0][0], max(e[1] for e in acc)
    print("sequences keyed by %s; %d accumulations, region %.2f ms (first start to last end), %.3f ms per MSM" % (key, timed, (t1 - t0) / 1e6, (t1 - t0) / 1e6 / timed))
    # in-flight histogram
    marks = sorted([(s, 1) for s, e, _, _ in acc] + [(e, -1) for s, e, _, _ in acc])
    hist, n, last = defaultdict(int), 0, t0
    for t, dlt in marks:
        hist[min(n, 3)] += t - last
        last, n = t, n + dlt
    tot = float(t1 - t0)
    print("accumulations in flight, share of the region:  0: %.1f %%   1: %.1f %%   2: %.1f %%   3+: %.1f %%" % tuple(100 * hist[k] / tot for k in range(4)))
    print("mean accumulation duration %.3f ms (min %.3f, max %.3f)" % (sum(e - s for s, e, _, _ in acc) / 1e6 / timed, min(e - s for s, e, _, _ in acc) / 1e6, max(e - s for s, e, _, _ in acc) / 1e6))
    # chains per sequence
    by = defaultdict(list)
    for e in ev:
        by[e[3]].append(e)
    front, back, nback, busy_back = [], [], [], []
    for s, e, _, k in acc:
        seq = by[k]
        before = [x for x in seq if x[0] < s]
        first = None
        for x in reversed(before):               # walk back to this sequence's first digit pass
            if "k_digit_pass<0" in x[2]:
                first = x
                break
            if is_acc(x[2]):
                break
        after = []
        for x in seq:
            if x[0] >= e:
                if "k_digit_pass<0" in x[2] or is_acc(x[2]):
                    break
                after.append(x)
        if first:
            front.append((s - first[0]) / 1e6)
        if after:
            back.append((max(x[1] for x in after) - e) / 1e6)
            nback.append(len(after))
            busy_back.append(sum(x[1] - x[0] for x in after) / 1e6)
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    print("front chain (first digit pass -> accumulation starts): mean %.3f ms, min %.3f, max %.3f  (%d sequences)" % (mean(front), min(front, default=0), max(front, default=0), len(front)))
    print("back chain (accumulation ends -> last kernel of the sequence on that %s ends): mean %.3f ms, min %.3f, max %.3f; %.1f launches, %.3f ms of kernel durations" % (key, mean(back), min(back, default=0), max(back, default=0), mean(nback), mean(busy_back)))
    queue_table(rows, t0, t1)
    names = defaultdict(lambda: [0, 0])
    for s, e, nm, _ in ev:
        if s >= t0 and e <= t1:
            nm = nm.split("(")[0].replace("void ", "").replace("zkhip::", "")
            names[nm][0] += 1
            names[nm][1] += e - s
    print("kernels inside the region: launches per MSM, mean us")
    for nm, (c, t) in sorted(names.items(), key=lambda kv: -kv[1][1]):
        print("  %-34s %6.2f  %9.1f" % (nm, c / timed, t / 1e3 / c))


if __name__ == "__main__":
    main()
