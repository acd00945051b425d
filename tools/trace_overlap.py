#!/usr/bin/env python3
"""Concurrency picture of a rocprofv3 --kernel-trace run: per kernel name the summed duration; over the steady-state window the time with
0 / 1 / 2 / ... kernels in flight (not capped); and per hardware queue (Queue_Id) the kernels it carried and its busy share of that window.
With a Stream_Id column (newer rocprofv3) also which streams fed each queue.  usage: trace_overlap.py <dir>"""
import collections, csv, glob, os, re, sys


def short(name):
    return re.sub(r"\(.*", "", name).replace("void ", "").strip()[:40]


def busy_ns(iv, lo, hi):
    """Length of the union of the intervals `iv`, clipped to [lo, hi]."""
    tot, end = 0, lo
    for s, e in sorted(iv):
        s, e = max(s, end), min(e, hi)
        if e > s:
            tot += e - s; end = e
    return tot


def main(d):
    f = max(glob.glob(d + "/**/*kernel_trace.csv", recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(f))]
    ev, per = [], collections.defaultdict(lambda: [0, 0])
    for r in rows:
        n = short(r["Kernel_Name"])
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        per[n][0] += e - s; per[n][1] += 1
        ev.append((s, 1)); ev.append((e, -1))
    ev.sort()
    # steady state = the middle launches of the kernel the run spends most time in (set-up and tear-down kernels stay outside): from the start
    # of the launch a quarter of the way through to the start of the one at 85 %
    top = max(per, key=lambda n: per[n][0])
    starts = sorted(int(r["Start_Timestamp"]) for r in rows if short(r["Kernel_Name"]) == top)
    lo, hi = starts[len(starts) // 4], starts[len(starts) * 85 // 100]
    if hi <= lo:
        lo, hi = ev[0][0], ev[-1][0]
    print("steady-state window: launches %d .. %d of %d of %s" % (len(starts) // 4, len(starts) * 85 // 100, len(starts), top))
    depth, last, hist = 0, None, collections.Counter()
    for t, dlt in ev:
        if last is not None and t > lo and last < hi:
            hist[depth] += min(t, hi) - max(last, lo)
        depth += dlt; last = t
    tot = sum(hist.values())
    print("window %.2f ms; kernels in flight: " % (tot / 1e6) + ", ".join("%d: %.1f %%" % (k, 100 * v / tot) for k, v in sorted(hist.items())))
    print("  >= 3 in flight: %.1f %%; >= 4: %.1f %%" % (100 * sum(v for k, v in hist.items() if k >= 3) / tot, 100 * sum(v for k, v in hist.items() if k >= 4) / tot))
    # per hardware queue, inside the window: busy share (union of its kernels' intervals), kernel names with launch counts, streams that fed it
    queues = collections.defaultdict(lambda: {"iv": [], "names": collections.Counter(), "streams": collections.Counter()})
    seen = set()
    for r in rows:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        seen.add(r["Queue_Id"])
        if e <= lo or s >= hi:
            continue
        q = queues[r["Queue_Id"]]
        q["iv"].append((s, e)); q["names"][short(r["Kernel_Name"])] += 1
        if r.get("Stream_Id") not in (None, ""):
            q["streams"][r["Stream_Id"]] += 1
    print("distinct queues: %d in the whole trace, %d in the window" % (len(seen), len(queues)))
    for qid, q in sorted(queues.items(), key=lambda x: -len(x[1]["iv"])):
        print("  queue %-4s busy %5.1f %% of the window, %5d kernels%s" % (qid, 100.0 * busy_ns(q["iv"], lo, hi) / (hi - lo), len(q["iv"]),
              ("; streams " + ", ".join("%s x%d" % kv for kv in sorted(q["streams"].items()))) if q["streams"] else ""))
        print("      " + ", ".join("%s x%d" % kv for kv in q["names"].most_common(12)))
    for n, (dur, c) in sorted(per.items(), key=lambda x: -x[1][0])[:14]:
        print("  %-42s %6d calls  %9.3f ms total  %8.1f us avg" % (n, c, dur / 1e6, dur / c / 1e3))


if __name__ == "__main__":
    main(sys.argv[1])
