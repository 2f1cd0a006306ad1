"""Condenses a rocprofv3 --kernel-trace CSV of `bench.py --only-headline`: did level 0's k_fast run beside the resize chain (csrc/orb.hip: orb_enqueue_kernels)?
A step is cut at every k_describe.  Per step: the span of the resize launches, start and end of each k_fast launch against the step's first kernel, the
microseconds the first k_fast overlaps the resize span, and each kernel's duration; then the means over the steps whose batch is the full one.
    python tools/fast_overlap_trace.py <kernel_trace.csv> [steps to print, default 5]"""
import csv, re, sys


def main():
    show = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    rows = []
    for r in csv.DictReader(open(sys.argv[1])):
        m = re.search(r"k_\w+", r["Kernel_Name"])
        if m:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), m.group(0), r.get("Queue_Id", "?")))
    rows.sort()
    steps, cur = [], []
    for k in rows:
        cur.append(k)
        if k[2] == "k_describe":
            steps.append(cur); cur = []
    out = []
    for s in steps:
        rs = [k for k in s if k[2].startswith("k_resize")]
        fs = [k for k in s if k[2] == "k_fast"]
        if not rs or not fs:
            continue
        t0 = min(k[0] for k in rs + fs)          # (the matcher's kernels of the step before lie in front of it)
        r0, r1 = min(k[0] for k in rs), max(k[1] for k in rs)
        f = fs[0]
        out.append(dict(resize=(r0 - t0, r1 - t0), resize_sum=sum(k[1] - k[0] for k in rs), fast=[(k[0] - t0, k[1] - t0, k[3]) for k in fs],
                        overlap=max(0, min(f[1], r1) - max(f[0], r0)) if len(fs) > 1 else 0, select=[k[0] - t0 for k in s if k[2] == "k_select"][:1],
                        span=max(k[1] for k in s) - t0, describe=[k[1] - k[0] for k in s if k[2] == "k_describe"][0]))
    big = max(o["resize_sum"] for o in out)
    full = [o for o in out if o["resize_sum"] > 0.7 * big]                 # the 256-frame steps (the bench also runs smaller calls)
    us = lambda ns: ns / 1e3
    for o in full[:show]:
        print("step: resize %.1f .. %.1f us (kernels %.1f us)  " % (us(o["resize"][0]), us(o["resize"][1]), us(o["resize_sum"])) +
              "  ".join("k_fast[q%s] %.1f .. %.1f (%.1f us)" % (q, us(a), us(b), us(b - a)) for a, b, q in o["fast"]) +
              "  overlap %.1f us  k_select at %s  step span %.1f us" % (us(o["overlap"]), "/".join("%.1f" % us(t) for t in o["select"]), us(o["span"])))
    n = len(full)
    mean = lambda f: sum(f(o) for o in full) / n
    nf = max(len(o["fast"]) for o in full)
    print("%d full steps, %d k_fast launch(es) per step; means: resize span %.1f us (its kernels alone %.1f us), " % (n, nf, us(mean(lambda o: o["resize"][1] - o["resize"][0])), us(mean(lambda o: o["resize_sum"]))) +
          ", ".join("k_fast #%d %.1f us" % (i, us(mean(lambda o: o["fast"][i][1] - o["fast"][i][0]))) for i in range(nf) if all(len(o["fast"]) > i for o in full)) +
          ", overlap %.1f us, k_describe %.1f us, step span (first extractor kernel to k_describe's end) %.1f us" % (us(mean(lambda o: o["overlap"])), us(mean(lambda o: o["describe"])), us(mean(lambda o: o["span"]))))


if __name__ == "__main__":
    main()
