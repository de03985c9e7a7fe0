#!/usr/bin/env python3
"""Per-launch timeline of the three headline kernels from a rocprofv3 --kernel-trace CSV: duration of every launch, the gap to the
previous launch on the device, and the spread over the run -- what `ms_per_step` is made of when the kernels take 0.1-0.2 ms.
usage: trace_launches.py <p_kernel_trace.csv> [--timed-steps K]
--timed-steps K: the trace is of a plain `bench.py --steps K` run, whose last 3 K launches are the timed steps (an event record
before and after every launch) and whose earlier ones the untimed settle and warm-up steps (no records): one table for each."""
import csv
import sys

KEYS = (("sad_nxn_kernel<8", "sad_8x8"), ("satd8_kernel", "satd_8x8"), ("dct32_mfma_kernel<32, false", "dct_32x32"))


def table(title, launches):
    """launches: (start, end, kernel, gap before it or None) in the order they ran"""
    per = {}
    for (s, e, k, gap) in launches:
        d = per.setdefault(k, {"dur": [], "gap": []})
        d["dur"].append((e - s) / 1e3)
        if gap is not None:
            d["gap"].append(gap / 1e3)
    if title:
        print(title)
    print("kernel        launches   duration us: mean  median     min     max    p90 | gap before launch us: mean  median     max")
    for k, d in per.items():
        du, ga = sorted(d["dur"]), sorted(d["gap"]) or [0.0]
        print("%-12s %9d %19.1f %7.1f %7.1f %7.1f %6.1f | %27.1f %7.1f %7.1f"
              % (k, len(du), sum(du) / len(du), du[len(du) // 2], du[0], du[-1], du[int(len(du) * 0.9)], sum(ga) / len(ga), ga[len(ga) // 2], ga[-1]))
    return per


def busy(launches):
    if launches:
        first, last = launches[0][0], launches[-1][1]
        b = sum(e - s for (s, e, _, _) in launches)
        print("device busy with these kernels %.1f %% of the %.2f ms between the first start and the last end" % (100.0 * b / (last - first), (last - first) / 1e6))


def main():
    args = sys.argv[1:]
    timed_steps = 0
    if "--timed-steps" in args:
        i = args.index("--timed-steps")
        timed_steps = int(args[i + 1])
        del args[i:i + 2]
    rows = []
    for r in csv.DictReader(open(args[0])):
        name = r.get("Kernel_Name", "")
        k = next((v for p, v in KEYS if p in name), None)
        if k:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k))
    rows.sort()
    launches, prev_end = [], None
    for (s, e, k) in rows:
        launches.append((s, e, k, None if prev_end is None else s - prev_end))
        prev_end = e
    per = table("", launches)
    # the launches in the order they ran (warm-up first): is the spread a drift, an alternation, or scattered?
    for k, d in per.items():
        print("%-10s in order: %s" % (k, " ".join("%.0f" % v for v in d["dur"])))
    busy(launches)
    if timed_steps and len(launches) > 3 * timed_steps:
        untimed, timed = launches[:-3 * timed_steps], launches[-3 * timed_steps:]
        print()
        table("untimed launches (settle and warm-up steps: no event records between the launches)", untimed)
        busy(untimed)
        print()
        table("timed launches (the last %d steps: an event record before and after every launch)" % timed_steps, timed)
        busy(timed)
        for k in ("sad_8x8", "satd_8x8", "dct_32x32"):
            print("%-10s gaps in order: %s" % (k, " ".join("%.1f" % (g / 1e3) for (_, _, kk, g) in timed if kk == k and g is not None)))


if __name__ == "__main__":
    main()
