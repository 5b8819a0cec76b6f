"""Per-SF kernel times out of a rocprofv3 kernel trace of tools/bench_soft.py (the aggregate kernel_stats.csv mixes the spreading factors):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_soft.py --runs 5
    python tools/soft_kernel_summary.py DIR/*/*_kernel_trace.csv [--windows 4096] [--sf 7 --sf 9 --sf 12]

bench_soft.py launches, per spreading factor, soft_symbols_kernel and then detect_windows_kernel over --windows windows (2 warm-ups + runs
each, one workgroup of 256 threads per window): the runs of consecutive full-grid launches of either kernel are taken in that order.  One
line per kernel and SF: launches, median and smallest duration, median per window."""
import argparse
import csv
import statistics


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace")
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--sf", type=int, action="append")
    a = ap.parse_args()
    rows = sorted(csv.DictReader(open(a.trace)), key=lambda r: int(r["Start_Timestamp"]))
    groups = {"soft_symbols_kernel": [], "detect_windows_kernel": []}
    last = None
    for r in rows:
        name = next((k for k in groups if k in r["Kernel_Name"]), None)
        if name is None or int(r["Grid_Size_X"]) != a.windows * 256: # (copies, the decode calls' launches)
            continue
        if name != last:
            groups[name].append([])
            last = name
        groups[name][-1].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, runs in groups.items():
        for sf, us in zip(a.sf or (7, 9, 12), runs):
            med = statistics.median(us)
            print("%s SF%d: %d launches of %d windows, median %.1f us, min %.1f us, %.1f ns per window" % (name, sf, len(us), a.windows, med, min(us), 1e3 * med / a.windows))


if __name__ == "__main__":
    main()
