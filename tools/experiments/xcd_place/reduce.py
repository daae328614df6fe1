"""Reduce the rocprofv3 output folders of tools/experiments/xcd_place/profile.sh into two tables:
    python tools/experiments/xcd_place/reduce.py ROOT pmc.tsv times.tsv
ROOT/<run>_pmc_*/ hold counter_collection.csv files (one --pmc run each), ROOT/<run>_trace/ a kernel_stats.csv.
pmc.tsv:   run, kernel, counter, launches, mean per launch       (the c2 kernels only)
times.tsv: run, kernel, launches, mean, min, max and standard deviation in us"""
import collections
import csv
import glob
import os
import re
import sys

KERNEL = re.compile(r"(k_(?:layer|chain|gather)<[^>]*>)")


def main():
    root, pmc_out, times_out = sys.argv[1:4]
    acc = collections.defaultdict(list)
    for d in sorted(glob.glob(os.path.join(root, "*_pmc_*"))):
        run = os.path.basename(d).split("_pmc_")[0]
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                m = KERNEL.search(r["Kernel_Name"])
                if m:
                    acc[(run, m.group(1), r["Counter_Name"])].append(float(r["Counter_Value"]))
    with open(pmc_out, "w") as o:
        o.write("run\tkernel\tcounter\tlaunches\tmean_per_launch\n")
        for (run, k, c), v in sorted(acc.items()):
            o.write(f"{run}\t{k}\t{c}\t{len(v)}\t{sum(v) / len(v):.1f}\n")
    with open(times_out, "w") as o:
        o.write("run\tkernel\tlaunches\tmean_us\tmin_us\tmax_us\tstddev_us\n")
        for d in sorted(glob.glob(os.path.join(root, "*_trace"))):
            run = os.path.basename(d)[:-len("_trace")]
            for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    m = KERNEL.search(r["Name"])
                    if m:
                        o.write(f"{run}\t{m.group(1)}\t{r['Calls']}\t{float(r['AverageNs']) / 1e3:.2f}\t"
                                f"{float(r['MinNs']) / 1e3:.2f}\t{float(r['MaxNs']) / 1e3:.2f}\t{float(r['StdDev']) / 1e3:.2f}\n")


if __name__ == "__main__":
    main()
