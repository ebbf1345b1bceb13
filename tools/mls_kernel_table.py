"""The launches of mls_kernel and normals_radius_kernel in a rocprofv3 kernel trace of `tools/mls_bench.py --kernels`, grouped in
launch order (consecutive launches of one kernel on one grid size are one group: the tool runs each call --reps times in turn --
radius 1 mm, radius 2.5 mm, the merged object) with the mean, smallest and largest duration of each group in microseconds.
Usage: python tools/mls_kernel_table.py profiles/mls_kernel_trace.csv
"""
import csv
import re
import sys


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups = []
    for r in rows:
        name = r["Kernel_Name"]
        if "mls_kernel" not in name and "normals_radius_kernel" not in name:
            continue
        short = re.search(r"(\w+<[^>]*>)\(", name).group(1)           # e.g. mls_kernel<false, true>
        key = (short, r["Grid_Size_X"])
        d = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if groups and groups[-1][0] == key:
            groups[-1][1].append(d)
        else:
            groups.append((key, [d]))
    print("kernel,grid_x,launches,mean_us,min_us,max_us")
    for (short, grid), d in groups:
        print("%s,%s,%d,%.1f,%.1f,%.1f" % (short.replace(", ", ";"), grid, len(d), sum(d) / len(d) / 1e3, min(d) / 1e3, max(d) / 1e3))


if __name__ == "__main__":
    main()
