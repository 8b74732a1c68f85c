"""Sum a rocprofv3 kernel trace per (kernel, grid size): separates the layers that one kernel instantiation serves.

    rocprofv3 --kernel-trace -d OUT -o s -f csv -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline
    python tools/kernel_trace_by_grid.py OUT/**/s_kernel_trace.csv RUN [substring ...]  > rows.csv

Prints csv rows run, kernel, grid_size_x, calls, total_ns for the kernels whose name holds one of the substrings (default: the
conv_tap family, the max pools and the pooling fix-up -- profiles/tail_pool_kernel_stats.csv), largest total first."""
import collections
import csv
import sys


def by_grid(path, keys):
    agg = collections.defaultdict(lambda: [0, 0])
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if any(k in name for k in keys):
            a = agg[(name, r["Grid_Size_X"])]
            a[0] += 1
            a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return sorted(agg.items(), key=lambda kv: -kv[1][1])


if __name__ == "__main__":
    path, run = sys.argv[1], sys.argv[2]
    keys = sys.argv[3:] or ["conv_tap", "maxpool", "pool_fixup"]
    out = csv.writer(sys.stdout)
    out.writerow(["run", "kernel", "grid_size_x", "calls", "total_ns"])
    for (name, grid), (calls, total) in by_grid(path, keys):
        out.writerow([run, name, grid, calls, total])
