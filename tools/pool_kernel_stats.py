"""Kernel times of the embedding templates (csrc/trl_pool.hip) by the method of profiles/track_kernel_stats.csv: rocprofv3 kernel
trace, one process per row count, 2 calls of warm-up and 5 measured per id pattern.

    python tools/pool_kernel_stats.py --all out_dir > profiles/pool_kernel_stats.csv        # every shape, then the table
    rocprofv3 --kernel-trace -d out_dir/M -o t -f csv -- python3 tools/pool_kernel_stats.py run M       (what --all starts)
    python tools/pool_kernel_stats.py --table out_dir

A shape is M rows (2^16, 2^20) of normal float32 under one id pattern: "one" (every row in group 0: the contention case), "runs16"
(runs of 16 equal ids, a tracker's output or a sorted gallery), "random4096" (uniform over 4,096 groups) and "distinct" (a group per
row).  Per call: trl_pool_reset, trl_pool_add, trl_pool_finish and trl_pool_rep_add at the default tile, on one stream.  A row of
the table is one kernel of one shape: the median, smallest and largest of the 5 measured launches; beside it the time HBM needs to
read the rows once (M x 2 KB at the 6.29 TB/s a float4 copy reaches), the bytes k_pool_add adds atomically per second (8 bytes per
distinct (group in tile, element): the measured 64-bit integer atomic rate at this contention), and the median of
torch.nn.functional.normalize + index_add_ on the same data (HIP events, same process, same counts), which gives a float sum whose
bits depend on the order of arrival.  Timings are reported, not gated."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS, WARMUP, WARM, TILE = (1 << 16, 1 << 20), 2, 5, 32
PATTERNS = ("one", "runs16", "random4096", "distinct")
KERNELS = ("k_pool_add", "k_pool_finish", "k_pool_rep_add")
HBM_BYTES_PER_S = 6.29e12


def ids_of(pattern, m, gen):
    import torch
    i = torch.arange(m, device="cuda", dtype=torch.int64)
    if pattern == "one":
        return torch.zeros_like(i), 1
    if pattern == "runs16":
        return i // 16, m // 16
    if pattern == "random4096":
        return torch.randint(0, 4096, (m,), generator=gen, device="cuda"), 4096
    return i, m


def run(m):
    import torch
    import truely_amd
    gen = torch.Generator(device="cuda").manual_seed(m)
    x = torch.randn((m, 512), generator=gen, device="cuda")
    info = {"rows": m, "patterns": {}}
    for pattern in PATTERNS:
        ids64, groups = ids_of(pattern, m, gen)
        ids = ids64.to(torch.int32)
        # distinct (group, tile) pairs: what k_pool_add sends out, 512 adds of 8 bytes each
        pairs = int(torch.unique(ids64 * ((m + TILE - 1) // TILE) + torch.arange(m, device="cuda") // TILE).numel())
        pool = truely_amd.EmbeddingPool(groups)
        torch.cuda.synchronize()
        for _ in range(WARMUP + WARM):
            pool.reset()
            pool.add(x, ids)
            r = pool.result()
            pool._representatives(r["template"], lambda: iter([(0, x, None)]), ids, None)
        torch.cuda.synchronize()
        times = []
        acc = torch.zeros((groups, 512), device="cuda")
        for _ in range(WARMUP + WARM):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            acc.zero_()
            acc.index_add_(0, ids64, torch.nn.functional.normalize(x, dim=1))
            torch.nn.functional.normalize(acc, dim=1)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        info["patterns"][pattern] = {"groups": groups, "pairs": pairs, "torch_us": statistics.median(times[-WARM:])}
        del pool, r, acc
    print(json.dumps(info))


def _trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    return sorted(rows)


def table(out):
    print("rows,pattern,groups,kernel,launches,median_us,min_us,max_us,hbm_read_floor_us,atomic_added_GB_per_s,torch_normalize_index_add_us")
    for m in ROWS:
        d = os.path.join(out, str(m))
        info = json.load(open(os.path.join(d, "info.json")))
        tr = _trace(d)
        floor = m * 2048 / HBM_BYTES_PER_S * 1e6
        for k in KERNELS:
            t = [(e - s) / 1e3 for s, e, name in tr if k in name]
            per = WARMUP + WARM
            assert len(t) == per * len(PATTERNS), (m, k, len(t))
            for p, pattern in enumerate(PATTERNS):
                pi = info["patterns"][pattern]
                tp = t[p * per:(p + 1) * per][-WARM:]
                med = statistics.median(tp)
                rate = f"{pi['pairs'] * 512 * 8 / med / 1e3:.1f}" if k == "k_pool_add" else ""
                print(f"{m},{pattern},{pi['groups']},{k},{len(tp)},{med:.1f},{min(tp):.1f},{max(tp):.1f},{floor:.1f},{rate},{pi['torch_us']:.1f}")


def run_all(out):
    for m in ROWS:
        d = os.path.join(out, str(m))
        os.makedirs(d, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "run", str(m)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"{m} rows failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, file=sys.stderr, flush=True)
        open(os.path.join(d, "info.json"), "w").write(line)
    table(out)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(int(sys.argv[2]))
    elif len(sys.argv) == 3 and sys.argv[1] == "--all":
        run_all(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        sys.exit(__doc__)
