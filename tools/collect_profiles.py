#!/usr/bin/env python3
"""Builds profiles/<tag>_* from gpurun_out/refresh/ (written by tools/refresh_profiles.sh on the GPU box).

  python tools/collect_profiles.py [tag]        # tag defaults to round4
"""
import csv
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpurun_out", "refresh")
DST = os.path.join(ROOT, "profiles")
tag = sys.argv[1] if len(sys.argv) > 1 else "round4"


def pmc_rows(path, counter):
    """Per-dispatch totals of one counter for the pyramid / PNet kernels (rocprofv3 emits one row per XCD)."""
    rows = list(csv.DictReader(open(path)))
    agg = {}
    for r in rows:
        if r["Counter_Name"] != counter:
            continue
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
        if "k_pnet_fused" not in name and "k_pyramid" not in name:
            continue
        key = (int(r["Dispatch_Id"]), name.split("(")[0])
        agg[key] = agg.get(key, 0.0) + float(r["Counter_Value"])
    return [(k[0], k[1], v) for k, v in sorted(agg.items())]


def main():
    os.makedirs(DST, exist_ok=True)
    shutil.copy(os.path.join(SRC, "bench.json"), os.path.join(DST, f"{tag}_bench.json"))
    shutil.copy(os.path.join(SRC, "stats", "s_kernel_stats.csv"), os.path.join(DST, f"{tag}_bench_kernel_stats.csv"))             # the driver's command (one batch in flight)
    if os.path.exists(os.path.join(SRC, "stats2", "s_kernel_stats.csv")):
        shutil.copy(os.path.join(SRC, "stats2", "s_kernel_stats.csv"), os.path.join(DST, f"{tag}_bench_kernel_stats_inflight2.csv"))  # --in-flight 2
    if os.path.exists(os.path.join(SRC, "bench_inflight2.json")):
        shutil.copy(os.path.join(SRC, "bench_inflight2.json"), os.path.join(DST, f"{tag}_bench_inflight2.json"))
    summ = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "step_timeline.py"), os.path.join(SRC, "stats", "s_kernel_trace.csv"), "2", "--all"],
                          capture_output=True, text=True, check=True).stdout
    open(os.path.join(DST, f"{tag}_step_timeline.txt"), "w").write(summ)
    for name in ("bench_sustained", "bench_config2", "bench_config4", "bench_prelu_general", "bench_prelu_general_inflight1", "bench_ingest_nv12",
                 "bench_gloo2_sharded", "bench_gloo2_streams", "bench_gloo2_streams_nv12", "bench_embed_group3", "bench_config0", "run_config0",
                 "bench_driver_threads", "bench_embed_group1", "bench_embed_group4", "bench_inflight1_group1", "bench_inflight1_group1_nocarry"):
        src = os.path.join(SRC, name + ".json")
        if os.path.exists(src) and os.path.getsize(src) > 0:
            shutil.copy(src, os.path.join(DST, f"{tag}_{name}.json"))
    for sub, out in (("stats_c2", "config2_kernel_stats.csv"), ("stats_c4", "config4_kernel_stats.csv"),
                     ("stats_fn2048", "facenet_2048faces_kernel_stats.csv")):
        src = os.path.join(SRC, sub, "s_kernel_stats.csv")
        if os.path.exists(src):
            shutil.copy(src, os.path.join(DST, f"{tag}_{out}"))
    for sub in ("sq1", "sq2"):
        src = os.path.join(SRC, sub, "p_counter_collection.csv")
        if os.path.exists(src):
            txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pmc_summary.py"), src], capture_output=True, text=True, check=True).stdout
            open(os.path.join(DST, f"{tag}_sq_pmc_{sub}.txt"), "w").write(txt)
    for name in ("pnet_phase_clocks.txt", "pnet_phase_pmc.txt", "front_ablation.txt", "batch_sweep_config1.json", "batch_sweep_config4.json"):
        src = os.path.join(SRC, name)
        if os.path.exists(src) and os.path.getsize(src) > 0:
            shutil.copy(src, os.path.join(DST, f"{tag}_{name}"))
    for name in ("crowded_timing.jsonl", "run_wall_time.json"):
        src = os.path.join(SRC, name)
        if os.path.exists(src) and os.path.getsize(src) > 0:
            shutil.copy(src, os.path.join(DST, f"{tag}_{name}"))
    for name in ("facenet_ms.txt", "facenet_stamps.txt"):
        src = os.path.join(SRC, name)
        if os.path.exists(src):
            shutil.copy(src, os.path.join(DST, f"{tag}_{name}"))
    per_launch = {}
    for counter, sub in (("FETCH_SIZE", "fetch"), ("WRITE_SIZE", "write")):
        rows = pmc_rows(os.path.join(SRC, sub, "p_counter_collection.csv"), counter)
        with open(os.path.join(DST, f"{tag}_pmc_{counter}.csv"), "w") as f:
            f.write("Dispatch_Id,Kernel_Name,Counter_Name,Counter_Value\n")
            for d, n, v in rows:
                f.write(f"{d},{n},{counter},{v:.6f}\n")
        pn = [v for d, n, v in rows if "k_pnet_fused" in n]
        per_launch[counter] = sum(pn) / len(pn)
    # pyramid kernels of one step (k_pyramid0 / k_pyramid_stream dispatches between two k_pnet_fused dispatches)
    pyr_hbm = 0.0
    for counter, sub, mul in (("FETCH_SIZE", "fetch", 2.0), ("WRITE_SIZE", "write", 1.0)):
        rows = pmc_rows(os.path.join(SRC, sub, "p_counter_collection.csv"), counter)
        pn = [d for d, n, v in rows if "k_pnet_fused" in n]
        if len(pn) >= 2:
            pyr_hbm += mul * 1024.0 * sum(v for d, n, v in rows if "k_pyramid" in n and pn[-2] < d < pn[-1])
    bench = json.loads(open(os.path.join(SRC, "bench.json")).read().strip().splitlines()[-1])
    hbm = (2.0 * per_launch["FETCH_SIZE"] + per_launch["WRITE_SIZE"]) * 1024.0
    traffic = {
        "kernel": "k_pnet_fused",
        "source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes), python bench.py --steps 2 --warmup 1 --full --no-cpu-baseline",
        "FETCH_SIZE_KB_per_launch": per_launch["FETCH_SIZE"],
        "WRITE_SIZE_KB_per_launch": per_launch["WRITE_SIZE"],
        "correction": "gfx950: FETCH_SIZE counts 128-B requests as 64 B for wide coalesced 16 B/lane reads (MI355X_MICROARCH.md, HBM) -> x2; WRITE_SIZE exact",
        "hbm_bytes_per_launch": hbm,
        "pyramid_read_bytes": 2057127936,   # 256 frames x 669,638 pyramid pixels (720p, 11 levels, 64-padded) x 12 B
        "note": "the pyramid (three floats per pixel) is read once; the 42x42 input tiles overlap by 1.72x and most of that halo is served by L2",
        "pyramid_kernels_hbm_bytes_per_step": pyr_hbm,
    }
    json.dump(traffic, open(os.path.join(DST, f"{tag}_pnet_traffic.json"), "w"), indent=1)
    print(json.dumps(bench)[:600])
    print(summ[-900:])
    print("traffic GB/launch", hbm / 1e9)


if __name__ == "__main__":
    main()
