"""Row-band sweep of the streaming pyramid pass (k_pyramid_stream): its duration per forced band count.

    rocprofv3 --kernel-trace -d OUT -o s -f csv -- python3 tools/pyramid_band_sweep.py run [n H W] [bands ...]
    python3 tools/pyramid_band_sweep.py table OUT

`run` builds the pyramid of n random frames (default 256 x 720 x 1280) REPS times per band count, 0 (the pass's own policy) first,
through trl_debug_option("pyr_row_bands"); `table` reads the kernel trace and prints the average and the minimum per band count
(the first launch of each is dropped).  TRUELY_HIP_LIB selects another build of the library."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 6
DEFAULT_BANDS = [0, 1, 2, 3, 4, 5, 6, 8]


def run(argv):
    import torch
    import truely_amd
    from truely_amd.engine import Engine
    n, H, W = (int(v) for v in argv[:3]) if len(argv) >= 3 else (256, 720, 1280)
    bands = [int(v) for v in argv[3:]] or DEFAULT_BANDS
    eng = Engine(truely_amd.weights.synthetic_blob(0), device=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    forced = False
    for k in bands:
        if k or forced:                                      # (a policy-only run also works on a build without the option)
            eng.option("pyr_row_bands", k)
            forced = True
        for _ in range(REPS):
            eng.pyramid_batch(frames)
        torch.cuda.synchronize()
        plan = eng.pyramid_plan()
        print("bands", k, "plan", sorted({(p["kernel"], p["row_bands"]) for p in plan if p["kernel"].startswith("S")}), flush=True)
    eng.close()


def table(argv):
    f = glob.glob(os.path.join(argv[0], "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if "k_pyramid_stream" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    bands = [int(v) for v in argv[1:]] or DEFAULT_BANDS
    # pyramid_batch asks for the layout first (no launch), then builds: launches per call = streaming groups of the shape
    per = len(rows) // (len(bands) * REPS)
    assert per >= 1 and per * len(bands) * REPS == len(rows), (len(rows), per)
    print("row bands (0 = policy): k_pyramid_stream launches per call %d; us per call, average / minimum of %d" % (per, REPS - 1))
    for i, k in enumerate(bands):
        calls = []
        for c in range(1, REPS):
            rr = rows[(i * REPS + c) * per:(i * REPS + c + 1) * per]
            calls.append(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rr) / 1e3)
        print("%3d  %9.1f  %9.1f" % (k, sum(calls) / len(calls), min(calls)))


if __name__ == "__main__":
    {"run": run, "table": table}[sys.argv[1]](sys.argv[2:])
