"""Kernel times of face quality (csrc/trl_quality.hip) by the method of profiles/pool_kernel_stats.csv: rocprofv3 kernel trace, one
process per shape, 2 calls of warm-up and 5 measured.

    python tools/quality_kernel_stats.py --all out_dir > profiles/quality_kernel_stats.csv      # every shape, then the table
    rocprofv3 --kernel-trace -d out_dir/SHAPE -o t -f csv -- python3 tools/quality_kernel_stats.py run SHAPE     (what --all starts)
    python tools/quality_kernel_stats.py --table out_dir

Shapes: "720p" -- 256 frames of 1280 x 720 (the bench clip's first 32 frames, eight times), the largest face of each as
extract_faces finds it, so the bench's typical boxes; "270p" -- the multi-face 270p clip sixteen times (32 frames), every face.
Per call: trl_face_quality with the O-Net points (k_quality_accum, k_quality_finish) and trl_extract_faces on the same rows
(k_extract: the other kernel that reads these rectangles, to 160 x 160).  A row of the table is one kernel of one shape: the
median, smallest and largest of the 5 measured launches; beside it the rectangles' bytes (3 N per face) and the time HBM needs to
read them once at the 6.29 TB/s a float4 copy reaches, and the median over that floor.  Timings are reported, not gated."""
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES, WARMUP, WARM = ("720p", "270p"), 2, 5
KERNELS = ("k_quality_accum", "k_quality_finish", "k_extract")
HBM_BYTES_PER_S = 6.29e12


def run(shape):
    import numpy as np
    import torch
    import truely_amd
    from truely_amd.engine import Engine
    eng = Engine(truely_amd.weights.synthetic_blob(0))
    if shape == "720p":
        base, reps, keep_all = truely_amd.synthetic.synthetic_frames(32, 720, 1280, seed=0), 8, False
    else:
        z = np.load(os.path.join(ROOT, "tests", "golden", "clip_multiface_270p.npz"))
        base = truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))
        reps, keep_all = 16, True
    d = eng.extract_faces(base, keep_all=keep_all, quality=True)
    k, m1 = base.shape[0], d["box"].shape[0]
    frames = torch.from_numpy(base).to(eng.device).repeat(reps, 1, 1, 1)
    step = torch.arange(reps, device=eng.device, dtype=torch.int32).repeat_interleave(m1) * k
    frame_of = torch.where(d["frame"].repeat(reps) >= 0, d["frame"].repeat(reps) + step, -1).int()
    box, pts = d["box"].repeat(reps, 1), d["points"].repeat(reps, 1)
    torch.cuda.synchronize()
    for _ in range(WARMUP + WARM):
        q = eng.face_quality(frames, frame_of, box, pts)
        eng.extract_boxes(frames, frame_of, box)
    torch.cuda.synchronize()
    raw = q["raw"].cpu().numpy()
    live = raw[:, 0] > 0
    print(json.dumps({"shape": shape, "frames": int(frames.shape[0]), "rows": int(len(raw)), "faces": int(live.sum()),
                      "rect_bytes": int(3 * raw[:, 0].sum()), "median_w": float(np.median(raw[live, 7])),
                      "median_h": float(np.median(raw[live, 0] / raw[live, 7])), "mean_quality": float(q["quality"].mean())}))


def _trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    return sorted(rows)


def table(out):
    print("shape,frames,rows,faces,median_w,median_h,rect_MB,kernel,launches,median_us,min_us,max_us,hbm_read_floor_us,median_over_floor")
    for shape in SHAPES:
        d = os.path.join(out, shape)
        info = json.load(open(os.path.join(d, "info.json")))
        tr = _trace(d)
        floor = info["rect_bytes"] / HBM_BYTES_PER_S * 1e6
        for k in KERNELS:
            t = [(e - s) / 1e3 for s, e, name in tr if re.search(k + r"(?![_a-z0-9])", name)][-WARM:]
            assert len(t) == WARM, (shape, k, len(t))
            med = statistics.median(t)
            print(f"{shape},{info['frames']},{info['rows']},{info['faces']},{info['median_w']:.0f},{info['median_h']:.0f},"
                  f"{info['rect_bytes'] / 1e6:.2f},{k},{len(t)},{med:.1f},{min(t):.1f},{max(t):.1f},{floor:.2f},{med / floor:.1f}")


def run_all(out):
    for shape in SHAPES:
        d = os.path.join(out, shape)
        os.makedirs(d, exist_ok=True)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "run", shape], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(f"{shape} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, file=sys.stderr, flush=True)
        open(os.path.join(d, "info.json"), "w").write(line)
    table(out)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--all":
        run_all(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        sys.exit(__doc__)
