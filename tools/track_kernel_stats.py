"""Kernel times of the face tracker (csrc/trl_tracks.hip) by the method of profiles/groups_kernel_stats.csv: rocprofv3 kernel
trace, one process per shape, 3 windows of warm-up and 5 measured.

    python tools/track_kernel_stats.py --all out_dir > profiles/track_kernel_stats.csv      # every shape, then the table
    rocprofv3 --kernel-trace -d out_dir/f_e -o t -f csv -- python3 tools/track_kernel_stats.py run FACES EMB     (what --all starts)
    python tools/track_kernel_stats.py --table out_dir

A shape is FACES people in every frame of a 256-frame window (1, 4, 16, 64), with embeddings (EMB = 1: each person a unit row plus
noise of 0.03 per element, so every face finds its track by similarity) or without (EMB = 0: the IoU alone).  The people stand on a
grid, each box jittered by a pixel, and come in another order in every frame.  FaceTracker(iou_min=0.1, sim_min=0.4, max_age=3);
the clip's first window creates the tracks, then 3 + 5 further windows of the same clip are updated and `k_track_update` is one
launch per window.  On the one-face shape with embeddings the same rows then go through Engine.drift_update, 3 + 5 windows as
well: `drift_sims_kernel` + `drift_scan_kernel` are the only existing code that does this job on any of these shapes.  A row of
the table is one kernel of one shape: the median, smallest and largest of the 5 measured windows, and the median per frame."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FACES, FRAMES, WARMUP, WARM = (1, 4, 16, 64), 256, 3, 5
KERNELS = ("k_track_update", "drift_sims_kernel", "drift_scan_kernel")


def window(gen, centres, faces):
    """One window: boxes (FRAMES * faces, 4), counts (FRAMES,), emb (FRAMES * faces, 512), the people in a new order per frame."""
    import torch
    order = torch.stack([torch.randperm(faces, generator=gen, device="cuda") for _ in range(FRAMES)])          # (FRAMES, faces)
    x, y = (order % 8) * 40.0, (order // 8) * 40.0
    jitter = torch.randint(0, 2, (FRAMES, faces, 2), generator=gen, device="cuda").float()
    boxes = torch.stack([x + jitter[..., 0], y + jitter[..., 1], x + jitter[..., 0] + 30, y + jitter[..., 1] + 30], dim=-1)
    emb = centres[order] + 0.03 * torch.randn((FRAMES, faces, 512), generator=gen, device="cuda")
    emb = torch.nn.functional.normalize(emb, dim=-1)
    return boxes.reshape(-1, 4), torch.full((FRAMES,), faces, dtype=torch.int32, device="cuda"), emb.reshape(-1, 512)


def run(faces, with_emb):
    import torch
    import truely_amd
    gen = torch.Generator(device="cuda").manual_seed(faces)
    centres = torch.nn.functional.normalize(torch.randn((faces, 512), generator=gen, device="cuda"), dim=1)
    trk = truely_amd.FaceTracker(iou_min=0.1, sim_min=0.4, max_age=3)
    windows = [window(gen, centres, faces) for _ in range(1 + WARMUP + WARM)]
    torch.cuda.synchronize()
    for boxes, counts, emb in windows:
        trk.update(boxes, counts, emb if with_emb else None)
    t = trk.tracks(FRAMES * len(windows) * 4, 30)
    info = {"faces": faces, "emb": int(with_emb), "tracks": int(len(t["id"])), "dropped": t["dropped"], "drift": 0}
    if faces == 1 and with_emb:
        eng = truely_amd.Engine(truely_amd.weights.synthetic_blob(0), device=0)
        state = eng.drift_state()
        valid = torch.ones((FRAMES,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _boxes, _counts, emb in windows[1:]:
            eng.drift_update(state, emb, valid, FRAMES * len(windows) * 4, 30, sync=False)
        torch.cuda.synchronize()
        info["drift"] = 1
    print(json.dumps(info))


def _trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    return sorted(rows)


def table(out):
    print("faces_per_frame,frames,embeddings,kernel,launches,median_us,min_us,max_us,median_us_per_frame,tracks,dropped")
    for faces in FACES:
        for with_emb in (1, 0):
            d = os.path.join(out, f"{faces}_{with_emb}")
            info = json.load(open(os.path.join(d, "info.json")))
            tr = _trace(d)
            for k in KERNELS:
                t = [(e - s) / 1e3 for s, e, name in tr if k in name]
                if not t:
                    continue
                assert len(t) == (1 if k == "k_track_update" else 0) + WARMUP + WARM, (faces, with_emb, k, len(t))
                t = t[-WARM:]
                med = statistics.median(t)
                print(f"{faces},{FRAMES},{with_emb},{k},{len(t)},{med:.1f},{min(t):.1f},{max(t):.1f},{med / FRAMES:.3f},{info['tracks']},{info['dropped']}")


def run_all(out):
    for faces in FACES:
        for with_emb in (1, 0):
            d = os.path.join(out, f"{faces}_{with_emb}")
            os.makedirs(d, exist_ok=True)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "-d", d, "-o", "t", "-f", "csv", "--", sys.executable, os.path.abspath(__file__),
                                "run", str(faces), str(with_emb)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"shape {faces} x {with_emb} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, file=sys.stderr, flush=True)
            open(os.path.join(d, "info.json"), "w").write(line)
    table(out)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(int(sys.argv[2]), bool(int(sys.argv[3])))
    elif len(sys.argv) == 3 and sys.argv[1] == "--all":
        run_all(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        sys.exit(__doc__)
