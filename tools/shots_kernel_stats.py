"""Kernel times of shot boundaries (csrc/trl_shots.hip) by the method of profiles/quality_kernel_stats.csv: rocprofv3 kernel trace
with its stats, no counters in the run, one process per shape, 2 calls of warm-up and 5 measured per content.

    python tools/shots_kernel_stats.py --all out_dir > profiles/shots_kernel_stats.csv      # every shape, then the table
    python tools/shots_kernel_stats.py --table out_dir
  what --all starts, one after the other, each under its own time limit, the next only if the last one ended well:
    timeout -k 10 420 rocprofv3 --kernel-trace --stats -d out_dir/720p -o t -f csv -- python3 tools/shots_kernel_stats.py run 720p &&
    timeout -k 10 420 rocprofv3 --kernel-trace --stats -d out_dir/4k -o t -f csv -- python3 tools/shots_kernel_stats.py run 4k

Shapes: "720p" -- 256 frames of 1280 x 720 (708 MB); "4k" -- 64 frames of 3840 x 2160 (1.59 GB).  Content per shape: "noise"
(uniform bytes), "constant" (every byte 128: each channel in ONE bin, the worst case for same-address LDS atomics) and "synthetic"
(synthetic.py's bench frames, repeated to the batch size).  Per content and call: trl_frame_signatures (k_shots_hist, k_shots_sum)
and a torch.clone of the batch.  The clone reads and writes every byte once, so HALF its time is the read floor the table quotes;
it is timed with events in the same process (a device-to-device copy is no kernel, so the kernel trace does not show it).  After
the contents: trl_signature_distance on 256 pairs and trl_shots_update on a window of 256 frames (k_shots_dist,
k_shots_window_dist, k_shots_scan).  A row of the table is one kernel of one shape and content: the median, smallest and largest of
the 5 measured launches, the floor, and the median over the floor.  Timings are reported, not gated."""
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
SHAPES = {"720p": (256, 720, 1280), "4k": (64, 2160, 3840)}
CONTENTS = ("noise", "constant", "synthetic")
WARMUP, WARM, LIMIT_S = 2, 5, 420
FRAME_KERNELS = ("k_shots_hist", "k_shots_sum")
CLIP_KERNELS = ("k_shots_dist", "k_shots_window_dist", "k_shots_scan")


def _batch(content, n, H, W, device):
    import torch
    import truely_amd
    if content == "noise":
        return torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=device)
    if content == "constant":
        return torch.full((n, H, W, 3), 128, dtype=torch.uint8, device=device)
    base = torch.from_numpy(truely_amd.synthetic.synthetic_frames(8, H, W, seed=0)).to(device)
    return base.repeat(n // 8, 1, 1, 1)


def run(shape):
    import torch
    import truely_amd
    n, H, W = SHAPES[shape]
    device = torch.device("cuda", 0)
    info = {"shape": shape, "frames": n, "H": H, "W": W, "bytes": n * H * W * 3}
    sig = None
    for content in CONTENTS:
        frames = _batch(content, n, H, W, device)
        torch.cuda.synchronize()
        clone_ms, call_ms = [], []
        for _ in range(WARMUP + WARM):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            sig = truely_amd.frame_signatures(frames)
            e[1].record()
            copy = frames.clone()
            e[2].record()
            torch.cuda.synchronize()
            call_ms.append(e[0].elapsed_time(e[1]))
            clone_ms.append(e[1].elapsed_time(e[2]))
            del copy
        info[content] = {"clone_us": [1e3 * v for v in clone_ms[-WARM:]], "call_us": [1e3 * v for v in call_ms[-WARM:]],
                         "sum_ok": bool((sig.sum(-1)[:, 0, 0] == (H // 4) * (W // 4)).all())}
        del frames
    sig = sig[:256] if sig.shape[0] >= 256 else sig.repeat(256 // sig.shape[0], 1, 1, 1)
    det = truely_amd.ShotDetector(device=device)
    state = det._state
    from truely_amd import _lib
    from truely_amd._tensors import ptr, stream
    lib = _lib.load()
    dist = torch.empty((256,), dtype=torch.float32, device=device)
    cut = torch.empty((256,), dtype=torch.uint8, device=device)
    shot = torch.empty((256,), dtype=torch.int32, device=device)
    for _ in range(WARMUP + WARM):
        truely_amd.signature_distance(sig, sig.roll(1, 0), H, W)
        _lib.check(lib.trl_shots_update(ptr(state), ptr(sig), 256, H, W, None, ptr(dist), ptr(cut), ptr(shot), stream(device)))
    torch.cuda.synchronize()
    info["cuts"] = int(cut.sum())
    print(json.dumps(info))


def _trace(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    return sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))


def _times(tr, kernel):
    return [(e - s) / 1e3 for s, e, name in tr if re.search(kernel + r"(?![_a-z0-9])", name)]


def table(out):
    print("shape,frames,MB,content,kernel,launches,median_us,min_us,max_us,clone_median_us,read_floor_us,median_over_floor")
    for shape in SHAPES:
        d = os.path.join(out, shape)
        info = json.load(open(os.path.join(d, "info.json")))
        tr = _trace(d)
        head = f"{shape},{info['frames']},{info['bytes'] / 1e6:.0f}"
        for k in FRAME_KERNELS:
            t = _times(tr, k)
            assert len(t) == len(CONTENTS) * (WARMUP + WARM), (shape, k, len(t))
            for i, content in enumerate(CONTENTS):
                part = t[i * (WARMUP + WARM):(i + 1) * (WARMUP + WARM)][-WARM:]
                clone = statistics.median(info[content]["clone_us"])
                med = statistics.median(part)
                print(f"{head},{content},{k},{len(part)},{med:.1f},{min(part):.1f},{max(part):.1f},{clone:.1f},{clone / 2:.1f},{med / (clone / 2):.2f}")
        for content in CONTENTS:
            c, clone = info[content]["call_us"], statistics.median(info[content]["clone_us"])
            print(f"{head},{content},trl_frame_signatures (events),{len(c)},{statistics.median(c):.1f},{min(c):.1f},{max(c):.1f},{clone:.1f},"
                  f"{clone / 2:.1f},{statistics.median(c) / (clone / 2):.2f}")
        for k in CLIP_KERNELS:
            t = _times(tr, k)[-WARM:]
            assert len(t) == WARM, (shape, k, len(t))
            print(f"{head},256 signatures,{k},{len(t)},{statistics.median(t):.1f},{min(t):.1f},{max(t):.1f},,,")


def run_all(out):
    for shape in SHAPES:                                        # one after the other; the first failure ends the run
        d = os.path.join(out, shape)
        os.makedirs(d, exist_ok=True)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "-f", "csv", "--",
                            sys.executable, os.path.abspath(__file__), "run", shape], capture_output=True, text=True)
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
