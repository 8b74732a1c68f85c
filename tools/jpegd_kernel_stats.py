"""Per-kernel times of the Motion-JPEG decoder: ten DeviceJpegDecoder.decode calls of a 32-frame batch (the wall-time tool's
synthetic frames, Pillow quality 80, 4:2:0, no restart markers), to be run under the profiler, one process per size:

    rocprofv3 --kernel-trace --stats -d out -o s -f csv -- python3 tools/jpegd_kernel_stats.py 360p      (and 720p)
    python tools/jpegd_kernel_stats.py --table out_360p out_720p > profiles/mjpegd_kernel_stats.csv

The first form prints the batch's mean file size and Huffman symbols per frame (counted by tests/jpegd_ref.py's entropy
decoder on three of the frames, on the host); the second turns the two runs' kernel_stats.csv into the committed table."""
import csv
import glob
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = {"360p": (360, 640), "720p": (720, 1280)}


def batch_files(shape):
    import truely_amd
    from PIL import Image
    H, W = SHAPES[shape]
    files = []
    for f in truely_amd.synthetic.synthetic_frames(32, H, W, seed=21):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(b, "JPEG", quality=80, subsampling=2)
        files.append(b.getvalue())
    return files


def symbols(data):
    """Huffman symbols in the file's scan: table lookups of the reference entropy decoder."""
    import jpegd_ref

    class Counted:
        n = 0

        def __init__(self, a):
            self.a = a

        def __getitem__(self, i):
            Counted.n += 1
            return self.a[i]
    info = jpegd_ref.parse(data)
    info["dc"] = [Counted(a) for a in info["dc"]]
    info["ac"] = [Counted(a) for a in info["ac"]]
    jpegd_ref.entropy_decode(data, info)
    return Counted.n


def run(shape):
    import torch
    from truely_amd import jpeg
    H, W = SHAPES[shape]
    files = batch_files(shape)
    dec = jpeg.DeviceJpegDecoder(W, H, max_frames=32)
    for _ in range(10):
        frames, status = dec.decode(files)
    torch.cuda.synchronize()
    assert (status == 0).all()
    print(json.dumps({"shape": shape, "bytes_per_frame": int(np.mean([len(f) for f in files])),
                      "symbols_per_frame": int(np.mean([symbols(f) for f in files[:3]]))}))


def table(dirs):
    print("shape,kernel,calls,avg_us,us_per_frame(32-frame batch),note")
    for shape, d in zip(("360p", "720p"), dirs):
        sym = int(np.mean([symbols(f) for f in batch_files(shape)[:3]]))
        f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
        for r in csv.DictReader(open(f)):
            name, us = r["Name"], float(r["AverageNs"]) / 1e3
            if "k_jpegd" in name:
                k = name.split("::")[1].split("(")[0]
                note = ""
                if k == "k_jpegd_huff":
                    note = (f"1 lane per wave kept (64 not measured); one segment per frame; {sym} Huffman symbols per segment = "
                            f"{sym / us:.2f} M symbols/s per segment")
                print(f"{shape},{k},{r['Calls']},{us:.2f},{us / 32:.3f},{note}")
            elif "fillBufferAligned" in name:
                print(f"{shape},coefficient memset (__amd_rocclr_fillBufferAligned),{r['Calls']},{us:.2f},{us / 32:.3f},")


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        table(sys.argv[2:4])
    else:
        run(sys.argv[1])
