"""Per-kernel times of the Motion-JPEG encoder and of the decoder on the encoder's own files, to be run under the profiler, one
process per measurement:

    rocprofv3 --kernel-trace --stats -d out/TAG -o s -f csv -- python3 tools/jpeg_kernel_stats.py 360p [--lib LIB]
              [--subsampling 0|1|2] [--restart-rows R] [--optimize] [--decode]
    python tools/jpeg_kernel_stats.py --table out > profiles/jpeg_options_kernel_stats.csv

The first form encodes a 32-frame batch (the wall-time tool's synthetic frames, quality 80) twenty times through the C ABI --
``trl_jpeg_create`` when no option is given, so that ``--lib`` can name another build of the library (the parent commit's), and
``trl_jpeg_create_ex`` otherwise -- and prints the mean file size.  ``--decode`` then decodes those files ten times with
``DeviceJpegDecoder`` (the method of tools/jpegd_kernel_stats.py, on this encoder's output instead of Pillow's).  The second form
turns every TAG's kernel_stats.csv under ``out`` into one table: a row per TAG and kernel, microseconds per batch and per frame."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"360p": (360, 640), "720p": (720, 1280)}
BATCH, CALLS = 32, 20


def run(a):
    import torch
    import truely_amd
    from truely_amd import _lib
    H, W = SHAPES[a.shape]
    frames = truely_amd.synthetic.synthetic_frames(BATCH, H, W, seed=21)
    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    lib = C.CDLL(a.lib or _lib.LIB_PATH)
    lib.trl_last_error.restype = C.c_char_p
    h = C.c_void_p()
    plain = a.subsampling == 2 and not a.restart_rows and not a.optimize
    if plain:
        st = lib.trl_jpeg_create(0, H, W, 80, BATCH, C.byref(h))
    else:
        opt = (C.c_int * 5)(80, a.subsampling, a.restart_rows, 0, int(a.optimize))
        st = lib.trl_jpeg_create_ex(0, H, W, opt, BATCH, C.byref(h))
    assert st == 0, lib.trl_last_error()
    cap = BATCH * H * W * 3
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    sizes = np.zeros(BATCH, np.int64)
    for _ in range(CALLS):
        st = lib.trl_jpeg_encode(h, C.c_void_p(d.data_ptr()), BATCH, C.c_longlong(H * W * 3), C.c_void_p(out.data_ptr()),
                                 C.c_longlong(cap), sizes.ctypes.data_as(C.c_void_p), None)
        assert st == 0 and sizes.sum() <= cap, lib.trl_last_error()
    torch.cuda.synchronize()
    lib.trl_jpeg_destroy(h)
    res = {"shape": a.shape, "subsampling": a.subsampling, "restart_rows": a.restart_rows, "optimize": bool(a.optimize),
           "lib": os.path.basename(os.path.dirname(a.lib)) if a.lib else "this", "bytes_per_frame": int(sizes.mean())}
    if a.decode:
        from truely_amd import jpeg
        data = out.cpu().numpy()
        ends = np.cumsum(sizes)
        files = [data[e - s:e].tobytes() for s, e in zip(sizes, ends)]
        dec = jpeg.DeviceJpegDecoder(W, H, max_frames=BATCH)
        for _ in range(10):
            got, status = dec.decode(files)
        torch.cuda.synchronize()
        assert (status == 0).all()
        res["decoded"] = True
    print(json.dumps(res))


def table(root):
    """us_per_batch is the kernel's total time over the process's batches (a batch above the workspace budget runs in chunks, so
    a kernel can run more than once per batch)."""
    print("tag,kernel,calls,us_per_batch,us_per_frame(32-frame batch)")
    for d in sorted(glob.glob(os.path.join(root, "*"))):
        fs = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not fs:
            continue
        tag, enc, dec = os.path.basename(d), 0.0, 0.0
        for r in csv.DictReader(open(fs[0])):
            name = r["Name"]
            if "k_jpeg" not in name:
                continue
            us = float(r["TotalDurationNs"]) / 1e3 / (10 if "k_jpegd" in name else CALLS)
            k = re.search(r"k_jpegd?_\w+(<\w+>)?", name).group(0)
            print(f"{tag},{k},{r['Calls']},{us:.2f},{us / BATCH:.3f}")
            if "k_jpegd" in name:
                dec += us
            else:
                enc += us
        print(f"{tag},all encoder kernels,,{enc:.2f},{enc / BATCH:.3f}")
        if dec:
            print(f"{tag},all decoder kernels,,{dec:.2f},{dec / BATCH:.3f}")


if __name__ == "__main__":
    if sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        p = argparse.ArgumentParser()
        p.add_argument("shape", choices=sorted(SHAPES))
        p.add_argument("--lib")
        p.add_argument("--subsampling", type=int, default=2)
        p.add_argument("--restart-rows", type=int, default=0)
        p.add_argument("--optimize", action="store_true")
        p.add_argument("--decode", action="store_true")
        run(p.parse_args())
