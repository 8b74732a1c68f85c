"""OPTIONAL -- dumps REAL facenet-pytorch face-extraction goldens.  Not runnable in the build container (no facenet-pytorch, no
OpenCV), never shipped as a dependency.

tests/extract_ref.py restates MTCNN.forward's extraction from the feature issue; its Pillow and torch rules are checked against
Pillow and torch, but its OpenCV INTER_AREA rule (numpy input) is recalled and UNPINNED.  Run this on any machine that has

    facenet-pytorch==2.6.0  opencv-python  Pillow  numpy<2

and it writes, for each seeded synthetic clip, `extract_<clip>.npz`: the frames' generator parameters, the library's
`detect(frame)` boxes / probs in its own order (select_largest=False) and `mtcnn(img)` outputs for every input kind (numpy,
tensor, PIL), keep_all, image_size and margin below.  Comparing `extract_ref.extract(frame, box, ...)` with the recorded faces
pins the resamplers independently of the detector weights.

    python tests/golden/dump_extract_goldens.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CASES = [("clip_multiface_270p", 2, 270, 480, 33, -1), ("clip_360p", 3, 360, 640, 11, 1), ("clip_odd", 3, 97, 131, 21, 1)]
SETTINGS = [(160, 0), (160, 20), (112, 44), (161, 10)]   # (image_size, margin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    args = ap.parse_args()
    import torch
    from PIL import Image
    from facenet_pytorch import MTCNN
    import truely_amd
    kinds = {"numpy": lambda a: a, "tensor": torch.from_numpy, "pil": Image.fromarray}
    for name, n, H, W, seed, faces in CASES:
        fr = truely_amd.synthetic.synthetic_frames(n, H, W, seed=seed, faces=faces)
        rec = {"n": n, "H": H, "W": W, "seed": seed, "faces_per_frame": faces, "frames_crc": int(fr.astype(np.uint64).sum())}
        det = MTCNN(select_largest=False, keep_all=True)
        for i in range(n):
            b, p = det.detect(fr[i])
            rec[f"f{i}_boxes"] = np.zeros((0, 4), np.float32) if b is None else np.asarray(b, np.float32)
            rec[f"f{i}_probs"] = np.zeros((0,), np.float32) if b is None else np.asarray(p, np.float32)
        for S, margin in SETTINGS:
            m = MTCNN(image_size=S, margin=margin, select_largest=False, keep_all=True, post_process=False)
            for kind, conv in kinds.items():
                for i in range(n):
                    out = m(conv(fr[i]))
                    rec[f"f{i}_{kind}_S{S}_m{margin}"] = (np.zeros((0, 3, S, S), np.float32) if out is None
                                                          else out.cpu().numpy().astype(np.float32))
        rec["source"] = "facenet-pytorch 2.6.0"
        np.savez_compressed(os.path.join(args.out, f"extract_{name}.npz"), **rec)
        print("wrote", name)


if __name__ == "__main__":
    main()
