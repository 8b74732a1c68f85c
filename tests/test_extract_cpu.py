"""CPU checks of the face-extraction restatement (tests/extract_ref.py) and of the new C ABI's symbols: the Pillow rule equals
Image.resize, the torch rule equals F.interpolate(mode="area").byte(), the OpenCV INTER_AREA restatement keeps its known answers,
select_boxes' ties go to the last tied box, and include/truely_hip.h + libtruely_hip.so carry the extraction entry points."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import extract_ref as R
from truely_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("trl_mtcnn_detect_ordered", "trl_select_faces", "trl_extract_faces")

# (crop h, crop w, S): up- and downscaling, mixed axes, 1-pixel crops, S in {112, 160, 161}
CASES = [(37, 53, 160), (300, 211, 160), (160, 500, 160), (17, 17, 160), (1000, 999, 112), (161, 159, 160), (1, 1, 160),
         (1, 7, 161), (9, 1, 112), (320, 320, 160), (2, 3, 112), (480, 80, 161), (700, 1300, 112), (160, 160, 160), (224, 224, 112),
         (80, 320, 160), (333, 96, 161), (161, 161, 161), (45, 400, 112), (250, 250, 161), (96, 97, 160), (500, 123, 112)]


def _crop(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("h,w,S", CASES)
def test_pil_rule_equals_pillow(h, w, S):
    a = _crop(h, w, h * 7 + w)
    ref = np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR))
    assert np.array_equal(R.resize_pil(a, S), ref)


@pytest.mark.parametrize("h,w,S", CASES)
def test_torch_rule_equals_interpolate_area(h, w, S):
    a = _crop(h, w, h * 5 + w)
    ref = F.interpolate(torch.from_numpy(a).permute(2, 0, 1)[None].float(), size=(S, S), mode="area").byte()[0].permute(1, 2, 0).numpy()
    assert np.array_equal(R.resize_torch(a, S), ref)


def test_cv2_area_known_answers():
    a = _crop(160, 160, 1)
    assert np.array_equal(R.resize_cv2(a, 160), a)                                  # scale 1: identity
    for (h, w) in [(37, 53), (320, 320), (300, 211), (80, 320), (161, 1)]:
        c = np.full((h, w, 3), 77, np.uint8)
        c[..., 1] = 200
        out = R.resize_cv2(c, 160)                                                  # a constant image stays constant
        assert (out[..., 0] == 77).all() and (out[..., 1] == 200).all(), (h, w)
    b = _crop(320, 320, 2).astype(np.int64)                                         # 2x2 blocks: (a+b+c+d+2) >> 2
    s = b[0::2, 0::2] + b[1::2, 0::2] + b[0::2, 1::2] + b[1::2, 1::2]
    assert np.array_equal(R.resize_cv2(b.astype(np.uint8), 160), (s + 2) >> 2)
    assert ((s & 3) == 2).any()                                                     # ... where half-to-even rounding would differ


def test_cv2_area_is_a_mean_downscaling():
    a = _crop(300, 211, 3)
    out = R.resize_cv2(a, 160).astype(np.float64)
    assert abs(out.mean() - a.mean()) < 1.0


def test_selection_ties_go_to_the_last_tied_box():
    b = np.array([[0, 0, 10, 10], [20, 20, 30, 30], [5, 5, 12, 12], [40, 40, 50, 50]], np.float32)   # rows 0, 1, 3: equal areas
    p = np.array([0.95, 0.99, 0.99, 0.91], np.float32)
    assert R.select(b, p, "largest", 64, 64) == 3
    assert R.select(b, p, "probability", 64, 64) == 2
    assert R.select(b, p, "largest_over_threshold", 64, 64) == 3
    assert R.select(b, np.array([0.95, 0.99, 0.99, 0.5], np.float32), "largest_over_threshold", 64, 64) == 1
    assert R.select(b, np.full(4, 0.9, np.float32), "largest_over_threshold", 64, 64) is None    # prob > 0.9 in f32: none pass
    # centre weighted: boxes 0 and 3 are mirror images about the frame centre (25, 25) -> equal keys, the later one wins
    assert R.select(b[[0, 3]], p[[0, 3]], "center_weighted_size", 50, 50) == 1
    for m in R.METHODS:                                                             # same as a reversed stable argsort
        key = {"largest": (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), "probability": p}.get(m)
        if key is not None:
            assert R.select(b, p, m, 64, 64) == int(np.argsort(key, kind="stable")[::-1][0])


def test_crop_box_margin_arithmetic():
    assert R.crop_box([10.7, 20.2, 50.9, 80.5], 160, 0, 100, 100) == (10, 20, 50, 80)
    # margin 20 of 160: mx = 20 * 40.2 / 140 in f64 (the f32 width), my = 20 * 60.3 / 140
    x1, y1, x2, y2 = (float(np.float32(v)) for v in (10.7, 20.2, 50.9, 80.5))
    mx, my = 20 * float(np.float32(x2 - x1)) / 140, 20 * float(np.float32(y2 - y1)) / 140
    assert R.crop_box([10.7, 20.2, 50.9, 80.5], 160, 20, 100, 100) == (int(x1 - mx / 2), int(y1 - my / 2), int(x2 + mx / 2), int(y2 + my / 2))
    assert R.crop_box([-5, -3, 120, 90], 160, 44, 100, 80) == (0, 0, 100, 80)          # clamped to the frame
    with pytest.raises(ValueError):
        R.extract(np.zeros((10, 10, 3), np.uint8), [12, 2, 15, 8], 160, 0)         # empty crop


def test_header_declares_and_library_exports_extraction():
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    declared = set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared, set(NEW) - declared
    assert set(NEW) <= set(_lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r"\bT (trl_[a-z0-9_]+)", out))
    assert set(NEW) <= exported, set(NEW) - exported
    src = open(os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc", "Makefile")).read()
    assert "trl_extract.hip" in src
