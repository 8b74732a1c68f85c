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
         (80, 320, 160), (333, 96, 161), (161, 161, 161), (45, 400, 112), (250, 250, 161), (96, 97, 160), (500, 123, 112),
         # both sides of Image.resize's switch to the vertical pass first (h > 100 * w and S < h)
         (600, 5, 160), (560, 5, 160), (330, 3, 128), (1300, 5, 512), (500, 5, 160), (300, 5, 160), (170, 3, 64), (600, 20, 160),
         (5, 600, 160), (601, 6, 160), (600, 6, 160), (606, 5, 700),
         # ... with both axes shrinking (S < w), and S between the two sizes
         (1700, 16, 8), (1601, 16, 15), (1600, 16, 15), (1601, 16, 17), (16, 1700, 8), (701, 7, 3)]


def _crop(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("h,w,S", CASES)
def test_pil_rule_equals_pillow(h, w, S):
    a = _crop(h, w, h * 7 + w)
    ref = np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR))
    assert np.array_equal(R.resize_pil(a, S), ref)


def _order_grid():
    """(h, w, S) around Image.resize's switch: tall crops and their mirrors (wide), S on either side of the crop sizes"""
    pts = []
    for w in (1, 2, 3, 5):                                     # narrow: S >= h // 4 > w, the horizontal axis always stretches
        for ratio in (60, 99, 100, 101, 110, 250):
            for dh in (0, 1):
                h = w * ratio + dh
                pts += [(h, w, S) for S in sorted({max(h // 4, 1), h - 1, h, h + 1, 64, 2 * h}) if S <= 320]
    # both axes shrink (S < w), and S between the two sizes, on both sides of h = 100 * w
    pts += [(h, 16, S) for h in (1599, 1600, 1601, 1650, 1700) for S in (1, 8, 15, 17)]
    pts += [(h, 7, S) for h in (699, 700, 701, 770) for S in (1, 3, 6, 8)]
    return pts + [(w, h, S) for h, w, S in pts]


def test_pil_pass_order_predicate_on_a_grid():
    """Image.resize filters vertically first for some very elongated crops.  On a grid around h = 100 * w -- tall, mirrored (wide),
    both-down and both-up crops, S on either side of the crop sizes -- wherever the two orders give different bytes, Pillow equals
    the order that extract_ref.pil_vertical_first names.  The counts at the end only keep the grid from going vacuous: each kind
    of point must stay in it in numbers, among the points where the orders differ."""
    rng = np.random.default_rng(12)
    differ = vertical = down_v = down_h = 0
    for h, w, S in _order_grid():
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        H, V = R.resize_pil(a, S, "h"), R.resize_pil(a, S, "v")
        if np.array_equal(H, V):
            continue
        v = R.pil_vertical_first(h, w, S)
        differ, vertical = differ + 1, vertical + v
        if S < min(h, w):
            down_v, down_h = down_v + v, down_h + (not v)
        ref = np.asarray(Image.fromarray(a).resize((S, S), Image.BILINEAR))
        assert np.array_equal(V if v else H, ref), (h, w, S, v)
    assert differ >= 100 and vertical >= 30 and differ - vertical >= 30, (differ, vertical)
    assert down_v >= 8 and down_h >= 8, (down_v, down_h)


def test_paths_known_answers():
    assert R.paths(320, 320, 160, "cv2")["mode"] == "fast" and R.paths(320, 321, 160, "cv2")["mode"] == "area"
    assert R.paths(100, 321, 160, "cv2")["mode"] == "linear" and R.paths(0, 5, 160, "pil")["status"] == -1
    p = R.paths(5500, 80, 160, "pil")                                               # scale 34.375: 69 or 70 taps, T = 34
    assert (p["order"], p["T"], p["chunks"], p["slots"]) == ("h", 34, 3, 2) and p["taps_y"] in (69, 70) and p["taps_x"] == 2
    assert R.paths(5500, 40, 160, "pil")["order"] == "v" and R.paths(5500, 40, 160, "pil")["chunks"] is None
    assert (R.paths(9, 9, 1024, "pil")["slots"], R.paths(9, 9, 1024, "pil")["T"]) == (12, 5)
    assert R.paths(100, 100, 7, "torch")["taps_y"] == 16                            # bin 3: rows floor(300 / 7) = 42 .. ceil(400 / 7) = 58
    for n, S in [(37, 160), (300, 160), (2561, 1024), (5500, 160), (1, 7)]:         # the tap counts are those of the coefficients
        nz = int((R.pil_coeffs(n, S)[1] != 0).sum(1).max())                         # a tap at the filter's edge may weigh 0
        assert nz <= R._pil_taps(n, S) <= nz + 2


def test_table_reaches_every_path_and_edge():
    """extract_ref.TABLE (the cases of test_gpu_extract_table.py) reaches what each case says it is there for, by the path
    restatement, and together the cases reach every item of extract_ref.REQUIRED."""
    names = [c["name"] for c in R.TABLE]
    assert len(set(names)) == len(names)
    declared = set()
    for c in R.TABLE:
        got = R.reached(c)
        assert set(c["reach"]) <= got, (c["name"], sorted(set(c["reach"]) - got))
        declared |= set(c["reach"])
        n, H, W = c["dims"]
        assert n * H * W * 3 <= 4 << 20 and 1 <= c["S"] <= 1024 and 0 <= c["margin"] < c["S"]
    assert set(R.REQUIRED) <= declared, sorted(set(R.REQUIRED) - declared)
    # the Pillow cases stand on both sides of the pass-order switch
    orders = {R.paths(*hw, c["S"], "pil")["order"] for c in R.TABLE for st, hw in R.case_crops(c) if st == 1}
    assert orders == {"h", "v"}


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
