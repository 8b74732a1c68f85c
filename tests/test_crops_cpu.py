"""The face-crop references (tests/crop_ref.py) against the C oracle on the whole case table, without a GPU.

The oracle's crop code restates OpenCV and facenet-pytorch from memory; crop_ref.py restates the same operations from their
definitions in plain numpy, and a float64 form of each says what both approximate.  Where two independent restatements agree
bit for bit on every rectangle of the table -- 1 px wide, exact 1x / 2x / 1/2x ratios, all four frame corners, 1-px frames,
4K -- and stay within a derived distance of exact arithmetic, a clamp that is off by one or a swapped pair of rows has nowhere
to hide.  tests/test_gpu_crops.py runs the kernels on the same table.
"""
import numpy as np
import pytest

import crop_ref as R


def _cases(H, W, contents=R.CONTENTS):
    """(content, frame, rect) over the table of an H x W frame; one frame per content."""
    for ci, kind in enumerate(contents):
        img = R.content_frames(kind, 1, H, W, seed=1000 * ci + H + W)[0]
        for r in R.rect_table(H, W):
            yield kind, img, r


def test_table_holds_the_geometries_it_names():
    for H, W in R.GEOMETRIES:
        t = R.rect_table(H, W)
        assert (0, 0, W, H) in t and (0, 0, 1, 1) in t and (W - 1, H - 1, W, H) in t and len(set(t)) == len(t)
        assert all(0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H for x0, y0, x1, y1 in t)
        for s in R.SIDES:
            if s <= min(H, W):
                got = [r for r in t if r[2] - r[0] == s and r[3] - r[1] == s]
                assert (0, 0, s, s) in got and (W - s, H - s, W, H) in got and (W - s, 0, W, s) in got and (0, H - s, s, H) in got
    t = R.rect_table(2160, 3840)
    assert {(r[2] - r[0], r[3] - r[1]) for r in t} >= {(1, 2160), (3840, 1), (2, 161), (161, 2), (240, 240), (3840, 2160)}
    assert any(0 < r[0] and r[2] < 3840 and 0 < r[1] and r[3] < 2160 for r in t)      # interior placements exist


@pytest.mark.parametrize("H,W", R.GEOMETRIES)
def test_resize_restatements_agree(oracle, H, W):
    """oracle.resize_linear_u8 == crop_ref.resize_linear_u8_int, bit for bit, on every rectangle and content of the table."""
    k = 0
    for kind, img, (x0, y0, x1, y1) in _cases(H, W):
        assert np.array_equal(oracle.resize_linear_u8(img, y0, y1, x0, x1), R.resize_linear_u8_int(img, y0, y1, x0, x1)), (kind, x0, y0, x1, y1)
        k += 1
    assert k == 4 * len(R.rect_table(H, W))


@pytest.mark.parametrize("H,W", R.GEOMETRIES)
def test_area_restatements_agree(oracle, H, W):
    """oracle.crop_area_std == crop_ref.crop_area_std (exact integer floor of the bin mean), bit for bit, rgb off and on, S = 160
    on the whole table and S = 1, 7, 80 on its random frames -- there only on rectangles whose bins are small enough for the
    floor to stand for the f32 expression (crop_ref.area_floor_is_exact; S = 160 satisfies it on every rectangle of the table)."""
    seen = set()
    for kind, img, r in _cases(H, W):
        assert R.area_floor_is_exact(r[3] - r[1], r[2] - r[0], 160)
        for S in (160,) if kind != "random" else (160, 1, 7, 80):
            if not R.area_floor_is_exact(r[3] - r[1], r[2] - r[0], S):
                continue
            seen.add(S)
            for rgb in (False, True):
                assert np.array_equal(oracle.crop_area_std(img, r, S=S, rgb=rgb), R.crop_area_std(img, *r, S=S, rgb=rgb)), (kind, r, S, rgb)
    assert seen == {160, 1, 7, 80}


def test_fixed_point_stays_within_its_derived_bound(capsys):
    """|resize_linear_u8_int - resize_linear_f64| <= crop_ref.resize_fixed_point_bound() = 1.381 grey levels on every output of
    the table.  The derivation (weights: 2^-12 rounding + 2^-13 f32 centre + 2^-25; horizontal 2 * 255 * e = 0.187; >> 4: 1/128;
    vertical 0.187; two >> 16: 0.5; final rounding: 0.5) is in that function's docstring.  Measured maximum over the table:
    0.8013 grey levels (random content, the 79 x 79 rectangle at the top-right corner of the 180 x 320 frame)."""
    bound = R.resize_fixed_point_bound()
    assert 1.0 < bound < 1.5
    worst, where = 0.0, None
    for H, W in R.GEOMETRIES:
        for kind, img, (x0, y0, x1, y1) in _cases(H, W, ("random", "checker")):
            assert max(x1 - x0, y1 - y0) <= 4096
            d = np.abs(R.resize_linear_u8_int(img, y0, y1, x0, x1).astype(np.float64) - R.resize_linear_f64(img, y0, y1, x0, x1)).max()
            if d > worst:
                worst, where = float(d), (H, W, kind, x0, y0, x1, y1)
    with capsys.disabled():
        print(f"\n  max |fixed point - exact bilinear| = {worst:.4f} grey levels at {where}; derived bound {bound:.4f}")
    assert worst <= bound, (worst, where)


ALIGN_GEOMETRIES = R.GEOMETRIES + ((300, 420),)


def test_aligned_oracle_is_the_f64_warp_within_f32_rounding(oracle, capsys):
    """|oracle.crop_aligned - crop_ref.crop_aligned_f64| <= crop_ref.aligned_f32_bound() = (13 * 255 + 128) / 128 * 2^-24 * 1.01
    = 1.62e-6 (three f32 lerps on values of at most 255, the subtraction of 127.5, an exact division by 128: derived in that
    function's docstring) for every landmark set, frame geometry and S in {160, 112, 1}; a NaN coordinate gives NaN in every
    output of both.  Measured maximum: 2.99e-7 (the template set on the 97 x 131 frame, S = 160)."""
    bound = R.aligned_f32_bound()
    assert 1.5e-6 < bound < 1.7e-6
    worst, where = 0.0, None
    for H, W in ALIGN_GEOMETRIES:
        img = R.content_frames("random", 1, H, W, seed=H * 7 + W)[0]
        for name, pts in R.landmark_sets(H, W):
            for S in (160, 112, 1):
                for rgb in (True, False):
                    got, ref = oracle.crop_aligned(img, pts, S=S, rgb=rgb), R.crop_aligned_f64(img, pts, S=S, rgb=rgb)
                    assert got.shape == ref.shape == (S, S, 3)
                    if name == "nan":
                        assert np.isnan(got).all() and np.isnan(ref).all()
                        continue
                    d = float(np.abs(got.astype(np.float64) - ref).max())
                    if d > worst:
                        worst, where = d, (H, W, name, S, rgb)
    with capsys.disabled():
        print(f"\n  max |f32 aligned crop - f64 warp| = {worst:.3e} at {where}; derived bound {bound:.3e}")
    assert worst <= bound, (worst, where)


def test_align_params_agree(oracle):
    """The six similarity parameters: crop_ref's f64 restatement == the oracle's, bit for bit (same operation order)."""
    for H, W in ALIGN_GEOMETRIES:
        for name, pts in R.landmark_sets(H, W):
            assert np.array_equal(np.array(R.align_params(pts), np.float64), oracle.align_params(pts), equal_nan=True), (H, W, name)


@pytest.mark.parametrize("H,W", R.GEOMETRIES)
def test_exact_ratios_and_flat_frames(oracle, H, W):
    """Where the definition gives the answer outright: an 80 x 80 rectangle is copied, a 160 x 160 one becomes the rounded mean of
    its 2 x 2 blocks (both centres fall on weights 2048 / 0 and 1024 / 1024), an all-0 frame stays 0 and an all-255 frame 255 at
    every rectangle (weight pairs that do not sum to 2048 would show here); area pooling copies a 160 x 160 rectangle and
    duplicates the pixels of an 80 x 80 one."""
    n80 = n160 = 0
    for kind, img, (x0, y0, x1, y1) in _cases(H, W):
        for f in (oracle.resize_linear_u8, R.resize_linear_u8_int):
            out = f(img, y0, y1, x0, x1)
            if kind == "zeros":
                assert not out.any(), (x0, y0, x1, y1)
            elif kind == "ones":
                assert (out == 255).all(), (x0, y0, x1, y1)
            elif (x1 - x0, y1 - y0) == (80, 80):
                assert np.array_equal(out, img[y0:y1, x0:x1])
                n80 += 1
            elif (x1 - x0, y1 - y0) == (160, 160):
                blk = img[y0:y1, x0:x1].astype(np.int32).reshape(80, 2, 80, 2, 3).sum((1, 3))
                assert np.array_equal(out, ((blk + 2) >> 2).astype(np.uint8))
                n160 += 1
        if kind in ("zeros", "ones"):
            v = np.float32((0 if kind == "zeros" else 255) - 127.5) / np.float32(128)
            assert (oracle.crop_area_std(img, (x0, y0, x1, y1)) == v).all() and (R.crop_area_std(img, x0, y0, x1, y1) == v).all()
        elif (x1 - x0, y1 - y0) == (160, 160):
            assert np.array_equal(R.crop_area_u8(img, x0, y0, x1, y1), img[y0:y1, x0:x1])
        elif (x1 - x0, y1 - y0) == (80, 80):
            assert np.array_equal(R.crop_area_u8(img, x0, y0, x1, y1), img[y0:y1, x0:x1].repeat(2, 0).repeat(2, 1))
    if min(H, W) >= 160:
        assert n80 >= 2 * 2 * 5 and n160 >= 2 * 2 * 5       # two contents x two implementations x five placements


def test_references_read_nothing_outside_the_rectangle():
    """The property the GPU test leans on: changing every pixel outside the rectangle changes no reference output."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)
    for x0, y0, x1, y1 in ((0, 0, 1, 1), (5, 7, 46, 50), (89, 59, 90, 60), (10, 0, 90, 3)):
        other = rng.integers(0, 256, img.shape, dtype=np.uint8)
        other[y0:y1, x0:x1] = img[y0:y1, x0:x1]
        assert np.array_equal(R.resize_linear_u8_int(img, y0, y1, x0, x1), R.resize_linear_u8_int(other, y0, y1, x0, x1))
        assert np.array_equal(R.resize_linear_f64(img, y0, y1, x0, x1), R.resize_linear_f64(other, y0, y1, x0, x1))
        assert np.array_equal(R.crop_area_u8(img, x0, y0, x1, y1, 160), R.crop_area_u8(other, x0, y0, x1, y1, 160))
