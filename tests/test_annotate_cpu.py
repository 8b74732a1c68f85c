"""The rules of the drawing kernel, pinned on the CPU: tests/annotate_ref.py -- a scalar float32 restatement of
csrc/trl_annotate.hip, driven by annotate.draw_list / annotate.DrawList -- equals annotate.py's own array code (annotate,
rectangle, put_text) byte for byte, on every pixel of every frame."""
import numpy as np
import pytest

import annotate_ref as R
from truely_amd import annotate as A


@pytest.fixture(autouse=True)
def own_rasteriser(monkeypatch):
    monkeypatch.setattr(A, "cv2", None)                     # the kernel follows this module's rasteriser, not OpenCV's


def check_notes(bg, notes, hypot=R.hypot_double):
    want, got = bg.copy(), bg.copy()
    R.host_annotate(want, notes)
    R.draw(got, *A.draw_list(notes), hypot=hypot)
    return want, got


def test_empty_note_set_gives_empty_lists():
    flist, segs = A.draw_list([])
    assert len(flist) == 0 and len(segs) == 0
    assert flist.dtype == A.FRAME_DTYPE and segs.dtype == A.SEG_DTYPE
    assert A.FRAME_DTYPE.itemsize == 40 and A.SEG_DTYPE.itemsize == 24      # trl_draw_frame, trl_draw_seg


def test_segment_ranges_tile_the_list():
    notes = [(5, 88888, (3, 4, 50, 60), True), (0, 1, (3, 4, 50, 60), False), (9, 7, (0, 0, 1, 1), True), (2, 3, (1, 1, 5, 5), False)]
    flist, segs = A.draw_list(notes)
    assert flist["frame"].tolist() == [0, 2, 5, 9]
    assert flist["seg_begin"][0] == 0 and flist["seg_end"][-1] == len(segs)
    assert np.array_equal(flist["seg_begin"][1:], flist["seg_end"][:-1])
    per = [len(A.text_segments(t, (0, 0), 1)) for t in ("Real Frame", "Real Frame", "AI Detected - Frame 88888", "AI Detected - Frame 7")]
    assert (flist["seg_end"] - flist["seg_begin"]).tolist() == per and per[0] == 93 and per[2] == 293
    dl = A.DrawList()                                          # a rectangle alone, a text alone, an unknown character (a space), no text
    dl.rectangle(1, (0, 0), (3, 3), (1, 2, 3), 3)
    dl.put_text(4, "A?", (0, 9), 1, (4, 5, 6), 1)
    dl.put_text(6, "", (0, 9), 1, (4, 5, 6), 1)
    flist, segs = dl.arrays()
    assert flist["thickness"].tolist() == [3, 0, 0] and flist["seg_begin"].tolist() == [0, 0, 3] and flist["seg_end"].tolist() == [0, 3, 3]
    with pytest.raises(ValueError):
        dl.rectangle(4, (0, 0), (1, 1), (0, 0, 0))            # a rectangle after the text of the same frame
    with pytest.raises(ValueError):
        dl.put_text(4, "A", (0, 9), 1, (4, 5, 6))


@pytest.mark.parametrize("kind", R.BACKGROUNDS)
def test_both_note_kinds_on_every_rectangle(kind):
    H, W = 90, 160
    rects = R.rects(H, W)
    bg = R.background(kind, 2 * len(rects), H, W, seed=1)
    notes = [(2 * i + k, R.INDICES[i % len(R.INDICES)], r, bool(k)) for i, r in enumerate(rects) for k in (0, 1)]
    want, got = check_notes(bg, notes)
    assert np.array_equal(want, got)
    assert (want != bg).reshape(len(bg), -1).any(1).sum() >= len(bg) - 2    # (only the captions above / outside the frame leave no mark)


@pytest.mark.parametrize("index", R.INDICES)
def test_flagged_caption_with_every_digit(index):
    bg = R.background("ramp", 1, 48, 470, seed=index)
    want, got = check_notes(bg, [(0, index, (200, 20, 260, 44), True)])
    assert np.array_equal(want, got) and (want != bg).any()


def test_ramp_puts_every_byte_value_under_partly_covered_pixels():
    bg = R.background("ramp", 1, 48, 470)
    ink = R.background("zeros", 1, 48, 470)
    R.host_annotate(ink, [(0, 88888, (600, 600, 700, 700), True)])           # red on black: the red channel is the coverage
    partly = (ink[0, :, :, 2] > 0) & (ink[0, :, :, 2] < 255)
    for c in range(3):                                         # (all but one value per channel under this caption; the others' digits add it)
        assert len(np.unique(bg[0][partly][:, c])) >= 255


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (16, 24), (37, 53), (101, 333), (360, 640), (1080, 1920)])
def test_frame_sizes(H, W):
    rects = [(W // 4, H // 3, W // 2 + W // 5, H // 2 + H // 4), (-2, 9, W // 2, H + 3), (W // 3, 4, W - 1, H - 1)]
    bg = R.background("noise", 4, H, W, seed=H)
    notes = [(0, 123456, rects[0], True), (1, 968, rects[1], False), (3, 1350, rects[2], False)]
    want, got = check_notes(bg, notes)
    assert np.array_equal(want, got)
    assert np.array_equal(got[2], bg[2])


@pytest.mark.parametrize("scale,thickness,org", [(0.3, 1, (3, 20)), (0.75, 2, (2.5, 30.25)), (1.7, 3, (-12, 41)), (2, 1, (40, 70)),
                                                 (0.5, 3, (100, 8)), (1, 2, (150, 95))])
@pytest.mark.parametrize("kind", ("noise", "ramp"))
def test_generic_text_and_rectangle(scale, thickness, org, kind):
    H, W = 96, 200
    bg = R.background(kind, 2, H, W, seed=thickness)
    want = bg.copy()
    A.rectangle(want[1], (20, 70), (9, 12), (9, 200, 77), thickness)
    A.put_text(want[1], "Frame 4096 - Real", org, scale, (250, 3, 128), thickness)
    A.put_text(want[0], "Detected 57", org, scale, (0, 255, 0), thickness)
    dl = A.DrawList()
    dl.rectangle(1, (20, 70), (9, 12), (9, 200, 77), thickness)
    dl.put_text(1, "Frame 4096 - Real", org, scale, (250, 3, 128), thickness)
    dl.put_text(0, "Detected 57", org, scale, (0, 255, 0), thickness)
    got = bg.copy()
    R.draw(got, *dl.arrays())
    assert np.array_equal(want, got) and (want != bg).any()


def test_drawing_twice_blends_twice():
    bg = R.background("noise", 1, 60, 200, seed=4)
    notes = [(0, 42, (30, 25, 90, 50), False)]
    want, got = bg.copy(), bg.copy()
    for _ in range(2):
        R.host_annotate(want, notes)
        R.draw(got, *A.draw_list(notes))
    once = bg.copy()
    R.host_annotate(once, notes)
    assert np.array_equal(want, got) and not np.array_equal(want, once)


def thick_case():
    n, H, W = 16, 540, 3840
    bg = R.background("noise", n, H, W, seed=3)
    want, dl = bg.copy(), A.DrawList()
    for row, text, org, scale, col, th in R.thick_lines(n, H, W):
        A.put_text(want[row], text, org, scale, col, th)
        dl.put_text(row, text, org, scale, col, th)
    return bg, want, dl.arrays()


def test_thick_lines_and_the_hypot_form():
    """Long thick strokes: the restatement (run on arrays: ~20 million pixel-segment pairs) still equals annotate.py, and the
    same run with float32 sqrt(x*x + y*y) does not -- so a kernel that uses it fails this case, the one the GPU test repeats."""
    bg, want, (flist, segs) = thick_case()
    got = bg.copy()
    R.draw(got, flist, segs, scalar=False)
    assert np.array_equal(want, got)
    bad = bg.copy()
    R.draw(bad, flist, segs, hypot=R.hypot_float, scalar=False)
    assert 0 < (bad != want).sum() < 100                       # a handful of bytes, each off by one
    assert np.abs(bad.astype(int) - want).max() == 1


def test_array_run_equals_scalar_run():
    bg = R.background("ramp", 2, 60, 330, seed=2)
    notes = [(0, 790, (30, 25, 90, 50), True), (1, 7, (300, 20, 340, 70), False)]
    a, b = bg.copy(), bg.copy()
    R.draw(a, *A.draw_list(notes))
    R.draw(b, *A.draw_list(notes), scalar=False)
    assert np.array_equal(a, b)


def test_hypot_form_equals_numpy_hypot():
    rng = np.random.default_rng(0)
    x = rng.uniform(-30, 30, 2_000_000).astype(np.float32)
    y = rng.uniform(-30, 30, 2_000_000).astype(np.float32)
    assert np.array_equal(np.hypot(x, y), np.sqrt(x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2).astype(np.float32))
