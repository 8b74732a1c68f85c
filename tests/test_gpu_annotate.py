"""The device drawing (csrc/trl_annotate.hip: trl_draw) and the path it opens: annotate.annotate_device equals annotate.py's
own rasteriser byte for byte on every pixel of every frame of a batch; AviMjpegWriter.write_device writes the files write()
writes; run() writes the same AVI whether the frames stay on the device (the default) or are drawn on the writer thread
(TRUELY_DRAW=host) or encoded by Pillow, and by default no frame batch is copied to the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import annotate_ref as R
import truely_amd
from truely_amd import _lib, annotate as A, video_io

pytestmark = pytest.mark.gpu

ODD = np.load(os.path.join(os.path.dirname(__file__), "golden", "clip_odd.npz"))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(autouse=True)
def own_rasteriser(monkeypatch):
    monkeypatch.setattr(A, "cv2", None)                     # the kernel follows this module's rasteriser, not OpenCV's


def device_annotate(bg, notes, dev, **kw):
    d = torch.from_numpy(bg).to(dev)
    A.annotate_device(d, notes, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy()


def spread_notes(n, H, W, every=2):
    """Both note kinds over the rectangles of the grid, on every ``every``-th frame of an n-frame batch."""
    rects = R.rects(H, W)
    return [(f, R.INDICES[k % len(R.INDICES)], rects[k % len(rects)], bool((k // len(rects) + k) % 2))
            for k, f in enumerate(range(0, n, every))]


# ---- the kernel against annotate.py ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.BACKGROUNDS)
@pytest.mark.parametrize("H,W,n", [(360, 640, 53), (720, 1280, 27), (int(ODD["H"]), int(ODD["W"]), 53), (2160, 3840, 6)])
def test_device_equals_host_on_every_pixel(dev, H, W, n, kind):
    bg = R.background(kind, n, H, W, seed=n)
    notes = spread_notes(n, H, W)
    if H == 2160:                                           # few frames: note them all but one, kinds alternating
        notes = [(f, R.INDICES[f], R.rects(H, W)[2 * f], bool(f % 2)) for f in range(n - 1)]
    want = bg.copy()
    R.host_annotate(want, notes)
    got = device_annotate(bg, notes, dev)
    assert np.array_equal(want, got)
    noted = {f for f, *_ in notes}
    assert all(np.array_equal(got[f], bg[f]) for f in range(n) if f not in noted)
    assert sum((want[f] != bg[f]).any() for f in noted) >= len(noted) - 4   # (a note wholly outside its frame leaves no mark)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (16, 24), (37, 53)])
def test_tiny_frames_clip_the_text_on_all_sides(dev, H, W):
    bg = R.background("noise", 26, H, W, seed=W)
    notes = [(2 * k, R.INDICES[k % 7], r, bool(k % 2)) for k, r in enumerate(R.rects(H, W))]
    want = bg.copy()
    R.host_annotate(want, notes)
    assert np.array_equal(want, device_annotate(bg, notes, dev))


@pytest.mark.parametrize("index", R.INDICES)
def test_every_digit_on_the_ramp(dev, index):
    bg = R.background("ramp", 3, 48, 470, seed=index)
    notes = [(1, index, (200, 20, 260, 44), True)]
    want = bg.copy()
    R.host_annotate(want, notes)
    assert np.array_equal(want, device_annotate(bg, notes, dev))


@pytest.mark.parametrize("scale,thickness,org", [(0.3, 1, (3, 20)), (0.75, 2, (2.5, 30.25)), (1.7, 3, (-12, 41)), (2, 1, (40, 70)),
                                                 (0.5, 3, (100, 8)), (1, 2, (150, 95))])
def test_generic_text_and_rectangle(dev, scale, thickness, org):
    H, W = 96, 200
    bg = R.background("noise", 3, H, W, seed=thickness)
    want = bg.copy()
    A.rectangle(want[1], (20, 70), (9, 12), (9, 200, 77), thickness)
    A.put_text(want[1], "Frame 4096 - Real", org, scale, (250, 3, 128), thickness)
    A.put_text(want[0], "Detected 57", org, scale, (0, 255, 0), thickness)
    dl = A.DrawList()
    dl.rectangle(1, (20, 70), (9, 12), (9, 200, 77), thickness)
    dl.put_text(1, "Frame 4096 - Real", org, scale, (250, 3, 128), thickness)
    dl.put_text(0, "Detected 57", org, scale, (0, 255, 0), thickness)
    d = torch.from_numpy(bg).to(dev)
    A.draw_device(d, *dl.arrays())
    # the public single-frame entry points take a device frame as well
    video_io.draw_box(d[2], 5, 6, 50, 60, (1, 2, 3), thickness)
    video_io.put_text(d[2], "Real 8", org, scale, (7, 8, 9), thickness)
    A.rectangle(want[2], (5, 6), (50, 60), (1, 2, 3), thickness)
    A.put_text(want[2], "Real 8", org, scale, (7, 8, 9), thickness)
    torch.cuda.synchronize()
    assert np.array_equal(want, d.cpu().numpy())


def test_thick_lines_pin_the_hypot_form(dev):
    """The case tests/test_annotate_cpu.py shows to separate float32 sqrt(x*x + y*y) from numpy's hypot: long strokes 21 to 51
    pixels thick, more than 300 segments per frame (the kernel stages them in LDS in chunks)."""
    n, H, W = 16, 540, 3840
    bg = R.background("noise", n, H, W, seed=3)
    want, dl = bg.copy(), A.DrawList()
    for row, text, org, scale, col, th in R.thick_lines(n, H, W):
        A.put_text(want[row], text, org, scale, col, th)
        dl.put_text(row, text, org, scale, col, th)
    flist, segs = dl.arrays()
    assert (flist["seg_end"] - flist["seg_begin"]).max() > 256
    d = torch.from_numpy(bg).to(dev)
    A.draw_device(d, flist, segs)
    torch.cuda.synchronize()
    assert np.array_equal(want, d.cpu().numpy())


def test_strided_batch_side_stream_and_repeat_calls(dev):
    """Frames inside a larger buffer with sentinel bytes between and after them, drawn on a non-default stream, twice: what
    annotate.py gives when it draws twice; no sentinel byte changes."""
    n, H, W, gap = 9, 90, 160, 77
    bg = R.background("noise", n, H, W, seed=8)
    notes = spread_notes(n, H, W, every=1)[:n - 2]
    stride = H * W * 3 + gap
    buf = torch.full((n * stride + 64,), 0xA5, dtype=torch.uint8, device=dev)
    frames = torch.as_strided(buf, (n, H, W, 3), (stride, W * 3, 3, 1))
    frames.copy_(torch.from_numpy(bg).to(dev))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    want = bg.copy()
    for _ in range(2):
        A.annotate_device(frames, notes, stream=side)
        R.host_annotate(want, notes)
    side.synchronize()
    once = bg.copy()
    R.host_annotate(once, notes)
    assert not np.array_equal(want, once)                   # (drawing twice blends the soft edges twice: the case is not vacuous)
    assert np.array_equal(frames.cpu().numpy(), want)
    raw = buf.cpu().numpy()
    pad = np.concatenate([raw[k * stride + H * W * 3:(k + 1) * stride] for k in range(n)] + [raw[n * stride:]])
    assert (pad == 0xA5).all()
    with torch.cuda.stream(side):                           # the current stream is the default when none is given
        A.annotate_device(frames, notes)
    side.synchronize()
    R.host_annotate(want, notes)
    assert np.array_equal(frames.cpu().numpy(), want)


def test_abi_refusals_leave_the_frames_untouched(dev):
    lib = _lib.load()
    n, H, W = 4, 40, 60
    bg = R.background("noise", n, H, W, seed=2)
    d = torch.from_numpy(bg).to(dev)
    flist, segs = A.draw_list([(1, 42, (5, 5, 30, 30), True), (3, 7, (5, 15, 30, 30), False)])
    need = lib.trl_draw_workspace(len(flist), len(segs))
    work = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(fl=flist, sg=segs, n_=n, stride=H * W * 3, H_=H, W_=W, nf=None, ns=None, wb=need, w=work):
        fl, sg = np.ascontiguousarray(fl), np.ascontiguousarray(sg)
        return lib.trl_draw(C.c_void_p(d.data_ptr()), n_, stride, H_, W_, fl.ctypes.data_as(C.c_void_p), len(fl) if nf is None else nf,
                            sg.ctypes.data_as(C.c_void_p), len(sg) if ns is None else ns, C.c_void_p(w.data_ptr()), wb, None)

    def edited(arr, i, **kw):
        a = arr.copy()
        for k, v in kw.items():
            a[k][i] = v
        return a
    bad = [dict(fl=edited(flist, 1, frame=n)), dict(fl=edited(flist, 0, frame=-1)), dict(fl=edited(flist, 1, frame=1)),
           dict(fl=edited(flist, 1, seg_end=len(segs) + 1)), dict(fl=edited(flist, 1, seg_begin=-1)),
           dict(fl=edited(flist, 0, seg_begin=5, seg_end=4)), dict(fl=edited(flist, 0, thickness=-2)),
           dict(sg=edited(segs, 3, x0=np.nan)), dict(sg=edited(segs, 3, dx=np.inf)),
           dict(stride=H * W * 3 - 1), dict(H_=0), dict(W_=-3), dict(n_=0), dict(nf=-1), dict(ns=-1), dict(wb=need - 300)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"trl_draw" in lib.trl_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), bg)
    assert call(nf=0) == 0 and call(fl=flist[:0], sg=segs[:0]) == 0          # nothing to draw
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), bg)
    assert call() == 0                                                       # ... and the same lists, unedited, draw
    torch.cuda.synchronize()
    want = bg.copy()
    R.host_annotate(want, [(1, 42, (5, 5, 30, 30), True), (3, 7, (5, 15, 30, 30), False)])
    assert np.array_equal(d.cpu().numpy(), want)


# ---- the writer -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [(1, 31, 32, 33, 75), (75, 1, 33)])
def test_write_device_files_equal_write_files(dev, tmp_path, lengths):
    H, W = 72, 104
    total = sum(lengths) + 2 * len(lengths)
    fr = truely_amd.synthetic.synthetic_frames(total, H, W, seed=6)
    a, b = str(tmp_path / "a.avi"), str(tmp_path / "b.avi")
    wa = video_io.AviMjpegWriter(a, 30, (W, H), encoder="device", device=dev)
    wb = video_io.AviMjpegWriter(b, 30, (W, H), encoder="device", device=dev)
    k = 0
    for n in lengths:                                       # host frames before and after every device batch keep their place
        wa.write(fr[k]); wb.write(fr[k]); k += 1
        wa.write_device(torch.from_numpy(fr[k:k + n]).to(dev))
        for f in fr[k:k + n]:
            wb.write(f)
        k += n
        wa.write(fr[k]); wb.write(fr[k]); k += 1
    wa.release(); wb.release()
    assert open(a, "rb").read() == open(b, "rb").read()
    rd = video_io.AviMjpegReader(a)
    assert rd.n == total
    rd.release()
    with pytest.raises(ValueError):
        video_io.AviMjpegWriter(str(tmp_path / "c.avi"), 30, (W, H)).write_device(torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev))


def test_async_writer_batches_keep_order_and_bound(dev, tmp_path):
    H, W = 48, 64
    fr = truely_amd.synthetic.synthetic_frames(40, H, W, seed=2)
    notes = [(3, 7, (5, 5, 40, 40), True), (9, 8, (5, 15, 40, 40), False)]
    a, b = str(tmp_path / "a.avi"), str(tmp_path / "b.avi")
    w = video_io.AsyncWriter(video_io.AviMjpegWriter(a, 30, (W, H), encoder="device", device=dev), depth=16)
    w.put(fr[0].copy())
    ev = torch.cuda.Event()
    d = torch.from_numpy(fr[1:21]).to(dev)
    ev.record()
    w.put_batch(d, notes, ev)                               # 20 frames > depth: goes in alone
    w.put_batch(torch.from_numpy(fr[21:39]).to(dev), [], None)
    w.put(fr[39].copy())
    w.close()
    assert w.frames == 40
    ref = fr.copy()
    for row, index, rect, flagged in notes:
        A.annotate(ref[1 + row], index, rect, flagged)
    wb = video_io.AviMjpegWriter(b, 30, (W, H), encoder="device", device=dev)
    for f in ref:
        wb.write(f)
    wb.release()
    assert open(a, "rb").read() == open(b, "rb").read()


# ---- run() ------------------------------------------------------------------------------------------------------------------------
def _clip(tmp_path, kind, fr, fps):
    from truely_amd.ingest import bgr_to_nv12
    H, W = fr.shape[1:3]
    if kind == "bgr":
        src = str(tmp_path / "in_bgr.trlv")
        video_io.write_raw(src, fr, fps)
    elif kind == "nv12":
        src = str(tmp_path / "in_nv12.trlv")
        video_io.write_raw(src, bgr_to_nv12(fr), fps, pixfmt="nv12", size=(W, H))
    else:
        src = str(tmp_path / "in.y4m")
        video_io.write_y4m(src, bgr_to_nv12(fr), fps, (W, H))
    return src


def _run_modes(tmp_path, monkeypatch, src, engine):
    """run() by default, with TRUELY_DRAW=host and with TRUELY_JPEG=pillow: (score, file) each, the notes the default run drew
    (spied where they reach the device), how often write_device ran, and the largest tensor .cpu() was called on."""
    from truely_amd import engine as eng_mod, model
    monkeypatch.setattr(eng_mod, "_default", engine)
    spy = {"notes": [], "write_device": 0, "cpu_bytes": 0, "host_notes": []}
    real_dev, real_host, real_wd, real_cpu = A.annotate_device, A.annotate, video_io.AviMjpegWriter.write_device, torch.Tensor.cpu

    def spy_dev(frames, notes, stream=None):
        spy["notes"] += [(n[1], bool(n[3])) for n in notes]
        return real_dev(frames, notes, stream)

    def spy_host(frame, index, rect, flagged):
        spy["host_notes"].append((index, bool(flagged)))
        return real_host(frame, index, rect, flagged)

    def spy_wd(self, frames):
        spy["write_device"] += 1
        return real_wd(self, frames)

    def spy_cpu(self, *a, **k):
        if self.is_cuda:
            spy["cpu_bytes"] = max(spy["cpu_bytes"], self.numel() * self.element_size())
        return real_cpu(self, *a, **k)
    monkeypatch.setattr(A, "annotate_device", spy_dev)
    monkeypatch.setattr(A, "annotate", spy_host)
    monkeypatch.setattr(video_io.AviMjpegWriter, "write_device", spy_wd)
    outs = {}
    for mode, env in (("device", {}), ("host", {"TRUELY_DRAW": "host"}), ("pillow", {"TRUELY_JPEG": "pillow"})):
        for k in ("TRUELY_DRAW", "TRUELY_JPEG", "TRUELY_ANNOTATE", "TRUELY_WRITE_OUTPUT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dst = str(tmp_path / f"out_{mode}.avi")
        if mode == "device":
            monkeypatch.setattr(torch.Tensor, "cpu", spy_cpu)
        try:
            score = model.run(src, dst)
        finally:
            monkeypatch.setattr(torch.Tensor, "cpu", real_cpu)
        outs[mode] = (score, open(dst, "rb").read())
        if mode == "device":
            spy["device_calls"], spy["device_host_notes"] = spy["write_device"], len(spy["host_notes"])
    return outs, spy


def _check_modes(outs, spy, nframes, frame_bytes, tmp_path):
    assert isinstance(outs["device"][0], int) and outs["device"][0] == outs["host"][0] == outs["pillow"][0]
    assert len(outs["device"][1]) > 10000
    assert outs["device"][1] == outs["host"][1]
    assert outs["device"][1] == outs["pillow"][1]
    kinds = {f for _, f in spy["notes"]}
    assert kinds == {True, False}, f"the clip must produce flagged and unflagged notes, got {spy['notes']}"
    assert sorted(spy["notes"]) == sorted(set(spy["host_notes"])) and len(spy["host_notes"]) == 2 * len(spy["notes"])
    assert spy["device_calls"] >= 1 and spy["device_host_notes"] == 0          # the default path drew and wrote on the device
    assert spy["write_device"] == spy["device_calls"]                          # ... and the other two never did
    assert spy["cpu_bytes"] < frame_bytes                                      # no frame (let alone a batch) came back to the host
    rd = video_io.AviMjpegReader(str(tmp_path / "out_device.avi"))
    assert rd.n == nframes
    rd.release()


@pytest.mark.parametrize("kind", ["bgr", "nv12", "y4m"])
def test_run_avi_identical_whichever_side_draws(engine, tmp_path, monkeypatch, kind):
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    H, W, fps, N = 360, 640, 30, 88                      # configs[0]'s frame shape; 22 sampled frames, every one with a face
    fr = truely_amd.synthetic.synthetic_frames(N, H, W, seed=4)
    outs, spy = _run_modes(tmp_path, monkeypatch, _clip(tmp_path, kind, fr, fps), engine)
    _check_modes(outs, spy, N, H * W * 3, tmp_path)


def test_run_avi_identical_odd_clip(engine, tmp_path, monkeypatch):
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    H, W = int(ODD["H"]), int(ODD["W"])
    fr = truely_amd.synthetic.synthetic_frames(66, H, W, seed=7)             # (the golden's own seed shows no face; this one 22 of 22)
    outs, spy = _run_modes(tmp_path, monkeypatch, _clip(tmp_path, "bgr", fr, 25), engine)
    _check_modes(outs, spy, 66, H * W * 3, tmp_path)


def long_clip(N, H, W):
    """40 frames with a face (35 of them detected), each held for 4 and cycled; the frame number is stamped into the top left
    corner, 16 pixels of 0 / 255, so that no two frames are alike."""
    base = truely_amd.synthetic.synthetic_frames(40, H, W, seed=3)
    fr = base[(np.arange(N) // 4) % 40].copy()
    bits = ((np.arange(N)[:, None] >> np.arange(16)[None, :]) & 1).astype(np.uint8) * 255
    fr[:, :2, :16, :] = bits[:, None, :, None]
    return fr


@pytest.mark.parametrize("kind", ["bgr", "nv12"])
def test_run_many_windows_reuses_buffers(engine, tmp_path, monkeypatch, kind):
    """1,100 frames = 9 windows of 128 frames: each cascade context refills its staging buffer four times, the pinned ring goes
    round twice and the writer's queue (4 windows) fills: a frame overwritten before it was encoded would change the file."""
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    H, W, fps, N = 90, 160, 30, 1100
    fr = long_clip(N, H, W)
    outs, spy = _run_modes(tmp_path, monkeypatch, _clip(tmp_path, kind, fr, fps), engine)
    assert outs["device"] == outs["host"] and spy["device_calls"] == 9 and spy["device_host_notes"] == 0
    assert {i // 128 for i, _ in spy["notes"]} == set(range(9))                # every window drew something (the CPU oracle: 17 to 31 notes each)
    assert sorted(spy["notes"]) == sorted(set(spy["host_notes"]))
    rd = video_io.AviMjpegReader(str(tmp_path / "out_device.avi"))
    assert rd.n == N
    rd.release()


def test_run_without_annotation_still_writes_on_the_device(engine, tmp_path, monkeypatch):
    from truely_amd import engine as eng_mod, model
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    monkeypatch.setattr(eng_mod, "_default", engine)
    fr = truely_amd.synthetic.synthetic_frames(40, 90, 160, seed=5)
    src = _clip(tmp_path, "nv12", fr, 30)
    files = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("TRUELY_ANNOTATE", "0")
        monkeypatch.setenv("TRUELY_DRAW", mode)
        dst = str(tmp_path / f"plain_{mode}.avi")
        model.run(src, dst)
        files[mode] = open(dst, "rb").read()
    assert files["device"] == files["host"]
