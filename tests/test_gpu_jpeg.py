"""GPU tests of the Motion-JPEG encoder (csrc/trl_jpeg.hip, jpeg.DeviceJpeg): every file it writes is byte-identical to Pillow's
for the same frame, over sizes, qualities and content that reach every edge rule, in multi-frame batches; the C ABI's capacity,
stride and stream contracts; and run()'s annotated AVI, which must not change by a byte when the device encodes it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib

from test_jpeg_cpu import KINDS, QUALITIES, SIZES, make_frame, pillow_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _batch(H, W, seed=0, reps=1):
    """Every content kind, `reps` times with different seeds: a multi-frame batch whose frames differ in size class."""
    return np.stack([make_frame(k, H, W, seed=seed + r) for r in range(reps) for k in KINDS])


def _check_equal(frames, files, q):
    assert len(files) == len(frames)
    for i, (f, got) in enumerate(zip(frames, files)):
        exp = pillow_jpeg(f, q)
        assert got == exp, f"frame {i}: {len(got)} vs {len(exp)} bytes, first difference at {_first_diff(got, exp)}"


def _first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i
    return min(len(a), len(b))


@pytest.mark.parametrize("H,W", SIZES)
def test_device_bytes_equal_pillow(dev, H, W):
    from truely_amd.jpeg import DeviceJpeg
    frames = _batch(H, W, reps=2)
    for q in QUALITIES:
        enc = DeviceJpeg(W, H, q, device=dev, max_frames=len(frames))
        _check_equal(frames, enc.encode(torch.from_numpy(frames).to(dev)), q)


ODD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_odd.npz"))


@pytest.mark.parametrize("H,W,q", [(720, 1280, 80), (720, 1280, 100), (1080, 1920, 80), (1080, 1920, 1), (2160, 3840, 80),
                                   (int(ODD["H"]), int(ODD["W"]), 80), (int(ODD["H"]), int(ODD["W"]), 30)])
def test_device_bytes_equal_pillow_large_and_golden_shapes(dev, H, W, q):
    from truely_amd.jpeg import DeviceJpeg
    frames = _batch(H, W)
    if (H, W) == (int(ODD["H"]), int(ODD["W"])):
        frames = np.concatenate([frames, truely_amd.synthetic.synthetic_frames(int(ODD["n"]), H, W, seed=int(ODD["seed"]))])
    enc = DeviceJpeg(W, H, q, device=dev, max_frames=len(frames))
    _check_equal(frames, enc.encode(torch.from_numpy(frames).to(dev)), q)


def test_batches_larger_than_a_chunk(dev):
    """4K frames take more than one internal chunk per call (the workspace holds a few 4K frames): offsets carry across chunks."""
    from truely_amd.jpeg import DeviceJpeg
    frames = np.concatenate([_batch(2160, 3840, seed=5), _batch(2160, 3840, seed=9)])
    enc = DeviceJpeg(3840, 2160, 90, device=dev, max_frames=len(frames))
    _check_equal(frames, enc.encode(torch.from_numpy(frames).to(dev)), 90)


def test_host_frames_and_max_frames_split(dev):
    from truely_amd.jpeg import DeviceJpeg
    frames = _batch(53, 37, reps=3)                      # 12 frames through a 5-frame encoder: 3 calls
    enc = DeviceJpeg(37, 53, 80, device=dev, max_frames=5)
    _check_equal(frames, enc.encode(frames), 80)


def test_strided_slice_gives_same_bytes(dev):
    from truely_amd.jpeg import DeviceJpeg
    frames = _batch(100, 30, reps=2)
    d = torch.from_numpy(frames).to(dev)
    enc = DeviceJpeg(30, 100, 95, device=dev, max_frames=8)
    sl = d[1::2]
    assert sl.stride(0) == 2 * 100 * 30 * 3
    _check_equal(frames[1::2], enc.encode(sl), 95)


def _raw_encode(h, d, n, stride, out, capacity, stream):
    lib = _lib.load()
    sizes = np.zeros(n, np.int64)
    _lib.check(lib.trl_jpeg_encode(h, C.c_void_p(d.data_ptr()), n, stride, C.c_void_p(out.data_ptr() if out is not None else 0),
                                   capacity, sizes.ctypes.data_as(C.c_void_p), C.c_void_p(stream)))
    return sizes


@pytest.fixture
def raw_encoder(dev):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.trl_jpeg_create(dev.index or 0, 119, 7 * 9, 80, 8, C.byref(h)))
    yield h
    lib.trl_jpeg_destroy(h)


def test_nothing_written_past_sizes_or_capacity(dev, raw_encoder):
    H, W = 119, 63
    frames = _batch(H, W)
    d = torch.from_numpy(frames).to(dev)
    exp = [pillow_jpeg(f, 80) for f in frames]
    total = sum(len(e) for e in exp)
    out = torch.full((total + 8192,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = _raw_encode(raw_encoder, d, len(frames), H * W * 3, out, out.numel(), 0)
    torch.cuda.synchronize()
    assert list(sizes) == [len(e) for e in exp]
    o = out.cpu().numpy()
    assert o[:total].tobytes() == b"".join(exp)
    assert (o[total:] == 0xA5).all()
    # room for the first two files and a few bytes: those two are written, nothing else is touched
    cap = len(exp[0]) + len(exp[1]) + 5
    out.fill_(0x5A)
    sizes = _raw_encode(raw_encoder, d, len(frames), H * W * 3, out, cap, 0)
    torch.cuda.synchronize()
    assert list(sizes) == [len(e) for e in exp]
    o = out.cpu().numpy()
    assert o[:cap - 5].tobytes() == exp[0] + exp[1]
    assert (o[cap - 5:] == 0x5A).all()
    # no buffer at all: sizes only
    sizes = _raw_encode(raw_encoder, d, len(frames), H * W * 3, None, 0, 0)
    assert list(sizes) == [len(e) for e in exp]


def test_tiny_capacity_grows_and_reruns(dev):
    from truely_amd.jpeg import DeviceJpeg
    frames = _batch(180, 320, reps=2)
    enc = DeviceJpeg(320, 180, 100, device=dev, max_frames=len(frames))
    enc._grow(12)
    enc.capacity = 16
    files = enc.encode(torch.from_numpy(frames).to(dev))
    assert enc.reruns == 1 and enc.capacity >= sum(len(f) for f in files)
    _check_equal(frames, files, 100)


def test_non_default_stream_and_repeat_calls(dev, raw_encoder):
    H, W = 119, 63
    frames = _batch(H, W, seed=3)
    d = torch.from_numpy(frames).to(dev)
    out = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    s0 = _raw_encode(raw_encoder, d, len(frames), H * W * 3, out, out.numel(), 0)
    torch.cuda.synchronize()
    a = out.cpu().numpy()[:s0.sum()].tobytes()
    side = torch.cuda.Stream(dev)
    out2 = torch.zeros_like(out)
    side.wait_stream(torch.cuda.current_stream(dev))
    s1 = _raw_encode(raw_encoder, d, len(frames), H * W * 3, out2, out2.numel(), side.cuda_stream)
    s2 = _raw_encode(raw_encoder, d, len(frames), H * W * 3, out2, out2.numel(), side.cuda_stream)
    side.synchronize()
    assert list(s0) == list(s1) == list(s2)
    assert out2.cpu().numpy()[:s1.sum()].tobytes() == a == b"".join(pillow_jpeg(f, 80) for f in frames)


def test_encode_rejects_bad_arguments(dev, raw_encoder):
    lib = _lib.load()
    d = torch.zeros((2, 119, 63, 3), dtype=torch.uint8, device=dev)
    sizes = np.zeros(16, np.int64)
    for n, stride in ((9, 119 * 63 * 3), (-1, 119 * 63 * 3), (2, 100)):
        st = lib.trl_jpeg_encode(raw_encoder, C.c_void_p(d.data_ptr()), n, stride, None, 0, sizes.ctypes.data_as(C.c_void_p), None)
        assert st == -1 and b"trl_jpeg_encode" in lib.trl_last_error()
    h = C.c_void_p()
    assert lib.trl_jpeg_create(dev.index or 0, 0, 64, 80, 4, C.byref(h)) == -1 and not h.value


# ---- run(): the annotated output is the same file whichever encoder writes it ------------------------------------------------
def _run_both(tmp_path, monkeypatch, src, tag):
    from truely_amd import model
    outs = {}
    for enc in ("pillow", "device"):
        monkeypatch.setenv("TRUELY_JPEG", enc)
        dst = str(tmp_path / f"{tag}_{enc}.avi")
        outs[enc] = (model.run(src, dst), open(dst, "rb").read())
    return outs


@pytest.mark.parametrize("pixfmt", ["bgr", "nv12"])
def test_run_avi_identical_with_device_encoder(engine, tmp_path, monkeypatch, pixfmt):
    from truely_amd import engine as eng_mod, video_io
    from truely_amd.ingest import bgr_to_nv12
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    monkeypatch.setattr(eng_mod, "_default", engine)
    H, W, fps, N = 360, 640, 30, 75                      # configs[0]'s frame shape; 75 frames = 2 full device batches + a partial one
    fr = truely_amd.synthetic.synthetic_frames(N, H, W, seed=4)
    src = str(tmp_path / f"in_{pixfmt}.trlv")
    if pixfmt == "nv12":
        video_io.write_raw(src, bgr_to_nv12(fr), fps, pixfmt="nv12", size=(W, H))
    else:
        video_io.write_raw(src, fr, fps)
    outs = _run_both(tmp_path, monkeypatch, src, pixfmt)
    assert outs["device"][0] == outs["pillow"][0]
    assert len(outs["device"][1]) > 10000 and outs["device"][1] == outs["pillow"][1]
    rd = video_io.AviMjpegReader(str(tmp_path / f"{pixfmt}_device.avi"))
    assert rd.n == N
    rd.release()


def test_run_avi_identical_odd_clip(engine, tmp_path, monkeypatch):
    from truely_amd import engine as eng_mod, video_io
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    monkeypatch.setattr(eng_mod, "_default", engine)
    H, W = int(ODD["H"]), int(ODD["W"])
    fr = truely_amd.synthetic.synthetic_frames(40, H, W, seed=int(ODD["seed"]))
    src = str(tmp_path / "odd.trlv")
    video_io.write_raw(src, fr, 25)
    outs = _run_both(tmp_path, monkeypatch, src, "odd")
    assert outs["device"] == outs["pillow"]


def test_run_uses_device_encoder_by_default(engine, tmp_path, monkeypatch):
    """Without TRUELY_JPEG run() hands its engine's device to the writer."""
    from truely_amd import engine as eng_mod, model, video_io
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    monkeypatch.setattr(eng_mod, "_default", engine)
    monkeypatch.delenv("TRUELY_JPEG", raising=False)
    seen = []
    orig = video_io.AviMjpegWriter.__init__

    def spy(self, *a, **k):
        orig(self, *a, **k)
        seen.append(self.encoder)
    monkeypatch.setattr(video_io.AviMjpegWriter, "__init__", spy)
    fr = truely_amd.synthetic.synthetic_frames(8, 64, 96, seed=1)
    src = str(tmp_path / "s.trlv")
    video_io.write_raw(src, fr, 30)
    model.run(src, str(tmp_path / "s.avi"))
    assert seen == ["device"]
