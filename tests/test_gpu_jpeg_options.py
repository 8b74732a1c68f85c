"""GPU tests of the Motion-JPEG encoder's options (csrc/trl_jpeg.hip, jpeg.DeviceJpeg): 4:4:4 / 4:2:2 / 4:2:0, restart intervals and
per-frame optimal Huffman tables.  Every file equals Pillow's for the same frame and options, byte for byte, and decodes on the
device (jpeg.DeviceJpegDecoder) to Pillow's pixels; the defaults still give trl_jpeg_create's bytes; run() passes the options
from the environment to whichever encoder writes."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib

import jpeg_options_ref as R
from test_jpeg_cpu import make_frame, pillow_jpeg

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (17, 15), (33, 31), (64, 48), (100, 75), (320, 180)]       # (W, H): the CPU grid's cases named by the issue
SAMPLINGS = [0, 1, 2]
QUALITIES = [1, 50, 80, 100]
KINDS = ["noise", "gradient", "constant", "saturated"]
INTERVALS = [(0, 0), (1, 0), (0, 1), (0, 3)]                                # (restart_rows, restart_blocks)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


_expected = {}


def expected(kind, H, W, seed, q, s, rr, rb, opt):
    """Pillow's file of make_frame(kind, H, W, seed) with these options, computed once."""
    key = (kind, H, W, seed, q, s, rr, rb, opt)
    if key not in _expected:
        _expected[key] = R.pillow(make_frame(kind, H, W, seed), q, s, rr, rb, opt)
    return _expected[key]


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1]


def _first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i
    return min(len(a), len(b))


def check_files(files, exp, what):
    assert len(files) == len(exp)
    for i, (got, e) in enumerate(zip(files, exp)):
        assert got == e, f"{what} frame {i}: {len(got)} vs {len(e)} bytes, first difference at {_first_diff(got, e)}"


def check_round_trip(dec, files):
    """DeviceJpegDecoder reads every file on the device (status 0) and gives Pillow's pixels."""
    frames, status = dec.decode(files)
    assert (status == 0).all(), status
    got = frames.cpu().numpy()
    for k, f in enumerate(files):
        assert np.array_equal(got[k], pillow_pixels(f)), k


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("s", SAMPLINGS)
def test_device_bytes_equal_pillow_and_round_trip(dev, W, H, s):
    from truely_amd.jpeg import DeviceJpeg, DeviceJpegDecoder
    frames = np.stack([make_frame(k, H, W) for k in KINDS])
    d = torch.from_numpy(frames).to(dev)
    dec = DeviceJpegDecoder(W, H, device=dev, max_frames=len(KINDS) * len(INTERVALS) * 2)
    for q in QUALITIES:
        files = []
        for rr, rb in INTERVALS:
            for opt in (False, True):
                enc = DeviceJpeg(W, H, q, device=dev, max_frames=len(frames), subsampling=s, restart_rows=rr, restart_blocks=rb,
                                 optimize=opt)
                got = enc.encode(d)
                check_files(got, [expected(k, H, W, 0, q, s, rr, rb, opt) for k in KINDS], (q, rr, rb, opt))
                files += got
        check_round_trip(dec, files)


@pytest.mark.parametrize("s,rr,rb,opt", [(0, 1, 0, True), (1, 1, 0, True), (2, 1, 0, True), (0, 0, 3, False), (1, 0, 0, False),
                                         (2, 0, 1, False)])
def test_batch_of_three_640x360(dev, s, rr, rb, opt):
    from truely_amd.jpeg import DeviceJpeg, DeviceJpegDecoder
    H, W = 360, 640
    kinds = ("noise", "saturated", "gradient")
    frames = np.stack([make_frame(k, H, W) for k in kinds])
    enc = DeviceJpeg(W, H, 80, device=dev, max_frames=3, subsampling=s, restart_rows=rr, restart_blocks=rb, optimize=opt)
    files = enc.encode(torch.from_numpy(frames).to(dev))
    check_files(files, [expected(k, H, W, 0, 80, s, rr, rb, opt) for k in kinds], (s, rr, rb, opt))
    check_round_trip(DeviceJpegDecoder(W, H, device=dev, max_frames=3), files)


@pytest.mark.parametrize("s", [0, 1])
def test_optioned_batch_larger_than_a_chunk(dev, s):
    """Three 4K frames in one call with a marker per MCU row and optimize.  A block costs the workspace 372 bytes, so a 4:4:4 frame
    (388,800 blocks) takes 145 MB and a 4:2:2 frame (259,200) 96 MB: the 256 MB budget holds one and two, and the call runs in
    chunks of 1 + 1 + 1 and of 2 + 1.  A later chunk's frames use table, header-length and interval-start slots indexed within
    the chunk and output offsets indexed across chunks; every file still equals Pillow's."""
    from truely_amd.jpeg import DeviceJpeg
    H, W = 2160, 3840
    kinds = ("noise", "gradient", "saturated")
    frames = np.stack([make_frame(k, H, W) for k in kinds])
    enc = DeviceJpeg(W, H, 80, device=dev, max_frames=3, subsampling=s, restart_rows=1, optimize=True)
    files = enc.encode(torch.from_numpy(frames).to(dev))
    check_files(files, [expected(k, H, W, 0, 80, s, 1, 0, True) for k in kinds], s)


@pytest.mark.parametrize("s", SAMPLINGS)
def test_mixed_content_batch_keeps_tables_apart(dev, s):
    """Noise, a constant frame and a gradient in one batch under optimize: every frame carries its own four tables (the constant
    frame's are 20 bytes each), in either order of the batch."""
    from truely_amd.jpeg import DeviceJpeg, DeviceJpegDecoder
    H, W = 75, 100
    kinds = ("noise", "constant", "gradient")
    enc = DeviceJpeg(W, H, 80, device=dev, max_frames=3, subsampling=s, restart_rows=1, optimize=True)
    dec = DeviceJpegDecoder(W, H, device=dev, max_frames=3)
    for order in (kinds, kinds[::-1]):
        frames = np.stack([make_frame(k, H, W) for k in order])
        files = enc.encode(torch.from_numpy(frames).to(dev))
        check_files(files, [expected(k, H, W, 0, 80, s, 1, 0, True) for k in order], order)
        check_round_trip(dec, files)
    const = files[order.index("constant")]
    assert const.count(b"\xff\xc4\x00\x14") == 2            # its AC tables hold the EOB alone: 20-byte DHTs of one 1-bit code
    # mid-grey without restarts: every DC difference is 0 as well, so all four DHT segments are 20 bytes
    grey = np.full((1, H, W, 3), 128, np.uint8)
    enc = DeviceJpeg(W, H, 80, device=dev, max_frames=3, subsampling=s, optimize=True)
    files = enc.encode(torch.from_numpy(np.concatenate([frames[:1], grey, frames[2:]])).to(dev))
    assert files[1] == R.pillow(grey[0], 80, s, 0, 0, True) and files[1].count(b"\xff\xc4\x00\x14") == 4
    check_round_trip(dec, files)


def _create_ex(dev, H, W, q, s, rr, rb, opt, max_frames):
    lib = _lib.load()
    h = C.c_void_p()
    o = _lib.TrlJpegOptions(q, s, rr, rb, int(opt))
    _lib.check(lib.trl_jpeg_create_ex(dev.index or 0, H, W, C.byref(o), max_frames, C.byref(h)))
    return h


def _raw_encode(h, d, n, stride, out, capacity, stream):
    lib = _lib.load()
    sizes = np.zeros(n, np.int64)
    _lib.check(lib.trl_jpeg_encode(h, C.c_void_p(d.data_ptr()), n, stride, C.c_void_p(out.data_ptr() if out is not None else 0),
                                   capacity, sizes.ctypes.data_as(C.c_void_p), C.c_void_p(stream)))
    return sizes


@pytest.mark.parametrize("s,rr,rb,opt", [(0, 1, 0, True), (1, 0, 3, False), (2, 0, 1, True)])
def test_strided_batch_side_stream_and_capacity(dev, s, rr, rb, opt):
    """The C ABI's contracts on an optioned handle: frames at a stride with sentinel bytes between them (unchanged afterwards), a
    side stream, nothing written past the sizes, and a capacity that holds only the first two files."""
    lib = _lib.load()
    H, W = 31, 33
    n = len(KINDS)
    fb = H * W * 3
    stride = fb + 1000
    buf = torch.full((n * stride,), 0xC3, dtype=torch.uint8, device=dev)
    frames = [make_frame(k, H, W, seed=2) for k in KINDS]
    for k, f in enumerate(frames):
        buf[k * stride:k * stride + fb] = torch.from_numpy(f.reshape(-1)).to(dev)
    exp = [expected(k, H, W, 2, 80, s, rr, rb, opt) for k in KINDS]
    total = sum(len(e) for e in exp)
    h = _create_ex(dev, H, W, 80, s, rr, rb, opt, 8)
    try:
        side = torch.cuda.Stream(dev)
        out = torch.full((total + 4096,), 0xA5, dtype=torch.uint8, device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        sizes = _raw_encode(h, buf, n, stride, out, out.numel(), side.cuda_stream)
        side.synchronize()
        assert list(sizes) == [len(e) for e in exp]
        o = out.cpu().numpy()
        assert o[:total].tobytes() == b"".join(exp) and (o[total:] == 0xA5).all()
        b = buf.cpu().numpy().reshape(n, stride)
        assert (b[:, fb:] == 0xC3).all() and all((b[k, :fb] == frames[k].reshape(-1)).all() for k in range(n))
        cap = len(exp[0]) + len(exp[1]) + 5
        out.fill_(0x5A)
        sizes = _raw_encode(h, buf, n, stride, out, cap, 0)
        torch.cuda.synchronize()
        assert list(sizes) == [len(e) for e in exp]
        o = out.cpu().numpy()
        assert o[:cap - 5].tobytes() == exp[0] + exp[1] and (o[cap - 5:] == 0x5A).all()
    finally:
        lib.trl_jpeg_destroy(h)


@pytest.mark.parametrize("s", SAMPLINGS)
def test_same_encoder_twice_and_capacity_overflow(dev, s):
    """One encoder, two batches of different content (nothing of the first, tables included, survives into the second), then a
    batch that overflows a tiny capacity: the encoder grows, re-runs and gives the same bytes."""
    from truely_amd.jpeg import DeviceJpeg, DeviceJpegDecoder
    H, W = 75, 100
    enc = DeviceJpeg(W, H, 100, device=dev, max_frames=4, subsampling=s, restart_blocks=3, optimize=True)
    for seed in (0, 5):
        frames = np.stack([make_frame(k, H, W, seed) for k in KINDS])
        check_files(enc.encode(torch.from_numpy(frames).to(dev)), [expected(k, H, W, seed, 100, s, 0, 3, True) for k in KINDS], seed)
    before = enc.reruns
    enc._grow(12)
    enc.capacity = 16
    files = enc.encode(torch.from_numpy(frames).to(dev))
    assert enc.reruns > before and enc.capacity >= sum(len(f) for f in files)
    check_files(files, [expected(k, H, W, 5, 100, s, 0, 3, True) for k in KINDS], "after growing")
    check_round_trip(DeviceJpegDecoder(W, H, device=dev, max_frames=4), files)


def test_start_capacity_is_sized_for_the_sampling(dev):
    from truely_amd.jpeg import DeviceJpeg
    H, W = 360, 640
    caps = []
    frames = torch.from_numpy(np.stack([make_frame("gradient", H, W), make_frame("saturated", H, W)])).to(dev)
    for s in SAMPLINGS:
        enc = DeviceJpeg(W, H, 80, device=dev, max_frames=2, subsampling=s, restart_rows=1)
        caps.append(enc.capacity)
        enc.encode(frames)
        assert enc.reruns == 0
    per_px = [(c / 2 - 4096 - 700) / (H * W) for c in caps]                 # a third of a byte per sample: 3, 2, 1.5 samples per pixel
    assert 0.99 < per_px[0] < 1.01 and 0.66 < per_px[1] < 0.68 and 0.49 < per_px[2] < 0.51


def test_defaults_are_unchanged(dev):
    """trl_jpeg_create_ex with default options gives trl_jpeg_create's bytes, which are still Pillow's subsampling=2 files."""
    lib = _lib.load()
    for (W, H) in ((17, 15), (100, 75), (320, 180)):
        frames = np.stack([make_frame(k, H, W) for k in KINDS])
        d = torch.from_numpy(frames).to(dev)
        outs = []
        for make in ("create", "create_ex"):
            h = C.c_void_p()
            if make == "create":
                _lib.check(lib.trl_jpeg_create(dev.index or 0, H, W, 80, 4, C.byref(h)))
            else:
                h = _create_ex(dev, H, W, 80, 2, 0, 0, False, 4)
            out = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
            sizes = _raw_encode(h, d, 4, H * W * 3, out, out.numel(), 0)
            torch.cuda.synchronize()
            lib.trl_jpeg_destroy(h)
            outs.append(out.cpu().numpy()[:sizes.sum()].tobytes())
        assert outs[0] == outs[1] == b"".join(pillow_jpeg(f, 80) for f in frames)


def test_create_ex_refuses_bad_options(dev):
    from truely_amd.jpeg import DeviceJpeg
    lib = _lib.load()
    for s, rr, rb in ((-1, 0, 0), (3, 0, 0), (2, -1, 0), (2, 0, -1), (0, 0, 65536)):
        h = C.c_void_p()
        o = _lib.TrlJpegOptions(80, s, rr, rb, 0)
        assert lib.trl_jpeg_create_ex(dev.index or 0, 48, 64, C.byref(o), 4, C.byref(h)) == -1 and not h.value
        assert b"trl_jpeg_create_ex" in lib.trl_last_error()
    h = C.c_void_p()
    assert lib.trl_jpeg_create_ex(dev.index or 0, 48, 64, None, 4, C.byref(h)) == -1 and not h.value
    with pytest.raises(_lib.TrlError):
        DeviceJpeg(64, 48, device=dev, subsampling=4)


# ---- run(): the options reach whichever encoder writes ---------------------------------------------------------------------------
def _run_capture(tmp_path, monkeypatch, src, tag):
    """run() -> (the frames handed to the writer, the AVI's chunks)."""
    from truely_amd import model, video_io
    seen = []
    w0, wd0 = video_io.AviMjpegWriter.write, video_io.AviMjpegWriter.write_device

    def write(self, frame):
        seen.append(np.array(frame, np.uint8, copy=True))
        w0(self, frame)

    def write_device(self, frames):
        seen.extend(frames.cpu().numpy())
        wd0(self, frames)
    monkeypatch.setattr(video_io.AviMjpegWriter, "write", write)
    monkeypatch.setattr(video_io.AviMjpegWriter, "write_device", write_device)
    dst = str(tmp_path / f"{tag}.avi")
    model.run(src, dst)
    monkeypatch.setattr(video_io.AviMjpegWriter, "write", w0)
    monkeypatch.setattr(video_io.AviMjpegWriter, "write_device", wd0)
    r = video_io.AviMjpegReader(dst)
    chunks = []
    for off, size in r.frames:
        r.f.seek(off)
        chunks.append(r.f.read(size))
    r.release()
    return seen, chunks


def test_run_passes_the_environment_options_to_both_encoders(engine, tmp_path, monkeypatch):
    from truely_amd import engine as eng_mod, video_io
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() writes H.264 through cv2")
    monkeypatch.setattr(eng_mod, "_default", engine)
    N, H, W = 12, 64, 96
    src = str(tmp_path / "s.trlv")
    video_io.write_raw(src, truely_amd.synthetic.synthetic_frames(N, H, W, seed=1), 30)
    monkeypatch.setenv("TRUELY_JPEG_SUBSAMPLING", "444")
    monkeypatch.setenv("TRUELY_JPEG_RESTART_ROWS", "1")
    monkeypatch.setenv("TRUELY_JPEG_OPTIMIZE", "1")
    files = {}
    for enc in ("device", "pillow"):
        monkeypatch.setenv("TRUELY_JPEG", enc)
        seen, chunks = _run_capture(tmp_path, monkeypatch, src, enc)
        assert len(seen) == len(chunks) == N
        assert chunks == [R.pillow(f, 80, 0, 1, 0, True) for f in seen], enc
        files[enc] = chunks
    assert files["device"] == files["pillow"]
    assert b"\xff\xdd\x00\x04\x00\x0c" in files["device"][0]                # DRI: one row of 12 MCUs of 8 x 8
    for v in ("TRUELY_JPEG_SUBSAMPLING", "TRUELY_JPEG_RESTART_ROWS", "TRUELY_JPEG_OPTIMIZE"):
        monkeypatch.delenv(v)
    monkeypatch.setenv("TRUELY_JPEG", "device")
    seen, chunks = _run_capture(tmp_path, monkeypatch, src, "plain")
    assert chunks == [pillow_jpeg(f, 80) for f in seen]     # none set: the file of the writer without options
