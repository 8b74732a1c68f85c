"""GPU tests of the Motion-JPEG decoder (csrc/trl_jpegd.hip) through jpeg.DeviceJpegDecoder, video_io and run(): every frame it
decodes equals Pillow's byte for byte, nothing is left to the fallback for files inside its scope, nothing outside a decoded
frame is written, and run() on Motion-JPEG AVI input gives the scores and output bytes of the Pillow path."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpegd_cases as cases
import jpegd_ref
import truely_amd
from truely_amd import _lib, jpeg, video_io

pytestmark = pytest.mark.gpu


def decode_all(files, W, H, max_frames=32):
    dec = jpeg.DeviceJpegDecoder(W, H, max_frames=max_frames)
    frames, status = dec.decode(files)
    torch.cuda.synchronize()
    return frames.cpu().numpy(), status


def assert_equals_pillow(files, frames, status, what=""):
    assert (status == 0).all(), f"{what}: statuses {status.tolist()} (every file is inside the decoder's scope)"
    for k, data in enumerate(files):
        assert np.array_equal(frames[k], cases.pillow_bgr(data)), f"{what}: frame {k}"


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("size", cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_pillow(size, sub):
    """The size x subsampling x quality / content / option table of the CPU test, one batch per cell."""
    W, H = size
    table = cases.good_files(W, H, sub)
    files = [d for _, d in table]
    frames, status = decode_all(files, W, H)
    assert (status == 0).all(), [(table[k][0], int(s)) for k, s in enumerate(status) if s]
    for k, (label, data) in enumerate(table):
        assert np.array_equal(frames[k], cases.pillow_bgr(data)), f"{W}x{H} subsampling {sub} {label}"


def mixed_files(n, W=64, H=48):
    """n files of one size: content, quality, subsampling, table sets and restart intervals all vary."""
    out = []
    for k in range(n):
        kw = [{}, {"optimize": True}, {"restart_marker_blocks": 1 + k % 5}, {"restart_marker_rows": 1}][k % 4]
        out.append(cases.encode(cases.content(cases.CONTENT[k % 4], W, H, k), cases.QUALITIES[(k // 4) % 4], k % 3, **kw))
    return out


@pytest.mark.parametrize("n", [1, 2, 33, 70])
def test_batch_sizes_cross_max_frames(n):
    files = mixed_files(n)
    frames, status = decode_all(files, 64, 48, max_frames=32)
    assert_equals_pillow(files, frames, status, f"batch of {n}")


def test_batch_mixes_table_sets():
    files = [cases.encode(cases.content("noise", 64, 48, k), 50 + 5 * (k % 3), 2, optimize=bool(k & 1)) for k in range(12)]
    frames, status = decode_all(files, 64, 48)
    assert_equals_pillow(files, frames, status, "optimised and standard tables")


def test_batch_mixes_restart_intervals():
    rgb = [cases.content("noise", 131, 97, k) for k in range(8)]
    kws = [{}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}, {"restart_marker_blocks": 7}, {}, {"restart_marker_rows": 2},
           {"restart_marker_blocks": 2}, {"restart_marker_blocks": 1000}]
    files = [cases.encode(a, 80, 2, **kw) for a, kw in zip(rgb, kws)]
    frames, status = decode_all(files, 131, 97)
    assert_equals_pillow(files, frames, status, "restart intervals")


@pytest.mark.parametrize("size", [(640, 360), (1280, 720)], ids=["360p", "720p"])
def test_video_sizes(size):
    W, H = size
    clip = truely_amd.synthetic.synthetic_frames(4, H, W, seed=5)
    files = [cases.encode(np.ascontiguousarray(f[:, :, ::-1]), 80, 2) for f in clip]
    files[3] = cases.encode(np.ascontiguousarray(clip[3][:, :, ::-1]), 80, 1, restart_marker_rows=1)
    frames, status = decode_all(files, W, H)
    assert_equals_pillow(files, frames, status, f"{W}x{H}")


def raw_decode(dec, files, out, stride, n=None, offsets=None, sizes=None, arena_bytes=None):
    """trl_jpegd_decode itself on a packed arena -> (return code, statuses)."""
    sizes = np.array([len(f) for f in files], np.int64) if sizes is None else np.asarray(sizes, np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])[:-1]]).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
    blob = b"".join(files)
    host = torch.frombuffer(bytearray(blob + bytes(64)), dtype=torch.uint8)
    dev = host.cuda()
    n = len(files) if n is None else n
    status = np.full(max(n, 1), -7, np.int32)
    rc = dec.lib.trl_jpegd_decode(dec.h, C.c_void_p(host.data_ptr()), C.c_void_p(dev.data_ptr()), offsets.ctypes.data_as(C.c_void_p),
                                  sizes.ctypes.data_as(C.c_void_p), n, C.c_void_p(out.data_ptr()), stride, status.ctypes.data_as(C.c_void_p),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, status


def test_sentinels_and_damaged_files_in_a_batch():
    """Good frames between unsupported and damaged ones, written into a strided, poisoned output: the good frames equal Pillow,
    the others report 1 or 2 exactly as the CPU build of the same function did (tests/test_jpegd_cpu.py runs every one of these
    streams first) and keep their poison, as do the bytes between frames and past the last one.  These are the OUTPUT sentinels:
    the decoder owns its workspace, which has no guard region a caller can look at (its bounds are what the sanitized CPU build
    of the same decode function checks)."""
    W, H = 64, 48
    bad = cases.damaged_files(W, H) + cases.unsupported_files()
    good = mixed_files(len(bad) + 1, W, H)
    files, kinds = [], []
    for k, (label, data) in enumerate(bad):
        files += [good[k], data]
        kinds += [None, label]
    files.append(good[-1]); kinds.append(None)
    n = len(files)
    dec = jpeg.DeviceJpegDecoder(W, H, max_frames=n)
    fb, gap = H * W * 3, 96
    out = torch.full((n * (fb + gap) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, status = raw_decode(dec, files, out, fb + gap)
    assert rc == 0, _lib.load().trl_last_error()
    got = out.cpu().numpy()
    seen = set()
    for k in range(n):
        frame = got[k * (fb + gap):k * (fb + gap) + fb].reshape(H, W, 3)
        assert (got[k * (fb + gap) + fb:(k + 1) * (fb + gap)] == 0xA5).all(), f"gap after frame {k}"
        if kinds[k] is None:
            assert status[k] == 0
            assert np.array_equal(frame, cases.pillow_bgr(files[k])), f"good frame {k}"
            continue
        try:
            info = jpegd_ref.parse(files[k])
            want, ref = (0, jpegd_ref.decode(files[k])) if (info["W"], info["H"]) == (W, H) else (1, None)    # another size: not attempted
        except jpegd_ref.Unsupported:
            want = 1
        except jpegd_ref.Irregular:
            want = 2
        assert status[k] == want, (kinds[k], int(status[k]), want)
        seen.add(int(status[k]))
        if want == 0:
            assert np.array_equal(frame, ref), kinds[k]
            assert np.array_equal(frame, cases.pillow_bgr(files[k])), f"{kinds[k]}: status 0 but not Pillow's bytes"
        else:
            assert (frame == 0xA5).all(), f"{kinds[k]}: status {status[k]} but bytes were written"
    assert (got[n * (fb + gap):] == 0xA5).all()
    assert {1, 2} <= seen


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("size", cases.SYN_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_table(size, sub):
    """Streams no encoder writes from pixels (edited headers, hand-coded scans, coefficients up to and past the IDCT gate), one call
    per size and subsampling with more table sets than the call's cache of 16 holds and a gated frame between good ones wherever
    there is one: a "pillow" frame has status 0 and Pillow's bytes, a "gated" frame status 2 and its poison, as have the gaps."""
    W, H = size
    table = cases.synthetic_files(W, H, sub)
    good, gated = [r for r in table if r[2] == "pillow"], [r for r in table if r[2] == "gated"]
    assert len(good) > len(gated) >= 40
    rows = [good[0]]
    for k, g in enumerate(gated):
        rows += [g, good[1 + k]]
    rows += good[1 + len(gated):]
    files = [d for _, d, _ in rows]
    assert len({cases.table_set(d) for d in files}) > 16
    n = len(files)
    dec = jpeg.DeviceJpegDecoder(W, H, max_frames=n)
    fb, gap = H * W * 3, 96
    out = torch.full((n * (fb + gap) + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, status = raw_decode(dec, files, out, fb + gap)
    assert rc == 0, _lib.load().trl_last_error()
    got = out.cpu().numpy()
    wrong = [(label, expect, int(st)) for (label, _, expect), st in zip(rows, status) if st != (0 if expect == "pillow" else 2)]
    assert not wrong, wrong
    for k, (label, data, expect) in enumerate(rows):
        frame = got[k * (fb + gap):k * (fb + gap) + fb].reshape(H, W, 3)
        assert (got[k * (fb + gap) + fb:(k + 1) * (fb + gap)] == 0xA5).all(), f"gap after frame {k}"
        if expect == "pillow":
            assert np.array_equal(frame, cases.pillow_bgr(data)), label
        else:
            assert (frame == 0xA5).all(), f"{label}: status 2 but bytes were written"
    assert (got[n * (fb + gap):] == 0xA5).all()


def test_refusals_write_nothing():
    W, H = 64, 48
    files = mixed_files(4, W, H)
    dec = jpeg.DeviceJpegDecoder(W, H, max_frames=3)
    fb = H * W * 3
    out = torch.full((8 * fb,), 0x5A, dtype=torch.uint8, device="cuda")
    total = sum(len(f) for f in files)
    for kw in (dict(n=4),                                                    # n > max_frames
               dict(n=2, stride=fb - 1),                                     # frames would overlap
               dict(n=2, offsets=[0, dec.max_bytes - 10]),                   # a file that ends outside the buffer
               dict(n=2, sizes=[len(files[0]), -1]),
               dict(n=2, offsets=[-1, 0])):
        stride = kw.pop("stride", fb)
        rc, status = raw_decode(dec, files, out, stride, **kw)
        assert rc == -1, kw
        assert (status == -7).all()
        assert (out.cpu().numpy() == 0x5A).all()
    rc, status = raw_decode(dec, files[:3], out, fb)
    assert rc == 0 and (status[:3] == 0).all() and total > 0


def test_side_stream_repeats_and_poisoned_workspace():
    """One decoder, three calls on a side stream with a different batch each, its whole device workspace filled with 0xCD, 0xFF (NaN where
    read as floats) or 0x7F before each call: nothing of an earlier call or of the
    poison shows."""
    W, H = 131, 97
    dec = jpeg.DeviceJpegDecoder(W, H, max_frames=8)
    side = torch.cuda.Stream()
    for rep in range(3):
        files = [cases.encode(cases.content(cases.CONTENT[(k + rep) % 4], W, H, 10 * rep + k), 80, (k + rep) % 3,
                              **([{}, {"restart_marker_rows": 1}][k & 1])) for k in range(3 + 2 * rep)]
        assert dec.lib.trl_jpegd_debug_poison(dec.h, [0xCD, 0xFF, 0x7F][rep]) == 0       # 0xFF..: NaN where read as floats
        sizes = np.array([len(f) for f in files], np.int64)
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        host = torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8).pin_memory()
        out = torch.full((len(files), H, W, 3), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            dev = host.to("cuda", non_blocking=True)
            status = dec.decode_into(host, dev, offsets, sizes, out)
        side.synchronize()
        assert_equals_pillow(files, out.cpu().numpy(), status, f"call {rep}")


def test_avi_round_trip(tmp_path):
    """AviMjpegWriter -> DeviceJpegDecoder: the Pillow-encoded and the device-encoded AVI decode to the frames read() yields."""
    clip = truely_amd.synthetic.synthetic_frames(6, 97, 131, seed=2)
    for encoder, device in (("pillow", None), ("device", torch.device("cuda", 0))):
        path = str(tmp_path / f"{encoder}.avi")
        w = video_io.AviMjpegWriter(path, 30, (131, 97), device=device)
        for f in clip:
            w.write(f)
        w.release()
        r = video_io.AviMjpegReader(path)
        chunks = [r.read_chunk(i) for i in range(r.n)]
        want = []
        while True:
            ok, f = r.read()
            if not ok:
                break
            want.append(f)
        r.release()
        assert len(want) == len(clip) == len(chunks)
        frames, status = decode_all(chunks, 131, 97)
        assert (status == 0).all()
        assert np.array_equal(frames, np.stack(want)), encoder


# ---- run() on Motion-JPEG AVI input ----------------------------------------------------------------------------------------------
def write_avi(path, frames, fps=30, edit=None):
    """A Motion-JPEG AVI of these BGR frames with Pillow's encoder; edit(k, file) -> file replaces frame k's chunk."""
    H, W = frames.shape[1:3]
    w = video_io.AviMjpegWriter(path, fps, (W, H), quality=92)
    for k, f in enumerate(frames):
        data = w.encode_frame(f)
        w.append_encoded(edit(k, data, f) if edit else data)
    w.release()


class RunProbe:
    """Runs model.run with one environment, recording what the test asserts on: the score, the output's bytes, the final frame
    count handed to the drift pass, which chunks were read by position, and every large host -> device copy."""

    def __init__(self, engine, monkeypatch, tmp_path):
        from truely_amd import engine as eng_mod
        self.engine, self.mp, self.tmp = engine, monkeypatch, tmp_path
        monkeypatch.setattr(eng_mod, "_default", engine)

    def __call__(self, src, tag, write_out, mjpeg):
        from truely_amd import model
        from truely_amd.engine import Engine
        mp = self.mp
        mp.setenv("TRUELY_WRITE_OUTPUT", "1" if write_out else "0")
        mp.setenv("TRUELY_MJPEG", mjpeg)
        rec = dict(reads=[], h2d=[], frame_counts=[])
        H, W = self.hw
        read_chunk, drift_update, copy_ = video_io.AviMjpegReader.read_chunk, Engine.drift_update, torch.Tensor.copy_
        to, cuda = torch.Tensor.to, torch.Tensor.cuda

        def spy_read(rd, i, dst=None):
            rec["reads"].append((int(i), dst is not None))
            return read_chunk(rd, i, dst)

        def spy_drift(eng, state, emb, valid, frame_count, *a, **kw):
            rec["frame_counts"].append(int(frame_count))
            return drift_update(eng, state, emb, valid, frame_count, *a, **kw)

        def spy_copy(dst, src, *a, **kw):
            if dst.is_cuda and not src.is_cuda and src.numel() >= H * W * 3:
                rec["h2d"].append(tuple(src.shape))
            return copy_(dst, src, *a, **kw)

        def spy_move(orig):                                 # .to(device) / .cuda() of a host tensor are uploads too
            def moved(src, *a, **kw):
                out = orig(src, *a, **kw)
                if out.is_cuda and not src.is_cuda and src.numel() >= H * W * 3:
                    rec["h2d"].append(tuple(src.shape))
                return out
            return moved

        with mp.context() as m:
            m.setattr(torch.Tensor, "to", spy_move(to))
            m.setattr(torch.Tensor, "cuda", spy_move(cuda))
            m.setattr(video_io.AviMjpegReader, "read_chunk", spy_read)
            m.setattr(Engine, "drift_update", spy_drift)
            m.setattr(torch.Tensor, "copy_", spy_copy)
            dst = str(self.tmp / f"{tag}_output.mp4")
            rec["score"] = model.run(src, dst)
        rec["bytes"] = open(dst, "rb").read() if write_out else None
        rec["frame_count"] = rec["frame_counts"][-1] if rec["frame_counts"] else 0
        return rec


@pytest.fixture
def probe(engine, monkeypatch, tmp_path):
    if video_io.cv2 is not None:
        pytest.skip("OpenCV present: run() takes the cv2 path for .avi")
    return RunProbe(engine, monkeypatch, tmp_path)


def compare_paths(probe, src, write_out, fallback_frames=0, sampled_only=None):
    dev = probe(src, f"dev{int(write_out)}", write_out, "device")
    pil = probe(src, f"pil{int(write_out)}", write_out, "pillow")
    assert dev["score"] == pil["score"]
    assert dev["frame_count"] == pil["frame_count"]
    assert dev["bytes"] == pil["bytes"]
    assert not pil["reads"], "TRUELY_MJPEG=pillow is the sequential path: no positioned reads"
    H, W = probe.hw
    # on the device path what travels host -> device is the compressed arena (1-D bytes) and the fallback frames, nothing else
    assert [s for s in dev["h2d"] if len(s) != 1] == [(H, W, 3)] * fallback_frames, dev["h2d"]
    return dev, pil


@pytest.mark.parametrize("size", [(320, 180), (131, 97)], ids=["320x180", "odd"])
def test_run_on_avi_equals_pillow_path(probe, tmp_path, size):
    W, H = size
    probe.hw = (H, W)
    clip = truely_amd.synthetic.synthetic_frames(36, H, W, seed=3)
    src = str(tmp_path / "clip.avi")
    write_avi(src, clip)
    dev, _ = compare_paths(probe, src, write_out=False)
    # output skipped: only the sampled frames' chunks are read (30 fps: every 4th), each once, into the arena
    assert sorted(dev["reads"]) == [(i, True) for i in range(0, 36, 4)]
    assert dev["frame_count"] == 36
    dev, _ = compare_paths(probe, src, write_out=True)
    assert sorted(dev["reads"]) == [(i, True) for i in range(36)]
    assert dev["bytes"] is not None and len(dev["bytes"]) > 0


def test_run_progressive_frame_goes_through_the_fallback(probe, tmp_path):
    H, W = 180, 320
    probe.hw = (H, W)
    clip = truely_amd.synthetic.synthetic_frames(36, H, W, seed=3)

    def edit(k, data, f):
        if k != 16:
            return data
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(b, "JPEG", quality=92, progressive=True)
        return b.getvalue()
    src = str(tmp_path / "clip.avi")
    write_avi(src, clip, edit=edit)
    for write_out in (False, True):
        dev, _ = compare_paths(probe, src, write_out, fallback_frames=1)
        assert (16, False) in dev["reads"]                 # the fallback read that chunk again, for Pillow
        assert dev["frame_count"] == 36


def test_run_gated_frame_goes_through_the_fallback(probe, tmp_path):
    """A sampled frame whose quantisers were multiplied by 16: regular baseline JPEG inside the former int16 gate, with outputs far
    outside what the IDCT's range limit leaves alone.  The device reports it irregular and Pillow decides what it is."""
    H, W = 180, 320
    probe.hw = (H, W)
    clip = truely_amd.synthetic.synthetic_frames(36, H, W, seed=3)

    def edit(k, data, f):
        if k != 16:
            return data
        out = cases.rescaled(data, lambda t, i, q: 16 * q)
        assert cases.gate_expectation(out) == "gated" and not cases.former_gate_trips(out)
        return out
    src = str(tmp_path / "clip.avi")
    write_avi(src, clip, edit=edit)
    for write_out in (False, True):
        dev, _ = compare_paths(probe, src, write_out, fallback_frames=1)
        assert (16, False) in dev["reads"]                 # the fallback read that chunk again, for Pillow
        assert dev["frame_count"] == 36


def test_run_truncated_frame_ends_the_clip_where_pillow_ends_it(probe, tmp_path, capsys):
    H, W = 180, 320
    probe.hw = (H, W)
    clip = truely_amd.synthetic.synthetic_frames(36, H, W, seed=3)
    src = str(tmp_path / "clip.avi")
    write_avi(src, clip, edit=lambda k, data, f: data[:len(data) // 2] if k == 20 else data)     # frame 20 is a sampled frame
    for write_out in (False, True):
        capsys.readouterr()
        dev, pil = compare_paths(probe, src, write_out)
        assert dev["frame_count"] == pil["frame_count"] == 20
        text = capsys.readouterr().out
        assert text.count("Warning: frame 20 of 36 cannot be decoded") == 2      # today's warning, once per path
