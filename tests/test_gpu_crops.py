"""The three face-crop kernels (k_crop_resize80, k_crop_area_std, k_crop_aligned) on the case table of tests/crop_ref.py.

Every embedding passes through one of them.  Each call here is checked against the plain-numpy reference (crop_ref.py), against
the C oracle, and -- where the operation approximates exact arithmetic -- against the float64 form within the bound derived in
crop_ref.py (tests/test_crops_cpu.py proves the three agree with each other on this table without a GPU).

How a wrong read becomes a wrong result: frames hold random bytes (or a 1-px checkerboard, all 0, all 255), every rectangle size
sits at all four frame corners and once inside, a batch gives every frame its own rectangle, the last frame's rectangle touches
its bottom-right corner, and the frames are the head of a device buffer whose tail is 0xFF -- a tap one pixel or one row too far
lands on other content of the frame, on the next frame, or on the 0xFF tail, never out of the allocation.  One row in five is
invalid with a garbage rectangle and must come back exactly zero; outputs are pre-filled with NaN, so an element the kernel does
not write fails every comparison.  All comparisons cover whole tensors.
"""
import numpy as np
import pytest
import torch

import truely_amd
import crop_ref as R

pytestmark = pytest.mark.gpu

I32 = np.iinfo(np.int32)
GARBAGE = ((-5, -7, 3, 9), (50, 40, 10, 20), (10 ** 6, 10 ** 6, 2 * 10 ** 6, 3 * 10 ** 6), (I32.min, I32.min, I32.max, I32.max),
           (I32.max, I32.max, I32.min, I32.min), (0, 0, 0, 0))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _device_frames(engine, base, n):
    """n frames on the device, frame i = base[i % len(base)], as the head of a larger buffer whose tail is 0xFF.  Returns the
    (n, H, W, 3) view (the engine must pass it on as it is) and the buffer."""
    k, H, W, _ = base.shape
    fb = H * W * 3
    buf = torch.empty(n * fb + max(4096, 2 * W * 3 + 64), dtype=torch.uint8, device=engine.device)
    buf[n * fb:] = 0xFF
    frames = buf[:n * fb].view(n, H, W, 3)
    b = _t(base).to(engine.device)
    if k == n:
        frames.copy_(b)
    else:
        for j in range(min(k, n)):
            frames[j::k] = b[j]
    assert engine._frames(frames).data_ptr() == buf.data_ptr()
    return frames, buf


def _rows(H, W, n, start):
    """Rectangles and valid flags of an n-frame batch: valid rows walk the table from entry `start`, one row in five is invalid
    with a garbage rectangle, the last row is valid and touches the frame's bottom-right corner."""
    table = R.rect_table(H, W)
    corner = [r for r in table if r[2] == W and r[3] == H]
    rect, valid = np.zeros((n, 4), np.int32), np.ones(n, np.uint8)
    t = start
    for i in range(n):
        if i == n - 1:
            rect[i] = corner[start % len(corner)]
        elif i % 5 == 3:
            rect[i], valid[i] = GARBAGE[(i // 5) % len(GARBAGE)], 0
        else:
            rect[i] = table[t % len(table)]
            t += 1
    return rect, valid, table


def _nan(engine, n, S):
    return torch.full((n, S, S, 3), float("nan"), dtype=torch.float32, device=engine.device)


def _check_rect_crops(engine, oracle, kind, base, n, rect, valid, area_S=160):
    """Both rectangle kernels on one batch.  Flat content has its answer in closed form (test_crops_cpu.py: the references give
    it at every rectangle of the table); random and checkerboard content go through the references and the oracle."""
    frames, buf = _device_frames(engine, base, n)
    H, W = base.shape[1:3]
    got80 = engine.crop_resize(frames, _t(rect), _t(valid), out=_nan(engine, n, 80)).cpu().numpy()
    area = {rgb: engine.crop_area(frames, _t(rect), _t(valid), S=area_S, rgb=rgb, out=_nan(engine, n, area_S)).cpu().numpy() for rgb in (False, True)}
    del frames, buf
    bound = R.resize_fixed_point_bound()
    for i in range(n):
        tag = (kind, H, W, n, i, rect[i].tolist())
        if not valid[i]:
            assert not got80[i].any() and not area[False][i].any() and not area[True][i].any(), tag     # exactly zero: NaN is "any"
            continue
        img = base[i % len(base)]
        x0, y0, x1, y1 = (int(v) for v in rect[i])
        if kind in ("zeros", "ones"):
            flat = 0 if kind == "zeros" else 255
            assert (got80[i] == np.float32(flat) / np.float32(255)).all(), tag
            for rgb in (False, True):
                assert (area[rgb][i] == (np.float32(flat) - np.float32(127.5)) / np.float32(128)).all(), tag
            continue
        ref = R.resize_linear_u8_int(img, y0, y1, x0, x1)
        assert np.array_equal(got80[i], ref.astype(np.float32) / np.float32(255.0)), tag                 # to_tensor's division
        assert np.array_equal(ref, oracle.resize_linear_u8(img, y0, y1, x0, x1)), tag
        lv = np.rint(got80[i].astype(np.float64) * 255.0)      # the grey levels the device produced (== ref, by the equality above)
        assert np.abs(lv - R.resize_linear_f64(img, y0, y1, x0, x1)).max() <= bound, tag
        a = (R.crop_area_u8(img, x0, y0, x1, y1, area_S).astype(np.float32) - np.float32(127.5)) / np.float32(128.0)
        assert np.array_equal(area[False][i], a), tag
        assert np.array_equal(area[True][i], a[..., ::-1]), tag
        for rgb in (False, True):
            assert np.array_equal(area[rgb][i], oracle.crop_area_std(img, (x0, y0, x1, y1), S=area_S, rgb=rgb)), tag


@pytest.mark.parametrize("H,W", R.GEOMETRIES)
def test_rect_crops_on_the_table(engine, oracle, H, W):
    """k_crop_resize80 and k_crop_area_std (S = 160, rgb 0 and 1): batches of 256 frames with a different rectangle per frame for
    each content -- the valid rows of one batch cover the whole table of the geometry -- and single-frame calls."""
    fb = H * W * 3
    for ci, kind in enumerate(R.CONTENTS):
        n = 256
        base = R.content_frames(kind, n if n * fb <= (64 << 20) else 3, H, W, seed=77 * ci + H)
        rect, valid, table = _rows(H, W, n, start=ci * 17)
        used = {tuple(r) for r, v in zip(rect.tolist(), valid) if v}
        assert used >= set(table) and (valid == 0).sum() >= n // 5 - 1 and valid[-1] and tuple(rect[-1][2:]) == (W, H)
        _check_rect_crops(engine, oracle, kind, base, n, rect, valid)
    base = R.content_frames("random", 1, H, W, seed=H + W)
    table = R.rect_table(H, W)
    for r in (table[0], table[len(table) // 2], (W - 1, H - 1, W, H), (0, 0, W, H)):
        _check_rect_crops(engine, oracle, "random", base, 1, np.array([r], np.int32), np.ones(1, np.uint8))
    _check_rect_crops(engine, oracle, "random", base, 1, np.array([GARBAGE[0]], np.int32), np.zeros(1, np.uint8))


def test_rect_crops_thousand_frames(engine, oracle):
    """One batch of 1000 odd-pitch frames (97 x 131: 393 B rows, 38121 B frames -- three frames in four start off a 4 B boundary), all distinct;
    the area crop at S = 112 here."""
    H, W, n = 97, 131, 1000
    rect, valid, _ = _rows(H, W, n, start=5)
    _check_rect_crops(engine, oracle, "random", R.content_frames("random", n, H, W, seed=9), n, rect, valid, area_S=112)
    _check_rect_crops(engine, oracle, "checker", R.content_frames("checker", n, H, W, seed=0), n, rect, valid, area_S=112)


@pytest.mark.parametrize("H,W", R.GEOMETRIES)
def test_aligned_crop_on_every_geometry(engine, oracle, H, W):
    """k_crop_aligned on crop_ref.landmark_sets (the sets of test_aligned_crop_kernel_bit_exact re-placed for each frame size,
    plus corner-centred sets, single points on and between integer coordinates at every edge, a NaN coordinate) at S = 160, 112
    and 1, rgb on and off, every third row invalid, each row on its own frame: device == oracle bit for bit (NaN where the
    oracle has NaN), and within crop_ref.aligned_f32_bound() of the float64 warp."""
    sets = R.landmark_sets(H, W)
    rows = []                                            # (name, pts, valid)
    for j, (name, pts) in enumerate(sets):
        rows.append((name, pts, 1))
        if j % 2 == 1:
            rows.append(("invalid", np.full(10, np.nan if j % 4 == 1 else 1e30, np.float32), 0))
    rows.append(("corner 11", dict(sets)["corner 11"], 1))          # the last frame samples around its bottom-right corner
    n = len(rows)
    base = R.content_frames("random", n if n * H * W * 3 <= (64 << 20) else 3, H, W, seed=H ^ W)
    frames, buf = _device_frames(engine, base, n)
    pts, valid = _t(np.stack([r[1] for r in rows])), _t(np.array([r[2] for r in rows], np.uint8))
    bound, seen_nan = R.aligned_f32_bound(), 0
    for S in (160, 112, 1):
        for rgb in (True, False):
            got = engine.crop_aligned(frames, pts, valid, S=S, rgb=rgb, out=_nan(engine, n, S)).cpu().numpy()
            for i, (name, p, v) in enumerate(rows):
                tag = (H, W, S, rgb, i, name)
                if not v:
                    assert not got[i].any(), tag
                    continue
                img = base[i % len(base)]
                ref = oracle.crop_aligned(img, p, S=S, rgb=rgb)
                assert np.array_equal(got[i], ref, equal_nan=True), tag
                if name == "nan":
                    assert np.isnan(got[i]).all(), tag
                    seen_nan += 1
                    continue
                assert np.abs(got[i].astype(np.float64) - R.crop_aligned_f64(img, p, S=S, rgb=rgb)).max() <= bound, tag
    assert seen_nan == 6


def _whole_path_frames():
    """360 x 640 frames for the whole path: synthetic faces (the third one's box starts above the frame), the same frames rolled
    so that the box crosses the bottom and the left border, flat frames (no detection) and noise."""
    H, W = 360, 640
    fr = truely_amd.synthetic.synthetic_frames(4, H, W, seed=11)
    c = [fr[0], fr[1], fr[2], fr[3], np.roll(fr[0], W - 290, 1), np.roll(fr[3], H - 150, 0), np.roll(fr[1], -230, 1),
         np.roll(fr[1], (-100, -240), (0, 1)), np.full((H, W, 3), 128, np.uint8), np.zeros((H, W, 3), np.uint8),
         np.full((H, W, 3), 255, np.uint8), np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)]
    return np.stack(c)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_detect_crop_is_the_hook_on_its_own_rect(blob, oracle, mode):
    """Engine(embed_mode).detect_crop: the faces it returns are the mode's crop kernel applied to the rect / valid it returns (mode
    3: to the first landmark set of mtcnn_detect_landmarks), bit for bit; faceless frames give zero crops.  The batch must hold
    clamped rectangles and invalid frames, or the test proves nothing; rect / valid are the oracle's."""
    from truely_amd.engine import Engine
    eng = Engine(blob, embed_mode=mode)
    try:
        _check_whole_path(eng, oracle, mode)
    finally:
        eng.close()


def _check_whole_path(eng, oracle, mode):
    fr = _whole_path_frames()
    n, H, W, _ = fr.shape
    out = eng.detect_crop(fr)
    S = 80 if mode == 0 else 160
    faces, rect, valid, box = out["faces"].cpu().numpy(), out["rect"].cpu().numpy(), out["valid"].cpu().numpy(), out["box"].cpu().numpy()
    assert faces.shape == (n, S, S, 3)
    clamped = valid.astype(bool) & ((box[:, 0] < 0) | (box[:, 1] < 0) | (box[:, 2] > W) | (box[:, 3] > H))
    assert clamped.sum() >= 1 and (valid == 0).sum() >= 1 and valid.sum() >= 4, (valid, box)
    assert ((rect[clamped, 0] == 0) | (rect[clamped, 1] == 0) | (rect[clamped, 2] == W) | (rect[clamped, 3] == H)).all()
    ref = oracle.detect_embed(fr) if mode == 0 else oracle.detect_embed_mode(fr, mode)
    assert np.array_equal(valid, ref["valid"]) and np.array_equal(rect, ref["rect"])
    if mode == 0:
        hook = eng.crop_resize(fr, out["rect"], out["valid"], out=_nan(eng, n, S))
    elif mode == 3:
        pts = eng.mtcnn_detect(fr, landmarks=True)[3][:, 0, :].contiguous()
        hook = eng.crop_aligned(fr, pts, out["valid"], S=S, rgb=True, out=_nan(eng, n, S))
    else:
        hook = eng.crop_area(fr, out["rect"], out["valid"], S=S, rgb=mode == 2, out=_nan(eng, n, S))
    assert np.array_equal(faces, hook.cpu().numpy())
    assert not faces[valid == 0].any() and all(faces[i].any() for i in np.flatnonzero(valid))
    for i in np.flatnonzero(valid):                      # and the hook's crop is the reference's crop of that rectangle
        x0, y0, x1, y1 = (int(v) for v in rect[i])
        if mode == 0:
            assert np.array_equal(faces[i], R.resize_linear_u8_int(fr[i], y0, y1, x0, x1).astype(np.float32) / np.float32(255.0)), i
        elif mode != 3:
            assert np.array_equal(faces[i], R.crop_area_std(fr[i], x0, y0, x1, y1, S, rgb=mode == 2)), i


def test_crop_hook_arguments(engine):
    """The three hooks refuse what their kernels cannot take, before any launch: null pointers, n < 1, H or W < 1, S outside
    1..4096, and -- for the two kernels that carry the frame index in grid y -- n > 65535.  Shapes that do not match the frames
    are refused by the Python front-end."""
    import ctypes as C
    from truely_amd._lib import TrlError
    lib, h, dev = engine.lib, engine._h, engine.device
    fr = torch.zeros((2, 4, 5, 3), dtype=torch.uint8, device=dev)
    rect = torch.tensor([[0, 0, 5, 4], [1, 1, 2, 2]], dtype=torch.int32, device=dev)
    pts = torch.zeros((2, 10), dtype=torch.float32, device=dev)
    valid = torch.ones(2, dtype=torch.uint8, device=dev)
    out = torch.zeros((2, 160, 160, 3), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    null, s = C.c_void_p(0), engine._stream()
    good = dict(n=2, H=4, W=5, S=160)
    bad = [dict(n=0), dict(n=-1), dict(H=0), dict(W=0), dict(H=-3), dict(S=0), dict(S=4097)]

    def resize(n, H, W, S, fr_=p(fr), rect_=p(rect), valid_=p(valid), out_=p(out)):
        return lib.trl_debug_crop_resize(h, fr_, n, H, W, rect_, valid_, out_, s)

    def aligned(n, H, W, S, fr_=p(fr), rect_=p(pts), valid_=p(valid), out_=p(out)):
        return lib.trl_debug_crop_aligned(h, fr_, n, H, W, rect_, valid_, S, 1, out_, s)

    def area(n, H, W, S, fr_=p(fr), rect_=p(rect), valid_=p(valid), out_=p(out)):
        return lib.trl_debug_crop_area(h, fr_, n, H, W, rect_, valid_, S, 0, out_, s)
    for f in (resize, aligned, area):
        assert f(**good) == 0
        for b in bad:
            if f is resize and "S" in b:
                continue                                  # it has no S
            assert f(**{**good, **b}) == -1, (f.__name__, b)
        for k in ("fr_", "rect_", "valid_", "out_"):
            assert f(**good, **{k: null}) == -1, (f.__name__, k)
    for f in (aligned, area):
        assert f(**{**good, "n": 65536}) == -1, f.__name__
    assert lib.trl_debug_crop_resize(None, p(fr), 2, 4, 5, p(rect), p(valid), p(out), s) == -1
    assert lib.trl_debug_crop_aligned(None, p(fr), 2, 4, 5, p(pts), p(valid), 160, 1, p(out), s) == -1
    assert lib.trl_debug_crop_area(None, p(fr), 2, 4, 5, p(rect), p(valid), 160, 0, p(out), s) == -1
    torch.cuda.synchronize(dev)
    with pytest.raises(ValueError):
        engine.crop_resize(fr, rect[:1], valid)
    with pytest.raises(ValueError):
        engine.crop_area(fr, rect, valid[:1])
    with pytest.raises(ValueError):
        engine.crop_area(fr, rect, valid, out=out[:, :80, :80].contiguous())
    with pytest.raises(TrlError):
        engine.crop_area(fr, rect, valid, S=0)
