"""k_mtcnn_front's own output -- the pooled conv1 map of every R-/O-Net candidate -- on the window table of tests/front_ref.py.

trl_debug_front (Engine.front_pool) launches the kernel as trl_stage_net does, on records the test gives directly, and returns the
map the tail would read.  The reference is the C oracle: area_resample_norm, then orc_front (conv1, PReLU, MaxPool through the
functions orc_rnet / orc_onet run); tests/test_front_cpu.py holds the oracle to the plain restatement on the same records, bit for
bit, and asserts from front_path that these records reach every code path of the kernel's crop.

How a wrong read becomes a wrong result: frames hold random bytes (or all 0, all 255, a 1-px checkerboard), they are the head of a
device buffer whose tail is 0xFF (once 0x00), the windows sit at every frame corner of every frame, and in one batch all frames
are alike, so the same window read with plain loads (frame 0) and with the end-of-buffer clamp (last frame) must give the same
bits.  The launch covers more slots than there are records: maps are pre-filled with NaN, every live map is compared over the whole
tensor AS BITS (zeros keep their sign), every other slot must still be NaN.
"""
import functools

import numpy as np
import pytest
import torch

import truely_amd
import front_ref as R

pytestmark = pytest.mark.gpu
EXTRA = 5                                   # launch slots past the records


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_frames(engine, base, tail=0xFF, offset=0):
    """The frames at byte `offset` of a device buffer whose other bytes are `tail`; the engine must pass the view on as it is."""
    n, H, W, _ = base.shape
    fb = n * H * W * 3
    buf = torch.full((offset + fb + max(4096, 2 * W * 3 + 64),), tail, dtype=torch.uint8, device=engine.device)
    frames = buf[offset:offset + fb].view(n, H, W, 3)
    frames.copy_(torch.from_numpy(base))
    assert engine._frames(frames).data_ptr() == buf.data_ptr() + offset
    return frames, buf


def _run(engine, frames, rec, S):
    cap = len(rec) + EXTRA
    P, C1 = R.NETS[S]["P"], R.NETS[S]["C1"]
    out = torch.full((cap, P, P, C1), float("nan"), dtype=torch.float32, device=engine.device)
    got = engine.front_pool(frames, rec, S, cap, out=out).cpu().numpy()
    assert np.isnan(got[len(rec):]).all(), "a slot past the device total was written"
    return got[:len(rec)]


def _reference(oracle, base, rec, S):
    crops = np.stack([oracle.area_resample_norm(base[f], y0, y0 + ih, x0, x0 + iw, S, S) for f, y0, x0, ih, iw in rec.tolist()])
    return oracle.front(crops, S)


def _check(engine, oracle, base, rec, S, tag, tail=0xFF, offset=0, flat=False):
    frames, buf = _device_frames(engine, base, tail, offset)
    got = _run(engine, frames, rec, S)
    del frames, buf
    want = _reference(oracle, base, rec[:1] if flat else rec, S)        # a flat frame has one crop, whatever the window
    bad = [i for i in range(len(rec)) if not np.array_equal(_bits(got[i]), _bits(want[0 if flat else i]))]
    assert not bad, (tag, len(bad), [(rec[i].tolist(), R.front_path(rec[i], len(base), *base.shape[1:3], S)) for i in bad[:4]])
    return got


@pytest.mark.parametrize("nf,H,W", R.BATCHES)
@pytest.mark.parametrize("S", [24, 48])
def test_table_equals_the_oracle(engine, oracle, S, nf, H, W):
    """Every record of front_ref.placed (the records whose coverage test_front_cpu.py asserts), every content, seeded weights."""
    rec = R.placed(nf, H, W, S)
    for ci, kind in enumerate(("random", "checker", "zeros", "ones")):
        base = R.content_frames(kind, nf, H, W, seed=101 * ci + H + S)
        _check(engine, oracle, base, rec, S, (kind, nf, H, W), flat=kind in ("zeros", "ones"))
    # all frames alike, tail 0x00: a window's bits cannot depend on its frame (plain loads on frame 0, clamped on the last)
    base = R.content_frames("same", nf, H, W, seed=7 + W)
    got = _check(engine, oracle, base, rec, S, ("same", nf, H, W), tail=0x00)
    by_win = {}
    for i, r in enumerate(rec.tolist()):
        by_win.setdefault(tuple(r[1:]), []).append(i)
    multi = [v for v in by_win.values() if len(v) > 1]
    assert multi and any({rec[i][0] for i in v} >= {0, nf - 1} for v in multi)
    for v in multi:
        for i in v[1:]:
            assert np.array_equal(_bits(got[i]), _bits(got[v[0]])), rec[i].tolist()


def test_huge_bins_rnet(engine, oracle):
    """One 2500 x 16383 frame of mostly 255s: the full-frame window's bins hold ~71,700 px, their sums pass 2^24 (one rounding in
    the conversion, as in the oracle) and a single bin is wider than the column strip; a 7000-px window next to it takes the
    column sums without the reciprocal division."""
    nf, H, W = R.HUGE
    rng = np.random.default_rng(9)
    base = np.full((nf, H, W, 3), 255, np.uint8)
    base[0, rng.integers(0, H, 200000), rng.integers(0, W, 200000)] = rng.integers(0, 256, (200000, 3), dtype=np.uint8)
    base[0, ::97, ::13] = 0
    rec = np.array([(0, 0, 0, H, W), (0, 0, 0, H, 7000), (0, H - 2400, W - 7392, 2400, 7392), (0, 3, W - 7417, H - 3, 7417)], np.int32)
    paths = [R.front_path(r, nf, H, W, 24) for r in rec]
    assert [p["kind"] for p in paths] == ["wide", "big", "big", "wide"] and not any(p["fastdiv"] for p in paths)
    assert paths[0]["max_bin"] > 65793 and False in paths[2]["safe"]
    _, _, sums = R.area_resample(base[0], 0, 0, H, W, 24)
    assert sums.max() >= 1 << 24
    _check(engine, oracle, base, rec, 24, "huge")


@pytest.mark.parametrize("S", [24, 48])
def test_wide_bins(engine, oracle, S):
    """Two 12 x 16383 frames: windows on either side of the width past which one bin outgrows half the per-wave column strip
    (7,392 | 7,393 px for R-Net, 10,176 | 10,177 px for O-Net), at both edges of the first and of the last frame -- there the
    right-edge windows end at the buffer's last byte -- and the full frame."""
    nf, H, W = R.WIDE
    rec = R.wide_records(S)
    kinds = [R.front_path(r, nf, H, W, S)["kind"] for r in rec]
    assert set(kinds) == {"big", "wide"} and kinds.count("wide") == 8
    for ci, (kind, tail) in enumerate((("random", 0xFF), ("checker", 0x00))):
        _check(engine, oracle, R.content_frames(kind, nf, H, W, seed=50 + ci + S), rec, S, ("wide", kind), tail=tail)


@functools.lru_cache(maxsize=None)
def _variant(variant):
    from oracle.oracle import Oracle
    from truely_amd.engine import Engine
    blob = R.slope_blob(variant)
    return Engine(blob), Oracle(blob)


@pytest.mark.parametrize("variant", R.SLOPE_VARIANTS[1:])
def test_slope_classes(variant):
    """MODE 1 (slopes above 1), MODE 0 (negative slopes: the pool keeps the window's minimum next to its maximum) and slopes of
    exactly 0.0, 1.0 and -0.0, on flat dark and flat bright frames -- whole pooling windows of one sign -- and on random bytes."""
    eng, orc = _variant(variant)
    t = truely_amd.weights.unpack_tensors(R.slope_blob(variant))
    nf, H, W = 3, 211, 333
    for S in (24, 48):
        nm = R.NETS[S]["name"]
        rec = R.placed(nf, H, W, S)[::3]
        assert {R.front_path(r, nf, H, W, S)["kind"] for r in rec} == {"small", "big"}
        for kind in ("zeros", "ones", "random"):
            base = R.content_frames(kind, nf, H, W, seed=3)
            _check(eng, orc, base, rec, S, (variant, kind), flat=kind != "random")
            if kind != "random":                            # a flat crop: each channel's conv map is one value, of either sign
                crop = np.full((1, S, S, 3), (np.float32(base[0, 0, 0, 0]) - np.float32(127.5)) * np.float32(0.0078125), np.float32)
                conv = R.conv1(crop, t[f"{nm}.conv1.w"], t[f"{nm}.conv1.b"])
                assert (conv < 0).any() and (conv > 0).any()


def test_empty_list_and_refusals(engine):
    """nb = 0 writes nothing; a window outside its frame, a bad frame index, an empty window and a busy context are refused."""
    from truely_amd._lib import TrlError
    fr = torch.from_numpy(R.content_frames("random", 2, 40, 50, 1)).to(engine.device)
    for S in (24, 48):
        out = torch.full((4, R.NETS[S]["P"], R.NETS[S]["P"], R.NETS[S]["C1"]), float("nan"), device=engine.device)
        engine.front_pool(fr, np.zeros((0, 5), np.int32), S, 4, out=out)
        assert torch.isnan(out).all()
        for bad in ((0, 0, 0, 41, 50), (0, 1, 0, 40, 50), (0, 0, 1, 40, 50), (2, 0, 0, 4, 4), (-1, 0, 0, 4, 4), (0, -1, 0, 4, 4), (0, 0, -1, 4, 4),
                    (0, 0, 0, 0, 4), (0, 0, 0, 4, 0), (1, 2 ** 31 - 1, 0, 2, 2), (1, 0, 2 ** 31 - 1, 2, 2)):
            with pytest.raises(TrlError) as e:
                engine.front_pool(fr, np.array([(0, 0, 0, 40, 50), bad], np.int32), S, 4, out=out)
            assert e.value.status == -1, bad
        assert torch.isnan(out).all()
        engine.front_pool(fr, np.array([(1, 0, 0, 40, 50)], np.int32), S, 4, out=out)
        assert not torch.isnan(out[0]).any() and torch.isnan(out[1:]).all()
    small = truely_amd.synthetic.synthetic_frames(2, 97, 131, seed=1)
    engine.detect_embed_begin(small)
    with pytest.raises(TrlError) as e:
        engine.front_pool(fr, np.array([(0, 0, 0, 4, 4)], np.int32), 24)
    assert e.value.status == -5
    engine.detect_embed_end()


def test_frame_base_address(engine, oracle):
    """include/truely_hip.h: the frame pointer must be a multiple of 4 (the pyramid and front kernels turn it into dword and
    16-byte loads).  A batch that starts 1, 2 or 3 bytes into an allocation is refused by every entry point that takes one, with
    nothing written; one that starts 4 bytes in gives the bits of the run at the allocation's start."""
    from truely_amd._lib import TrlError
    nf, H, W = 5, 211, 333
    base = R.content_frames("random", nf, H, W, seed=17)
    clip = truely_amd.synthetic.synthetic_frames(3, 211, 333, seed=11)          # a face in every frame; a frame is 1 mod 4 bytes
    ref = engine.detect_embed(clip)
    ref = {k: ref[k].clone() for k in ("box", "prob", "rect", "valid", "emb")}
    assert int(ref["valid"].sum()) == 3
    win = np.array([(0, 0, 0, 40, 50)], np.int32)
    for offset in (1, 2, 3):
        frames, buf = _device_frames(engine, clip, 0xFF, offset)
        out = torch.full((2, 11, 11, 28), float("nan"), device=engine.device)
        for call in (lambda: engine.front_pool(frames, win, 24, 2, out=out), lambda: engine.detect_embed(frames),
                     lambda: engine.mtcnn_detect(frames), lambda: engine.detect_embed_begin(frames),
                     lambda: engine.front_net(frames[:1], np.array([[1, 1, 40, 40]], np.float32), 24),
                     lambda: engine.stage_net(frames, np.array([[0, 1, 1, 40, 40]], np.float32), 48, 1),
                     lambda: engine.pyramid_level(frames[0], 0)):
            with pytest.raises(TrlError) as e:
                call()
            assert e.value.status == -1 and "4-byte aligned" in str(e.value), offset
        assert torch.isnan(out).all()
        if offset == 3:                                           # frames of 1 mod 4 bytes: the second frame of this batch IS aligned
            engine.front_pool(frames[1:], win, 24, 2, out=out)
            assert not torch.isnan(out[0]).any() and torch.isnan(out[1]).all()
    for S in (24, 48):
        _check(engine, oracle, base, R.placed(nf, H, W, S), S, "offset 4", offset=4)
    frames, buf = _device_frames(engine, clip, 0xFF, 4)
    out = engine.detect_embed(frames)
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
