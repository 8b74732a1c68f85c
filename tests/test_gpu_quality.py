"""Face quality on the device (csrc/trl_quality.hip, quality.py) against tests/quality_ref.py.  Every comparison is equality: the
rectangle table on both frame batches, the same bits for every band height, on a side stream and over a workspace full of 0xFF, one
720p noise frame under a full-frame box, the points table under every parameter set, best shots over 1, 3 and 70 groups split into
calls three ways, and extract_faces / track_faces / FaceTracker(best_shots=True) on top."""
import os

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
from conftest import frames_small
import quality_ref as Q

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BANDS = (0, 1, 2, 7, 96)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _np(d: dict) -> dict:
    return {k: v.cpu().numpy() for k, v in d.items()}


def assert_same(got: dict, ref: dict, what="", hist=True):
    got = _np(got)
    assert np.array_equal(got["status"], ref["status"]) and got["status"].dtype == np.int32, what
    assert np.array_equal(got["raw"], ref["raw"]) and got["raw"].dtype == np.int64, (what, np.nonzero((got["raw"] != ref["raw"]).any(1))[0])
    if hist:
        assert np.array_equal(got["hist"], ref["hist"]) and got["hist"].dtype == np.int32, what
    bad = [i for i in range(len(ref["feat"])) if not Q.same_bits(got["feat"][i], ref["feat"][i])]
    assert not bad, (what, bad[:5], got["feat"][bad[0]].tolist(), ref["feat"][bad[0]].tolist())
    for i, name in enumerate(Q.FEAT[:10]):
        assert Q.same_bits(got[name], ref["feat"][:, i]), (what, name)


@pytest.fixture(scope="module")
def table_refs():
    frame_of, boxes = Q.rect_table()
    return {batch: Q.quality_ref(frames, frame_of, boxes) for batch, frames in Q.frame_batches().items()}


@pytest.mark.parametrize("batch", ("flat", "busy"))
def test_rectangle_table_at_every_band_height(lib, table_refs, batch):
    frame_of, boxes = Q.rect_table()
    ref = table_refs[batch]
    assert ref["status"].sum() == len(Q.RECTS) - len(Q.NO_FACE) and not ref["raw"][ref["status"] == 0].any()
    fr = torch.from_numpy(Q.frame_batches()[batch].copy()).cuda()
    fo, bx = torch.from_numpy(frame_of).cuda(), torch.from_numpy(boxes).cuda()
    for band in BANDS:
        assert_same(truely_amd.face_quality(fr, fo, bx, return_hist=True, max_band_rows=band), ref, (batch, band))
    # numpy inputs, no histogram asked for
    got = truely_amd.face_quality(Q.frame_batches()[batch].copy(), frame_of, boxes)
    assert "hist" not in got
    assert_same(got, ref, (batch, "numpy"), hist=False)
    # a side stream; a workspace that held 0xFF bytes, 8 bytes off a 256-byte boundary
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = truely_amd.face_quality(fr, fo, bx, return_hist=True, max_band_rows=7)
    side.synchronize()
    assert_same(got, ref, (batch, "side stream"))
    need = lib.trl_quality_workspace(len(boxes))
    for band in (0, 2):
        ws = torch.full((need // 8 + 1,), -1, dtype=torch.int64, device="cuda")
        assert_same(truely_amd.face_quality(fr, fo, bx, return_hist=True, max_band_rows=band, _workspace=ws[1:]), ref, (batch, band, "0xFF"))
    with pytest.raises(_lib.TrlError):
        truely_amd.face_quality(fr, fo, bx, _workspace=torch.zeros((need // 8 - 1,), dtype=torch.int64, device="cuda"))


def test_no_rows_and_refused_arguments(lib):
    fr = torch.from_numpy(Q.frame_batches()["busy"].copy()).cuda()
    got = truely_amd.face_quality(fr, np.zeros(0, np.int32), np.zeros((0, 4), F32), np.zeros((0, 10), F32), return_hist=True)
    assert got["quality"].shape == (0,) and got["raw"].shape == (0, 8) and got["hist"].shape == (0, 256) and got["status"].shape == (0,)
    with pytest.raises(ValueError):
        truely_amd.face_quality(fr, [0], [[0, 0, 5, 5]], params=truely_amd.QualityParams(clip_ref=0.0))
    with pytest.raises(ValueError):
        truely_amd.face_quality(fr, [0, 1], [[0, 0, 5, 5]])
    with pytest.raises(ValueError):
        truely_amd.face_quality(fr, [0], [[0, 0, 5, 5]], max_band_rows=-1)
    with pytest.raises(ValueError):
        truely_amd.face_quality(fr.float(), [0], [[0, 0, 5, 5]])


def test_720p_noise_frame_full_box(lib):
    """the sums' range and many bands' atomics at size: N = 921600, sum L^2 past 2^35"""
    rng = np.random.default_rng(720)
    frames = rng.integers(0, 256, (1, 720, 1280, 3), dtype=np.uint8)
    frame_of, boxes = np.zeros(2, np.int32), np.array([[0, 0, 1280, 720], [-3.5, 100.25, 1500, 619.5]], F32)
    ref = Q.quality_ref(frames, frame_of, boxes)
    assert ref["raw"][0, 0] == 921600 and ref["raw"][0, 4] > 2 ** 35 and ref["raw"][1, 0] == 1280 * 520
    fr = torch.from_numpy(frames).cuda()
    for band in (0, 1, 5):
        assert_same(truely_amd.face_quality(fr, frame_of, boxes, return_hist=True, max_band_rows=band), ref, band)


@pytest.mark.parametrize("params", range(len(Q.PARAM_SETS)))
def test_points_table(lib, params):
    prm = Q.PARAM_SETS[params]
    pts = Q.points_table()
    m = len(pts)
    frames = Q.frame_batches()["busy"].copy()
    frame_of = (np.arange(m) % 4).astype(np.int32)
    boxes = np.tile(np.array([[3.5, 2.25, 99.5, 90.0]], F32), (m, 1))
    boxes[1::2] = [20, 30, 50, 70.5]
    ref = Q.quality_ref(frames, frame_of, boxes, pts, prm)
    names = [n for n, _ in Q.POINTS]
    assert ref["yaw"][names.index("frontal")] == 0 and ref["pitch"][names.index("frontal")] == 0
    assert all(np.isnan(ref["yaw"][names.index(k)]) and ref["quality"][names.index(k)] == 0 for k in Q.NAN_POSE)
    assert ref["quality"].max() > 0
    qp = None if prm is None else truely_amd.QualityParams(**prm)
    assert_same(truely_amd.face_quality(frames, frame_of, boxes, pts, params=qp, return_hist=True), ref, params)
    # without points: the pose is NaN and its factor 1
    none = Q.quality_ref(frames, frame_of, boxes, None, prm)
    assert np.isnan(none["yaw"]).all() and (none["quality"] >= ref["quality"]).all()
    assert_same(truely_amd.face_quality(frames, frame_of, boxes, None, params=qp, return_hist=True), none, (params, "no points"))


# ---- best shots -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", (1, 3, 70))
def test_best_shots(lib, groups):
    q = Q.best_qualities()
    m = len(q)
    rng = np.random.default_rng(groups)
    gid = rng.integers(-2, groups + 2, m).astype(np.int32)
    faces = rng.standard_normal((m, 3, 5, 7)).astype(F32)
    faces[5, 0, 0, :2] = [np.nan, -0.0]                                        # (a copy keeps every bit)
    want = Q.best_brute(q, gid, groups)
    dq, dg, df = torch.from_numpy(q).cuda(), torch.from_numpy(gid).cuda(), torch.from_numpy(faces).cuda()
    for cuts in Q.BEST_SPLITS:
        keys, ref_faces = [0] * groups, np.zeros((groups, 3, 5, 7), F32)
        b = truely_amd.BestShots(groups, face_shape=(3, 5, 7))
        plain = truely_amd.BestShots(groups)
        for a, e in zip(cuts[:-1], cuts[1:]):
            Q.best_update(keys, q[a:e], gid[a:e], a, faces[a:e], ref_faces)
            b.add(dq[a:e], dg[a:e], df[a:e])
            plain.add(q[a:e], gid[a:e])
        row, quality = Q.best_read(keys, q)
        assert (row == want).all()
        got = _np(b.read())
        assert np.array_equal(got["row"], row) and got["row"].dtype == np.int32, cuts
        assert Q.same_bits(got["quality"], quality) and Q.same_bits(got["face"], ref_faces), cuts
        got = _np(plain.read())
        assert set(got) == {"row", "quality"} and np.array_equal(got["row"], row) and Q.same_bits(got["quality"], quality)
        assert b.rows_seen == plain.rows_seen == m
    # grow keeps the state; the new groups are empty; rows for them count from where the object stands
    b.grow(groups + 4)
    got = _np(b.read())
    assert np.array_equal(got["row"][:groups], row) and (got["row"][groups:] == -1).all() and np.isnan(got["quality"][groups:]).all()
    assert Q.same_bits(got["face"][:groups], ref_faces) and not got["face"][groups:].any()
    b.add(np.array([0.5, 2.0], F32), np.array([groups + 3, 0], np.int32), df[:2])
    got = _np(b.read())
    assert got["row"][groups + 3] == m and got["row"][0] == m + 1 and Q.same_bits(got["face"][0], faces[1])
    with pytest.raises(ValueError):
        b.grow(groups)
    with pytest.raises(ValueError):
        b.add(np.array([0.5], F32), np.array([0], np.int32))
    b.reset()
    got = _np(b.read())
    assert (got["row"] == -1).all() and b.rows_seen == 0


# ---- the engine and the tracker -----------------------------------------------------------------------------------------------------
def _multiface():
    z = np.load(os.path.join(GOLD, "clip_multiface_270p.npz"))
    return truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))


QUALITY_KEYS = set(Q.FEAT[:10]) | {"feat", "raw", "quality_status", "points"}


@pytest.mark.parametrize("clip", ("small", "multiface"))
def test_extract_faces_with_quality(engine, clip):
    fr = frames_small() if clip == "small" else _multiface()
    for keep_all, select_largest in ((True, True), (True, False), (False, True)):
        plain = engine.extract_faces(fr, keep_all=keep_all, select_largest=select_largest)
        off = engine.extract_faces(fr, keep_all=keep_all, select_largest=select_largest, quality=False)
        assert set(off) == set(plain) == {"faces", "frame", "box", "prob", "status", "counts" if keep_all else "valid"}
        assert all(torch.equal(off[k], plain[k]) for k in plain)
        got = engine.extract_faces(fr, keep_all=keep_all, select_largest=select_largest, quality=True)
        assert set(got) == set(plain) | QUALITY_KEYS
        assert all(torch.equal(got[k], plain[k]) for k in plain), (clip, keep_all, select_largest)
        m = got["box"].shape[0]
        assert got["points"].shape == (m, 10) and m >= (2 if keep_all and clip == "multiface" else 1)
        ref = Q.quality_ref(fr, got["frame"].cpu().numpy(), got["box"].cpu().numpy(), got["points"].cpu().numpy())
        assert_same(dict(got, status=got["quality_status"]), ref, (clip, keep_all, select_largest), hist=False)
        assert np.array_equal(ref["status"] == 1, got["frame"].cpu().numpy() >= 0)
        # Engine.face_quality on the same rows
        again = engine.face_quality(fr, got["frame"], got["box"], got["points"], return_hist=True)
        assert_same(again, ref, (clip, "face_quality"))


def test_track_faces_with_quality_and_best_shots(engine):
    fr = _multiface()
    windows = (fr, fr[::-1].copy(), fr)
    for strict in (False, True):
        # (synthetic weights put the five points anywhere: the references are set so that the pose zeroes no row, or every row)
        kw = dict(quality_params=truely_amd.QualityParams(yaw_ref=1e6, pitch_ref=1e-3 if strict else 1e6, clip_ref=1e6))
        trk = truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device, templates=True, best_shots=True)
        outs = [engine.track_faces(w, trk, quality=True, **kw) for w in windows]
        quality = np.concatenate([o["quality"].cpu().numpy() for o in outs])
        track = np.concatenate([o["track"].cpu().numpy() for o in outs])
        faces = np.concatenate([o["faces"].cpu().numpy() for o in outs])
        assert len(track) >= 6 and (track >= 0).all() and ((quality >= 0) & (quality <= 1)).all()
        best = _np(trk.best_shots())
        T = int(track.max()) + 1
        assert best["track"].tolist() == list(range(T)) and best["face"].shape == (T,) + faces.shape[1:]
        want = Q.best_brute(quality, track, T)
        assert np.array_equal(best["row"], want) and (want >= 0).all()
        for t in range(T):
            rows = np.nonzero(track == t)[0]
            assert quality[want[t]] == quality[rows].max() and want[t] == rows[quality[rows] == quality[rows].max()][0]
        assert Q.same_bits(best["quality"], quality[want]) and Q.same_bits(best["face"], faces[want])
        # the quality was the pool's weight: a row of quality 0 is skipped and counted, the others contribute
        tm = trk.templates()
        assert int(tm["skipped"]) == int((quality == 0).sum()) and int(tm["count"].sum()) == int((quality > 0).sum())
        assert (quality == 0).any() if strict else (quality > 0).any()
        # the same clip in one window gives the same best shots
        one = truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device, best_shots=True)
        engine.track_faces(np.concatenate(windows), one, quality=True, **kw)
        again = _np(one.best_shots())
        assert all(Q.same_bits(again[k], best[k]) for k in best)
        trk.reset()
        assert trk.best_shots()["row"].shape == (0,)
    # without quality the call is what it was
    t0, t1 = (truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device) for _ in range(2))
    a, b = engine.track_faces(fr, t0), engine.track_faces(fr, t1, quality=False)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        t0.update(a["box"], a["counts"], a["emb"], quality=a["prob"])
    with pytest.raises(ValueError):
        t0.best_shots()
    with pytest.raises(ValueError):
        truely_amd.FaceTracker(best_shots=True, device=engine.device).update(a["box"], a["counts"], a["emb"])
