"""trl_frame_signatures / trl_signature_distance / trl_shots_update (csrc/trl_shots.hip), trl_track_update_cuts and the Python on
top of them -- frame_signatures, signature_distance, ShotDetector, FaceTracker.update(cuts=), Engine.track_faces(shots=) -- held to
tests/shots_ref.py bit for bit.  Every reference is computed once per session and never changed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
import shots_ref as S
import track_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def batch_of(H, W):
    """(frames (9, H, W, 3): one frame of every content, their reference signatures)"""
    if (H, W) not in _CACHE:
        fr = np.concatenate([S.content_frames(kind, 1, H, W) for kind in S.CONTENTS])
        sig = S.signatures(fr)
        fr.setflags(write=False), sig.setflags(write=False)
        _CACHE[(H, W)] = fr, sig
    return _CACHE[(H, W)]


# ---- signatures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", S.SIZES)
def test_signatures_equal_reference(lib, H, W):
    fr, ref = batch_of(H, W)
    d = torch.from_numpy(fr.copy()).cuda()
    got = truely_amd.frame_signatures(d)
    assert got.dtype == torch.int32 and tuple(got.shape) == (9, 16, 3, 32)
    assert np.array_equal(got.cpu().numpy(), ref)
    N = S.region_pixels(H, W)
    assert np.array_equal(got.sum(-1).cpu().numpy(), np.broadcast_to(N[None, :, None], (9, 16, 3)))
    # batches of 1, 3 and 5, and a view that starts one frame in: with H W 3 odd, every byte phase of the 16-byte words
    for n in (1, 3, 5):
        assert np.array_equal(truely_amd.frame_signatures(d[:n]).cpu().numpy(), ref[:n]), n
    for a in range(1, 5):
        view = d[a:a + 3]
        assert view.data_ptr() == d.data_ptr() + a * H * W * 3
        assert np.array_equal(truely_amd.frame_signatures(view).cpu().numpy(), ref[a:a + 3]), a
    # a host array is uploaded
    assert np.array_equal(truely_amd.frame_signatures(fr[4:6].copy()).cpu().numpy(), ref[4:6])


def test_every_byte_phase(lib):
    """A 23 x 37 batch behind 0 .. 15 bytes of padding: the first and last 16-byte words are cut at every phase, and what lies in
    front of and behind the frames (255s: they would land in bin 31) reaches no count."""
    fr, ref = batch_of(23, 37)
    size = fr.size
    for phase in range(16):
        buf = torch.full((size + 64,), 255, dtype=torch.uint8, device="cuda")
        base = (-buf.data_ptr()) % 16 + phase
        buf[base:base + size] = torch.from_numpy(fr.reshape(-1).copy()).cuda()
        view = buf[base:base + size].view(9, 23, 37, 3)
        assert view.data_ptr() % 16 == phase
        assert np.array_equal(truely_amd.frame_signatures(view).cpu().numpy(), ref), phase


@pytest.mark.parametrize("H,W", ((23, 37), (180, 320)))
def test_band_heights_and_workspace_contents(lib, H, W):
    fr, ref = batch_of(H, W)
    d = torch.from_numpy(fr.copy()).cuda()
    for band in (0, 1, 2, 3, 7, H):
        assert np.array_equal(truely_amd.frame_signatures(d, max_band_rows=band).cpu().numpy(), ref), band
        need = lib.trl_shots_workspace(9, H, W, band)
        ws = torch.full((need // 8,), -1, dtype=torch.int64, device="cuda")           # every byte 0xFF
        assert np.array_equal(truely_amd.frame_signatures(d, max_band_rows=band, _workspace=ws).cpu().numpy(), ref), band
    short = torch.empty((lib.trl_shots_workspace(9, H, W, 1) // 8 - 1,), dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.TrlError, match="workspace"):
        truely_amd.frame_signatures(d, max_band_rows=1, _workspace=short)
    with pytest.raises(ValueError):
        truely_amd.frame_signatures(d[:, :3])
    assert tuple(truely_amd.frame_signatures(d[:0]).shape) == (0, 16, 3, 32)


# ---- distances ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", ((23, 37), (64, 64), (180, 320)))
def test_distances_equal_reference(lib, H, W):
    _, sig = batch_of(H, W)
    built = S.built_signature_pairs(H, W)
    a = np.stack([sig[i] for i in range(9) for j in range(9)] + [p[1] for p in built])
    b = np.stack([sig[j] for i in range(9) for j in range(9)] + [p[2] for p in built])
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    rd = [S.region_distances(x, y) for x, y in zip(a, b)]
    for drop in range(16):
        got = truely_amd.signature_distance(da, db, H, W, drop).cpu().numpy()
        want = np.array([S.distance_of(d, H, W, drop) for d in rd], F32)
        assert np.array_equal(_bits(got), _bits(want)), drop
        assert (got >= 0).all() and (got <= 1).all() and (got[::10][:9] == 0).all()
    names = [p[0] for p in built]
    got0 = truely_amd.signature_distance(da[81:], db[81:], H, W, 0).cpu().numpy()
    assert got0[names.index("extreme")] == 1.0 and got0[names.index("equal")] == 0.0
    assert truely_amd.signature_distance(da[81:], db[81:], H, W, 1).cpu().numpy()[names.index("one_region")] == 0.0
    assert tuple(truely_amd.signature_distance(da[:0], db[:0], H, W).shape) == (0,)
    with pytest.raises(ValueError):
        truely_amd.signature_distance(da, db, H, W, 16)


# ---- ShotDetector ---------------------------------------------------------------------------------------------------------------------
def _scene_ref(params):
    key = ("scene", tuple(sorted(params.items())))
    if key not in _CACHE:
        frames, starts = S.scene_clip()
        if "sigs" not in _CACHE:
            _CACHE["sigs"] = S.signatures(frames)
        _CACHE[key] = S.Shots(frames.shape[1], frames.shape[2], **params).update(_CACHE["sigs"])
    return _CACHE[key]


@pytest.mark.parametrize("params", (dict(), dict(min_shot=15), dict(threshold=0.0, drop=0), dict(threshold=0.05, drop=15, min_shot=3)))
def test_shot_detector_windows(lib, params):
    frames, starts = S.scene_clip()
    ref = _scene_ref(params)
    if not params:
        assert np.flatnonzero(ref["cut"]).tolist() == starts
    d = torch.from_numpy(frames).cuda()
    det = truely_amd.ShotDetector(truely_amd.ShotParams(**params))
    results = []
    for size in (1, 2, 7, 40):
        det.reset()
        outs = []
        for a in range(0, 40, size):
            outs.append(det.update(d[a:a + size]))
            empty = det.update(d[:0])                                             # an empty window between any two
            assert all(v.shape[0] == 0 for v in empty.values())
        got = {k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in ("sig", "dist", "cut", "shot")}
        assert np.array_equal(got["sig"], _CACHE["sigs"]), size
        assert np.array_equal(_bits(got["dist"]), _bits(ref["dist"])), size
        assert np.array_equal(got["cut"], ref["cut"]) and np.array_equal(got["shot"], ref["shot"]), size
        assert got["cut"].dtype == np.uint8 and got["shot"].dtype == np.int32
        results.append(got)
    state = det._state.cpu().numpy()
    cuts = np.flatnonzero(ref["cut"])
    assert state[0] == 40 and state[2] == len(cuts) and (len(cuts) == 0 or state[1] == cuts[-1])
    assert np.array_equal(state[4:].view(np.int32), _CACHE["sigs"][-1].reshape(-1))
    whole = truely_amd.detect_shots(d, truely_amd.ShotParams(**params), window=16)
    assert all(np.array_equal(whole[k].cpu().numpy(), results[0][k]) for k in ("dist", "cut", "shot"))
    # without reset() the clip goes on: its next frame is compared with the last one; another frame size is refused
    again = det.update(d[:1])
    assert again["dist"].item() == S.distance(_CACHE["sigs"][-1], _CACHE["sigs"][0], 36, 48, det.params.drop) and again["shot"].item() >= ref["shot"][-1]
    with pytest.raises(ValueError, match="reset"):
        det.update(d[:, :20])
    det.reset()
    first = det.update(d[:3])
    assert first["dist"][0].item() == 2.0 and np.array_equal(first["shot"].cpu().numpy(), ref["shot"][:3])


# ---- trl_track_update_cuts --------------------------------------------------------------------------------------------------------------
def _t(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()


def _cut_ref(name, emb_on):
    if ("cutref", name, emb_on) not in _CACHE:
        clip, cuts = S.cut_clips()[name]
        _CACHE[("cutref", name, emb_on)] = S.track_with_cuts(clip["counts"], clip["boxes"], clip["emb"] if emb_on else None, cuts, clip["iou_min"],
                                                           clip["sim_min"], clip["max_age"])
    return _CACHE[("cutref", name, emb_on)]


def _run_tracker(clip, cuts, emb_on, windows):
    trk = truely_amd.FaceTracker(clip["iou_min"], clip["sim_min"], clip["max_age"])
    counts = np.asarray(clip["counts"], np.int32)
    rows = np.concatenate([[0], np.cumsum(counts)])
    boxes, d_counts = _t(clip["boxes"]), _t(counts)
    emb = _t(clip["emb"]) if emb_on else None
    d_cuts = None if cuts is None else _t(cuts)
    outs = []
    for a, b in zip(windows[:-1], windows[1:]):
        ra, rb = int(rows[a]), int(rows[b])
        outs.append(trk.update(boxes[ra:rb], d_counts[a:b], None if emb is None else emb[ra:rb], cuts=None if d_cuts is None else d_cuts[a:b]))
    return trk, {k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in ("track", "sim", "flag")}


def _check_tracks(trk, got, ref, what):
    assert np.array_equal(got["track"], ref["track"]), what
    assert np.array_equal(_bits(got["sim"]), _bits(ref["sim"])), what
    assert np.array_equal(got["flag"], ref["flag"]), what
    t = trk.tracks(4 * max(ref["frames_seen"], 1), 30)
    assert len(t["id"]) == ref["next_id"] and t["dropped"] == ref["dropped"], what
    for col, name in enumerate(("first_frame", "last_frame", "n_obs", "run", "hits", "slot")):
        assert np.array_equal(t[name], ref["table"][:, col]), (what, name)
    assert int(trk._state.cpu().numpy()[0]) == ref["frames_seen"], what


@pytest.mark.parametrize("emb_on", (True, False))
@pytest.mark.parametrize("name", tuple(S.cut_clips()))
def test_cut_tracks_equal_the_per_shot_reference(lib, name, emb_on):
    clip, cuts = S.cut_clips()[name]
    n = len(cuts)
    ref = _cut_ref(name, emb_on)
    for windows in ([0, n], [0, n // 2, n], list(range(n + 1)) if n <= 10 else [0, 1, n - 1, n]):
        trk, got = _run_tracker(clip, cuts, emb_on, windows)
        _check_tracks(trk, got, ref, (name, emb_on, windows))
    if name == "one_face_drift" and emb_on:
        assert ref["table"][:, 3].tolist() == [19, 21, 17] and ref["table"][:, 4].tolist() == [4, 6, 2]
    if name == "crowd":
        assert ref["dropped"] == 2 + 2 + 1 + 1 and ref["next_id"] >= 64 + 64


def test_no_cuts_is_trl_track_update(lib):
    """d_cut NULL and d_cut all zero give trl_track_update's outputs, table, scores and state, byte for byte."""
    clip = T.cases()["alternate3"]
    counts, boxes, emb = _t(np.asarray(clip["counts"], np.int32)), _t(clip["boxes"]), _t(clip["emb"])
    n, m, cap = len(clip["counts"]), len(clip["boxes"]), 64
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for mode in ("plain", "null", "zeros"):
        state = torch.zeros((T.STATE_BYTES // 8,), dtype=torch.int64, device="cuda")
        track = torch.full((m,), -7, dtype=torch.int32, device="cuda")
        sim = torch.full((m,), -7.0, dtype=torch.float32, device="cuda")
        flag = torch.full((m,), 7, dtype=torch.uint8, device="cuda")
        table = torch.full((cap, 8), -7, dtype=torch.int32, device="cuda")
        rules = (float(clip["iou_min"]), float(clip["sim_min"]), int(clip["max_age"]))
        if mode == "plain":
            _lib.check(lib.trl_track_update(p(state), p(boxes), p(counts), n, m, p(emb), *rules, p(track), p(sim), p(flag), p(table), cap, stream))
        else:
            cut = None if mode == "null" else torch.zeros((n,), dtype=torch.uint8, device="cuda")
            _lib.check(lib.trl_track_update_cuts(p(state), p(boxes), p(counts), p(cut), n, m, p(emb), *rules, p(track), p(sim), p(flag), p(table),
                                                 cap, stream))
        score = torch.empty((cap,), dtype=torch.int32, device="cuda")
        summary = torch.empty((4,), dtype=torch.int32, device="cuda")
        _lib.check(lib.trl_track_scores(p(state), p(table), cap, 4 * n, 30, p(score), p(summary), stream))
        results.append([t.cpu().numpy().tobytes() for t in (track, sim, flag, table, score, summary, state)])
    assert results[0] == results[1] == results[2]
    ref = T.run_clip(clip["counts"], clip["boxes"], clip["emb"], clip["iou_min"], clip["sim_min"], clip["max_age"], lazy=True)
    assert results[0][0] == ref["track"].tobytes()


# ---- Engine.track_faces(shots=) -----------------------------------------------------------------------------------------------------------
def test_engine_track_faces_with_shots(engine):
    """The multi-face clip and then the same frames reversed.  The detector and the tracker used by hand give the same bits; the
    judge is the reference: shots_ref on the frames, the per-shot tracker on the boxes and embeddings."""
    z = np.load(os.path.join(GOLD, "clip_multiface_270p.npz"))
    fr = truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))
    fr = np.concatenate([fr, fr[::-1]])
    n, H, W = fr.shape[:3]
    # the clip has no hard cut: by the REFERENCE its distances are 2.0, 0.0243, 0 (the middle pair is one frame twice), 0.0243, so a
    # threshold of 0.02 makes frames 1 and 3 cuts and the tracker sees some
    params = dict(threshold=0.02, drop=4, min_shot=1)
    ref = S.Shots(H, W, **params).update(S.signatures(fr))
    assert ref["cut"].tolist() == [0, 1, 0, 1] and n == 4
    det = truely_amd.ShotDetector(truely_amd.ShotParams(**params), device=engine.device)
    trk = truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device)
    out = engine.track_faces(fr, trk, shots=det)
    hand = engine.extract_faces(fr, keep_all=True)
    assert set(out) == set(hand) | {"emb", "track", "sim", "flag", "dist", "cut", "shot"}
    for k in ("dist", "cut", "shot"):
        assert out[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    counts, boxes, emb = out["counts"].cpu().numpy(), out["box"].cpu().numpy(), out["emb"].cpu().numpy()
    tref = S.track_with_cuts(counts, boxes, emb, ref["cut"], 0.0, -np.inf, 3)
    _check_tracks(trk, {k: out[k].cpu().numpy() for k in ("track", "sim", "flag")}, tref, "engine")
    assert tref["next_id"] > counts[0]                           # the cuts started tracks that the plain tracker would not have
    # ... and the pieces by hand
    det2 = truely_amd.ShotDetector(truely_amd.ShotParams(**params), device=engine.device)
    trk2 = truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device)
    s2 = det2.update(torch.from_numpy(fr).to(engine.device))
    t2 = trk2.update(hand["box"], hand["counts"], engine.facenet_embed(hand["faces"].permute(0, 2, 3, 1)), cuts=s2["cut"])
    for k in ("track", "sim", "flag"):
        assert out[k].cpu().numpy().tobytes() == t2[k].cpu().numpy().tobytes(), k
    # without shots= nothing changes: the keys of before
    plain = engine.track_faces(fr, truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device))
    assert set(plain) == set(hand) | {"emb", "track", "sim", "flag"}
