"""trl_track_update / trl_track_scores (k_track_update, k_track_scores) and FaceTracker on the built clips of tests/track_ref.py.

Every comparison is bit for bit against the reference, and nothing is left out of one: the three per-row outputs, the whole track
table, the per-track scores and the summary.  One-hot and dyadic embeddings make every similarity exact and integer-grid boxes make
every IoU a known fraction, so every decision is known in advance (tests/test_tracks_cpu.py asserts what each clip is meant to
do); the one-face clips are drift_ref's and must equal Engine.drift_update.  The dense clips (track_ref.dense_cases) are the
opposite: nothing about them is exact, so the kernel's arithmetic and its hand-over of whole rows decide, and the state block is
compared as well.  No window exceeds 70 frames, no clip ~600 rows."""
import ctypes as C
import os

import numpy as np
import pytest

import drift_ref as D
import track_ref as T

pytestmark = pytest.mark.gpu
F32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FPS = 30
_REF = {}
CASES = tuple(T.cases())


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _t(x, device):
    import torch
    return torch.from_numpy(np.array(x, order="C")).to(device)


def ref_of(name, clip=None, lazy=False, table_cap=None):
    """The reference's answer for a built clip, computed once per session and never changed."""
    if (name, table_cap) not in _REF:
        c = clip or T.cases()[name]
        r = T.run_clip(c["counts"], c["boxes"], c["emb"], c["iou_min"], c["sim_min"], c["max_age"], table_cap=table_cap, lazy=lazy)
        for a in (r["track"], r["sim"], r["flag"]):
            a.setflags(write=False)
        _REF[(name, table_cap)] = r
    return _REF[(name, table_cap)]


def tracker_of(clip, device):
    import truely_amd
    return truely_amd.FaceTracker(clip["iou_min"], clip["sim_min"], clip["max_age"], device=device)


def run_windows(trk, clip, cuts=(), after=None):
    """The clip through FaceTracker.update in the windows cuts[k]..cuts[k+1] of its frames (0 and n are added); ``after(b)`` is
    called after the window that ends before frame b."""
    import torch
    counts = np.asarray(clip["counts"], np.int32)
    n = len(counts)
    rows = np.concatenate([[0], np.cumsum(counts)])
    cuts = sorted({0, n, *[c for c in cuts if 0 <= c <= n]})
    dev = trk.device
    d_boxes, d_counts = _t(clip["boxes"], dev), _t(counts, dev)
    d_emb = None if clip["emb"] is None else _t(clip["emb"], dev)
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]) if n else [(0, 0)]:
        ra, rb = int(rows[a]), int(rows[b])
        outs.append(trk.update(d_boxes[ra:rb], d_counts[a:b], None if d_emb is None else d_emb[ra:rb]))
        if after is not None:
            after(b)
    return {k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in ("track", "sim", "flag")}


def head_of(state):
    """(next_id, dropped, table_overflow) of a device state block."""
    w = state.cpu().numpy().view(np.int32)
    return int(w[T.HEAD_NEXT_ID]), int(w[T.HEAD_DROPPED]), int(w[T.HEAD_TABLE_OVERFLOW])


def check(trk, got, ref, what=""):
    """Outputs, table, scores, summary and the state's counters of a FaceTracker against the reference of the whole clip."""
    tr = ref["tracker"]
    assert np.array_equal(got["track"], ref["track"]), what
    assert np.array_equal(_bits(got["sim"]), _bits(ref["sim"])), what
    assert np.array_equal(got["flag"], ref["flag"]), what
    frame_count = max(tr.frames_seen, 1) * 4
    t = trk.tracks(frame_count, FPS)
    tab = tr.table_array()
    assert np.array_equal(t["id"], np.arange(tr.next_id)), what
    for col, name in enumerate(("first_frame", "last_frame", "n_obs", "run", "hits", "slot")):
        assert np.array_equal(t[name], tab[:, col]), (what, name)
    sc, summary = tr.scores(frame_count, FPS)
    assert np.array_equal(t["score"], sc), what
    assert [t["clip_score"], t["clip_track"], len(t["id"]), t["dropped"]] == summary, what
    assert trk.score(frame_count, FPS) == summary[0], what
    assert head_of(trk._state) == (tr.next_id, tr.dropped, 0), what
    assert int(trk._state.cpu().numpy()[0]) == tr.frames_seen, what


# ---- one face per frame: trl_drift_update ----------------------------------------------------------------------------------------
def _one_face_clips():
    out = {}
    for h, r in ((0, 0), (3, 16), (5, 2), (20, 30), (0, 15)):
        out[f"onehot_h{h}_r{r}"] = D.onehot_sequence(h, r)
    out["onehot_gaps"] = D.onehot_rows([D.DRIFT] * 17 + [D.NOFACE, D.NOFACE, D.DRIFT, D.SAME, D.NOFACE] + [D.DRIFT] * 20 + [D.NOFACE])
    pairs, _ = D.threshold_sweep()
    out["sweep"] = D.sweep_rows(pairs[384:417])               # the 33 pairs around 0.99f: below it, equal to it and above it
    for kind in ("plain", "sim_pos_inf", "sim_neg_inf", "scaled_up", "scaled_down"):      # the rows without a NaN similarity
        out[f"special_{kind}"] = D.special_rows()[kind]
    return out


ONE_FACE = tuple(_one_face_clips())


@pytest.mark.parametrize("name", ONE_FACE)
def test_one_face_is_drift_update(engine, name):
    """A clip with at most one face per frame, iou_min = 0, sim_min = -inf, max_age = INT32_MAX: the single track has the sims,
    flags, run, hits and score of Engine.drift_update for the same embeddings and valid = counts, window by window."""
    emb, valid = _one_face_clips()[name]
    n = len(valid)
    v = np.asarray(valid, bool)
    clip = {"counts": np.asarray(valid, np.int32), "boxes": np.tile(np.array(T.grid_box(3, 4), F32), (int(v.sum()), 1)),
            "emb": np.asarray(emb, F32)[v], "iou_min": 0.0, "sim_min": -np.inf, "max_age": T.INT32_MAX}
    cuts = list(range(0, n, 66))
    trk = tracker_of(clip, engine.device)
    got = run_windows(trk, clip, cuts)
    check(trk, got, ref_of(name, clip, lazy=True), name)
    # the drift kernels on the same windows (rows of frames without a face are never read: NaN)
    state = engine.drift_state()
    d_emb, d_valid = _t(np.where(v[:, None], np.asarray(emb, F32), np.nan).astype(F32), engine.device), _t(valid, engine.device)
    sims, flags, d = [], [], None
    for a, b in zip(cuts, cuts[1:] + [n]):
        d = engine.drift_update(state, d_emb[a:b], d_valid[a:b], n * 4, FPS)
        sims.append(d["sims"].cpu().numpy())
        flags.append(d["flags"].cpu().numpy())
    sims, flags = np.concatenate(sims), np.concatenate(flags)
    assert np.array_equal(_bits(got["sim"]), _bits(sims[v])) and (sims[~v] == 2.0).all(), name
    assert np.array_equal(got["flag"], flags[v]) and not flags[~v].any(), name
    t = trk.tracks(n * 4, FPS)
    assert (t["run"].tolist(), t["hits"].tolist(), t["score"].tolist()) == ([d["run"]], [d["hits"]], [d["score"]]), name
    assert (t["clip_score"], t["clip_track"]) == (d["score"], 0)
    if name == "sweep":
        s = got["sim"][D.SWEEP_PAIR::D.SWEEP_BLOCK]
        assert (s < F32(0.99)).any() and (s == F32(0.99)).any() and (s > F32(0.99)).any()
        assert np.array_equal(got["flag"][D.SWEEP_PAIR::D.SWEEP_BLOCK], (s < F32(0.99)).astype(np.uint8))


# ---- association, ageing, slots: every built clip in one call --------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_built_clip(engine, name):
    clip = T.cases()[name]
    trk = tracker_of(clip, engine.device)
    got = run_windows(trk, clip)
    check(trk, got, ref_of(name), name)


# ---- windows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("alternate3", "age2", "age0", "crossing_sim", "ties", "turnover", "counts_63_64_65", "counts_emb_off",
                                  "drifters", "slot_reuse"))
def test_every_cut(engine, name):
    """The clip cut at every frame boundary into two updates, and into windows of one frame: the outputs, the table and the
    summary of the single call."""
    clip = T.cases()[name]
    n = len(clip["counts"])
    ref = ref_of(name)
    trk = tracker_of(clip, engine.device)
    for cut in range(1, n):
        trk.reset()
        check(trk, run_windows(trk, clip, [cut]), ref, (name, cut))
    trk.reset()
    check(trk, run_windows(trk, clip, range(n)), ref, (name, "windows of 1"))


def test_empty_windows_and_rows_past_the_sum(engine):
    """n = 0 and m = 0 calls between the windows change nothing but the frame count; rows past the sum of counts are not read (they
    hold NaN boxes and embeddings) and come back as -1 / 2.0 / 0."""
    import torch
    clip = T.cases()["age2"]
    ref = ref_of("age2")
    dev = engine.device
    trk = tracker_of(clip, dev)
    none = torch.empty((0, 4), device=dev)
    out = trk.update(none, torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0, 512), device=dev))        # n = 0, m = 0
    assert out["track"].shape == (0,)
    got = run_windows(trk, clip, [5])
    trk.update(none, torch.empty((0,), dtype=torch.int32, device=dev), None)
    check(trk, got, ref)
    # m = 0 with frames: the all-empty window ages the tracks (max_age = 2: the fourth empty frame ends the two of the last frame)
    out = trk.update(none, torch.zeros((4,), dtype=torch.int32, device=dev), torch.empty((0, 512), device=dev))
    t = trk.tracks(100, FPS)
    assert (t["slot"] == -1).all() and np.array_equal(t["n_obs"], ref["tracker"].table_array()[:, 2])
    # rows past the sum
    trk.reset()
    counts = np.asarray(clip["counts"], np.int32)
    m = int(counts.sum())
    boxes = np.concatenate([clip["boxes"], np.full((5, 4), np.nan, F32)])
    emb = np.concatenate([clip["emb"], np.full((5, 512), np.nan, F32)])
    out = {k: v.cpu().numpy() for k, v in trk.update(_t(boxes, dev), _t(counts, dev), _t(emb, dev)).items()}
    assert (out["track"][m:] == -1).all() and (out["sim"][m:] == 2.0).all() and not out["flag"][m:].any()
    check(trk, {k: v[:m] for k, v in out.items()}, ref)
    # counts that promise more rows than there are: the rows that exist are tracked, nothing is read or written past them
    trk.reset()
    short = {k: v.cpu().numpy() for k, v in trk.update(_t(clip["boxes"][:3], dev), _t(counts, dev), _t(clip["emb"][:3], dev)).items()}
    assert np.array_equal(short["track"], ref["track"][:3])


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _c_update(lib, state, clip, track, sim, flag, table, cap, dev):
    import torch
    from truely_amd import _lib
    boxes, counts = _t(clip["boxes"], dev), _t(np.asarray(clip["counts"], np.int32), dev)
    emb = None if clip["emb"] is None else _t(clip["emb"], dev)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)
    _lib.check(lib.trl_track_update(p(state), p(boxes), p(counts), len(counts), len(boxes), p(emb), float(clip["iou_min"]),
                                    float(clip["sim_min"]), int(clip["max_age"]), p(track), p(sim), p(flag), p(table), cap,
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


@pytest.mark.parametrize("name,cap", (("ties", 3), ("turnover", 100), ("never", 0), ("alternate2_emb_off", 1)))
def test_small_table(engine, name, cap):
    """trl_track_update with a table smaller than the ids: the rows below table_cap are the full table's, the poison behind them
    is intact, the state counts the ids that had no row, and the tracking outputs do not change.  Outputs poison-filled before."""
    import torch
    from truely_amd import _lib
    lib, dev = _lib.load(), engine.device
    clip, full = T.cases()[name], ref_of(name)
    ref = ref_of(name, table_cap=cap)
    tr = ref["tracker"]
    m = len(clip["boxes"])
    assert tr.next_id > cap and tr.table_overflow == tr.next_id - cap
    state = torch.zeros((T.STATE_BYTES // 8,), dtype=torch.int64, device=dev)
    table = torch.full((cap + 32, 8), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    track = torch.full((m,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    sim = torch.full((m,), float("nan"), dtype=torch.float32, device=dev)
    flag = torch.full((m,), 0xFF, dtype=torch.uint8, device=dev)
    _c_update(lib, state, clip, track, sim, flag, table, cap, dev)
    tab = table.cpu().numpy()
    assert (tab[cap:] == 0x5A5A5A5A).all()
    assert np.array_equal(tab[:cap], tr.table_array(cap)) and np.array_equal(tab[:cap], full["tracker"].table_array()[:cap])
    assert head_of(state) == (tr.next_id, tr.dropped, tr.table_overflow)
    for got, want in ((track, full["track"]), (sim, full["sim"]), (flag, full["flag"])):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    # the scores of the rows that exist; the summary over them
    score = torch.full((cap + 32,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    summary = torch.zeros((4,), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr() if t.numel() else 0)
    _lib.check(lib.trl_track_scores(p(state), p(table), cap, 400, FPS, p(score), p(summary), None))
    sc, want = tr.scores(400, FPS, cap)
    assert np.array_equal(score.cpu().numpy()[:cap], sc) and (score.cpu().numpy()[cap:] == 0x5A5A5A5A).all()
    assert summary.cpu().numpy().tolist() == want


def test_table_grows_across_updates(engine):
    """FaceTracker owns the table: 281 tracks in two windows of 70 frames pass its first 256 rows, and no id goes without a row."""
    a, b = T.grid_box(0, 0), T.grid_box(6, 0)
    bad_nan = T.onehot([0])[0].copy()
    bad_nan[9] = np.nan
    frame = [(a, T.onehot([0])[0]), (b, np.zeros(512, F32)), (T.grid_box(40, 0), bad_nan)]
    clip = T.make_clip([frame] * 140, max_age=0)
    trk = tracker_of(clip, engine.device)
    assert trk._table.shape[0] == 256
    got = run_windows(trk, clip, [70])
    ref = ref_of("never_long", clip, lazy=True)
    assert ref["tracker"].next_id == 281 and trk._table.shape[0] >= 420
    check(trk, got, ref)


# ---- the answer does not depend on what the memory held ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("alternate3", "crowd64", "drifters"))
def test_reset_after_another_clip(engine, name):
    """A tracker that has seen another clip (all 64 slots taken, embeddings in the state, a table full of rows) and was reset()."""
    other = T.cases()["turnover"]
    clip = T.cases()[name]
    trk = tracker_of(clip, engine.device)
    run_windows(trk, other, [2])
    trk.reset()
    check(trk, run_windows(trk, clip, [1]), ref_of(name), name)


# ---- dense embeddings and real-valued boxes ---------------------------------------------------------------------------------------
# The clips of track_ref.dense_cases(): every one of an embedding's 512 elements is non-zero, n2 differs between slots by up to
# 2^80, no box coordinate is an integer, and the gates stand on computed values.  tests/test_tracks_cpu.py holds the reference to
# float64 and rational arithmetic on these clips and asserts what each contains; here the kernel equals the reference bit for bit.
@pytest.mark.parametrize("name", T.DENSE + T.GATE_NAMES)
def test_dense_clip(engine, name):
    clip = T.dense_clip(name)
    trk = tracker_of(clip, engine.device)
    check(trk, run_windows(trk, clip), T.dense_ref(name), name)


@pytest.mark.parametrize("name", T.DENSE)
def test_dense_every_cut(engine, name):
    """test_every_cut on the dense clips: the hand-over of 512 non-zero floats and their n2 per touched slot.  A track matched in
    the first window is read from the state in the second; for dense8 a three-window cut has a track matched in the first, absent
    for the whole second and matched from the state's copy, which the second window left alone, in the third."""
    clip, ref = T.dense_clip(name), T.dense_ref(name)
    n = len(clip["counts"])
    trk = tracker_of(clip, engine.device)
    for cut in range(1, n):
        trk.reset()
        check(trk, run_windows(trk, clip, [cut]), ref, (name, cut))
    trk.reset()
    check(trk, run_windows(trk, clip, range(n)), ref, (name, "windows of 1"))
    if name == "dense8":
        person, (a, b) = 1, (7, 9)                                                 # T.DENSE8_ABSENT: seen in frame 6, not in 7 and 8
        frame = np.repeat(np.arange(n), clip["counts"])
        ids = ref["track"][clip["person"] == person]
        at = frame[clip["person"] == person]
        assert ids[at == a - 1] == ids[at == b] and not ((frame >= a) & (frame < b) & (ref["track"] == ids[at == b])).any()
        trk.reset()
        check(trk, run_windows(trk, clip, [a, b]), ref, (name, "three windows"))


def check_state(trk, snap, emb, what):
    """The device's state block against track_ref.state_block of the reference's snapshot, bit for bit."""
    got = trk._state.cpu().numpy().view(np.uint8)
    want, compared = T.state_block(snap, emb)
    first = 32 + 64 * T.SLOTS
    assert got.shape == want.shape
    assert np.array_equal(got[:32].view(np.int32), want[:32].view(np.int32)), (what, "header")
    g, w = got[32:first].view(np.int32).reshape(T.SLOTS, 16), want[32:first].view(np.int32).reshape(T.SLOTS, 16)
    for lo, hi, field in ((0, 7, "used, id, first_frame, last_frame, n_obs, run, hits"), (7, 8, "src"), (8, 12, "box bits"),
                          (12, 13, "n2 bits"), (13, 16, "pad")):
        assert np.array_equal(g[:, lo:hi], w[:, lo:hi]), (what, field)
    g, w, c = (x[first:].reshape(T.SLOTS, 2048) for x in (got, want, compared))
    for s in range(T.SLOTS):
        if c[s].all():
            assert np.array_equal(g[s], w[s]), (what, "embedding of slot", s)
    assert np.array_equal(got[compared], want[compared]), what
    return compared


@pytest.mark.parametrize("name,cuts", (("dense8", (8,)), ("dense8", (14,)), ("dense8", None), ("dense_crowd", (2,)), ("dense_crowd", (4,)),
                                       ("dense_crowd", None)))
def test_state_after_each_window(engine, name, cuts):
    """After every window of a two-window run and of a run in windows of one frame (cuts = None), the whole state block: the
    header, every slot's integer fields with src == -1, its box and n2 bits and its padding, and all 512 floats of the embedding
    of every used slot against the row the reference names.  A slot never used holds zeros.  Left out, and nothing else: the
    embedding block of a slot that ageing has freed -- it keeps what the ended track left there, which nothing reads."""
    clip, ref = T.dense_clip(name), T.dense_ref(name)
    n = len(clip["counts"])
    trk = tracker_of(clip, engine.device)
    left_out = []
    after = lambda b: left_out.append(int((~check_state(trk, ref["states"][b], clip["emb"], (name, cuts, b))).sum()))
    check(trk, run_windows(trk, clip, range(n) if cuts is None else cuts, after), ref, (name, cuts))
    assert len(left_out) == (n if cuts is None else 2)
    if name == "dense8":                                                           # ageing has freed a slot by the clip's end
        assert left_out[-1] >= 2048
    assert (ref["states"][n]["slots"][:, 0] == 1).sum() == (8 if name == "dense8" else 64)


def test_rows_past_64_with_dense_rows(engine):
    """dense_crowd with NaN in the embeddings of detections 64 and 65 of every frame of 66: they come back as -1 / 2.0 / 0, and
    the answer for the rows before them is the one with numbers there -- the dropped rows are never read."""
    clip, ref = T.dense_clip("dense_crowd"), T.dense_ref("dense_crowd")
    emb = clip["emb"].copy()
    past = np.concatenate([66 * t + np.array([64, 65]) for t in range(4)])
    emb[past] = np.nan
    clip = dict(clip, emb=emb)
    trk = tracker_of(clip, engine.device)
    for cuts in ((), range(5)):
        trk.reset()
        got = run_windows(trk, clip, cuts)
        assert (got["track"][past] == -1).all() and (got["sim"][past] == 2.0).all() and not got["flag"][past].any()
        check(trk, got, ref, cuts)
        check_state(trk, ref["states"][5], clip["emb"], cuts)


# ---- Engine.track_faces -----------------------------------------------------------------------------------------------------------
def test_engine_track_faces(engine):
    """On the multi-face clip it is the three calls made by hand, bit for bit, and every row has a track."""
    import torch
    import truely_amd
    z = np.load(os.path.join(GOLD, "clip_multiface_270p.npz"))
    fr = truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))
    fr = np.concatenate([fr, fr])                              # (the clip twice: every face of the second half has a predecessor)
    trk = truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device)
    out = engine.track_faces(fr, trk)
    hand = engine.extract_faces(fr, keep_all=True)
    emb = engine.facenet_embed(hand["faces"].permute(0, 2, 3, 1))
    trk2 = truely_amd.FaceTracker(0.0, -np.inf, 3, device=engine.device)
    t2 = trk2.update(hand["box"], hand["counts"], emb)
    assert set(out) == set(hand) | {"emb", "track", "sim", "flag"}
    for k, v in hand.items():
        assert torch.equal(out[k], v), k
    assert out["emb"].cpu().numpy().tobytes() == emb.cpu().numpy().tobytes()
    for k in ("track", "sim", "flag"):
        assert out[k].cpu().numpy().tobytes() == t2[k].cpu().numpy().tobytes(), k
    counts, track = out["counts"].cpu().numpy(), out["track"].cpu().numpy()
    assert counts.sum() == len(track) >= 4 and (track >= 0).all()
    assert counts[0] >= 2 and (counts[1:] <= counts[0]).all(), counts.tolist()
    assert (out["sim"].cpu().numpy()[counts[0]:] != 2.0).all() and track.max() == counts[0] - 1     # no gate: every later face found a track
    # ... and it is the reference's answer for these boxes and embeddings
    clip = {"counts": counts, "boxes": out["box"].cpu().numpy(), "emb": emb.cpu().numpy(), "iou_min": 0.0, "sim_min": -np.inf, "max_age": 3}
    check(trk, {k: out[k].cpu().numpy() for k in ("track", "sim", "flag")}, ref_of("multiface", clip))
