"""Reference of shot boundaries (trl_frame_signatures / trl_signature_distance / trl_shots_update, csrc/trl_shots.h), of cut-aware
tracking (trl_track_update_cuts) and the built inputs their tests share.  numpy / Python only: no GPU, no oracle.

The rule ("Shots"):

    signature   of a frame u8 [H][W][3], 4 <= H, W <= 16384: sig[16][3][32] int32; region r = 4 i + j covers rows
                H i // 4 .. H (i + 1) // 4 - 1 and columns W j // 4 .. W (j + 1) // 4 - 1; sig[r][c][v >> 3] += 1 per pixel and channel
    distance    d_r = sum_c sum_{k = 0 .. 30} |Ca[c][k] - Cb[c][k]| over the cumulative counts; the regions by (d_r, r) ascending, the
                first 16 - drop kept; dist = float32(float64(sum of kept d_r) / float64(sum of kept 93 N_r))
    cuts        dist[0] of a clip is 2.0; cut[t] = dist[t] != 2.0 and dist[t] >= threshold and t - last_cut >= min_shot, last_cut
                = -min_shot before the first cut; shot[t] = the cuts at frames <= t

Cut-aware tracking is NOT written as "end every track at a cut": a clip with cuts is tracked as each shot alone, on a fresh
tests/track_ref.py tracker, and the pieces are joined -- ids shifted by the tracks created so far, frame numbers by the frames seen,
the dropped counts added, every track of an earlier shot ended (slot -1)."""
from __future__ import annotations

import numpy as np

import track_ref as T

F32 = np.float32
NO_DIST = F32(2.0)
DEFAULTS = {"threshold": 0.12, "drop": 4, "min_shot": 1}
SIZES = ((4, 4), (5, 7), (23, 37), (64, 64), (180, 320), (360, 642))


def edges(length):
    return [length * i // 4 for i in range(5)]


def region_pixels(H, W):
    """(16,) int64: N_r"""
    eh, ew = edges(H), edges(W)
    return np.array([(eh[i + 1] - eh[i]) * (ew[j + 1] - ew[j]) for i in range(4) for j in range(4)], np.int64)


def signature(frame):
    """(H, W, 3) uint8 -> (16, 3, 32) int32"""
    frame = np.asarray(frame)
    H, W, _ = frame.shape
    eh, ew = edges(H), edges(W)
    sig = np.zeros((16, 3, 32), np.int32)
    for i in range(4):
        for j in range(4):
            block = frame[eh[i]:eh[i + 1], ew[j]:ew[j + 1]] >> 3
            for c in range(3):
                for v in block[:, :, c].reshape(-1).tolist():
                    sig[4 * i + j, c, v] += 1
    return sig


def signature_fast(frame):
    """signature() with np.add.at: the same counts for the larger frames (test_shots_cpu.py holds the two to each other)"""
    frame = np.asarray(frame)
    H, W, _ = frame.shape
    eh, ew = edges(H), edges(W)
    ri = np.searchsorted(eh[1:4], np.arange(H), side="right")
    rj = np.searchsorted(ew[1:4], np.arange(W), side="right")
    r = (4 * ri[:, None] + rj[None, :])[:, :, None]
    idx = (r * 3 + np.arange(3)[None, None, :]) * 32 + (frame >> 3)
    sig = np.zeros(16 * 3 * 32, np.int32)
    np.add.at(sig, idx.reshape(-1), 1)
    return sig.reshape(16, 3, 32)


def signatures(frames):
    return np.stack([signature_fast(f) for f in frames]) if len(frames) else np.zeros((0, 16, 3, 32), np.int32)


def region_distances(a, b):
    """d_r as Python ints"""
    out = []
    for r in range(16):
        d = 0
        for c in range(3):
            ca = cb = 0
            for k in range(31):
                ca += int(a[r, c, k])
                cb += int(b[r, c, k])
                d += abs(ca - cb)
        out.append(d)
    return out


def distance_of(d, H, W, drop=4):
    N = region_pixels(H, W)
    order = sorted(range(16), key=lambda r: (d[r], r))[:16 - drop]
    D, M = sum(d[r] for r in order), sum(93 * int(N[r]) for r in order)
    return F32(np.float64(D) / np.float64(M))


def distance(a, b, H, W, drop=4):
    return distance_of(region_distances(np.asarray(a), np.asarray(b)), H, W, drop)


class Shots:
    """The cut scan, one frame at a time, with the state a clip carries."""

    def __init__(self, H, W, threshold=0.12, drop=4, min_shot=1):
        self.H, self.W, self.threshold, self.drop, self.min_shot = H, W, F32(threshold), drop, min_shot
        self.last_sig, self.frames_seen, self.last_cut, self.cuts = None, 0, -min_shot, 0

    def update(self, sigs):
        dist, cut, shot = [], [], []
        for s in sigs:
            t = self.frames_seen
            d = NO_DIST if self.last_sig is None else distance(self.last_sig, s, self.H, self.W, self.drop)
            is_cut = bool(d != NO_DIST and d >= self.threshold and t - self.last_cut >= self.min_shot)
            if is_cut:
                self.last_cut, self.cuts = t, self.cuts + 1
            dist.append(d), cut.append(is_cut), shot.append(self.cuts)
            self.last_sig, self.frames_seen = s, t + 1
        return {"dist": np.array(dist, F32), "cut": np.array(cut, np.uint8), "shot": np.array(shot, np.int32)}


def scan(dist, threshold=0.12, min_shot=1):
    """cut / shot of a clip from its distances alone"""
    threshold = F32(threshold)
    cut, shot, last, cuts = [], [], -min_shot, 0
    for t, d in enumerate(np.asarray(dist, F32)):
        c = bool(d != NO_DIST and d >= threshold and t - last >= min_shot)
        if c:
            last, cuts = t, cuts + 1
        cut.append(c), shot.append(cuts)
    return np.array(cut, np.uint8), np.array(shot, np.int32)


# ---- built frames ------------------------------------------------------------------------------------------------------------------
def sixteen_constants(H, W, base=0):
    """A frame whose region r is the constant 16 r + 5 c + base (mod 256) in channel c: one bin per (region, channel)"""
    eh, ew = edges(H), edges(W)
    f = np.zeros((H, W, 3), np.uint8)
    for i in range(4):
        for j in range(4):
            r = 4 * i + j
            f[eh[i]:eh[i + 1], ew[j]:ew[j + 1]] = [(16 * r + base) % 256, (16 * r + 5 + base) % 256, (16 * r + 10 + base) % 256]
    return f


CONTENTS = ("noise", "zero", "full", "edge_low", "edge_high", "ramp_x", "ramp_y", "checker", "sixteen")


def content_frames(kind, n, H, W, seed=0):
    """(n, H, W, 3) uint8 of one kind of content"""
    rng = np.random.default_rng([seed, H, W, CONTENTS.index(kind)])
    y, x = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if kind == "zero":
        return np.zeros((n, H, W, 3), np.uint8)
    if kind == "full":
        return np.full((n, H, W, 3), 255, np.uint8)
    if kind == "edge_low":                                      # 7 | 8: the two sides of the first bin edge
        return (7 + rng.integers(0, 2, (n, H, W, 3))).astype(np.uint8)
    if kind == "edge_high":                                     # 247 | 248: the two sides of the last
        return (247 + rng.integers(0, 2, (n, H, W, 3))).astype(np.uint8)
    if kind == "ramp_x":
        return np.stack([np.stack([(x * 256 // W + 40 * k + 85 * c) % 256 for c in range(3)], -1) for k in range(n)]).astype(np.uint8)
    if kind == "ramp_y":
        return np.stack([np.stack([(y * 256 // H + 40 * k + 85 * c) % 256 for c in range(3)], -1) for k in range(n)]).astype(np.uint8)
    if kind == "checker":                                       # two bins, pixel by pixel
        return np.stack([np.stack([np.where((x + y + k + c) % 2, 200, 40) for c in range(3)], -1) for k in range(n)]).astype(np.uint8)
    if kind == "sixteen":
        return np.stack([sixteen_constants(H, W, 3 * k) for k in range(n)])
    raise KeyError(kind)


def built_signature_pairs(H=23, W=37):
    """(name, a, b) of signatures BUILT for the distance: extremes, ties, one changed region"""
    N = region_pixels(H, W)

    def const(bins):
        s = np.zeros((16, 3, 32), np.int32)
        for r in range(16):
            s[r, :, bins[r]] = N[r]
        return s
    lo, hi = const([0] * 16), const([31] * 16)
    out = [("equal", lo, lo), ("extreme", lo, hi), ("extreme_swapped", hi, lo)]
    one = lo.copy()
    one[5, :, 0], one[5, :, 31] = 0, N[5]
    out.append(("one_region", lo, one))
    # every region moved by the same number of bins: on a size with equal N_r every d_r ties; with a shift per region, all distinct
    out.append(("all_shift_3", lo, const([3] * 16)))
    out.append(("descending", lo, const([16 - r for r in range(16)])))
    out.append(("pairs_tied", lo, const([1 + (r // 2) % 3 for r in range(16)])))
    half = lo.copy()
    half[:, 1, 0] //= 2
    half[:, 1, 17] = lo[:, 1, 0] - half[:, 1, 0]
    out.append(("one_channel_half", half, lo))
    return out


def scene_clip(n=40, H=36, W=48, starts=(0, 13, 27), seed=4):
    """n frames of three "scenes" (starting at `starts`): a scene is a fixed random layout of flat blocks, a frame is the scene plus
    a little noise and one small block that moves.  -> (frames, the frames at which a scene starts)"""
    rng = np.random.default_rng(seed)
    scenes = [np.kron(rng.integers(0, 256, (6, 8, 3)), np.ones((H // 6, W // 8, 1))).astype(np.int64) for _ in starts]
    frames = np.zeros((n, H, W, 3), np.uint8)
    for t in range(n):
        k = sum(t >= s for s in starts) - 1
        f = scenes[k] + rng.integers(-2, 3, (H, W, 3))
        f[10:16, (3 * t) % (W - 6):(3 * t) % (W - 6) + 6] = 255 - scenes[k][10:16, :6]
        frames[t] = np.clip(f, 0, 255)
    return frames, list(starts[1:])


# ---- cut-aware tracking: each shot alone, joined ---------------------------------------------------------------------------------------
def track_with_cuts(counts, boxes, emb, cuts, iou_min=0.0, sim_min=-np.inf, max_age=T.INT32_MAX):
    """-> dict(track, sim, flag (m,), table (next_id, 8) int32, next_id, dropped, frames_seen)"""
    counts = np.asarray(counts, np.int64)
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    n, rows = len(counts), np.concatenate([[0], np.cumsum(counts)])
    starts = [0] + [t for t in range(1, n) if cuts[t]]
    track, sim, flag, tables = [], [], [], []
    next_id = dropped = 0
    for a, b in zip(starts, starts[1:] + [n]):
        ra, rb = int(rows[a]), int(rows[b])
        r = T.run_clip(counts[a:b], boxes[ra:rb], None if emb is None else np.asarray(emb, F32)[ra:rb], iou_min, sim_min, max_age, lazy=True)
        tr = r["tracker"]
        track.append(np.where(r["track"] >= 0, r["track"] + next_id, -1).astype(np.int32))
        sim.append(r["sim"]), flag.append(r["flag"])
        tab = tr.table_array()
        tab[:, 0] += a
        tab[:, 1] += a
        if b < n:
            tab[:, 5] = -1                                      # the cut that follows ends every track of this shot
        tables.append(tab)
        next_id, dropped = next_id + tr.next_id, dropped + tr.dropped
    cat = lambda parts, dt, shape: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
    return {"track": cat(track, np.int32, 0), "sim": cat(sim, F32, 0), "flag": cat(flag, np.uint8, 0),
            "table": cat(tables, np.int32, (0, 8)), "next_id": next_id, "dropped": dropped, "frames_seen": n}


def cut_clips():
    """{name: (clip, cuts)} built from tests/track_ref.py's people: the windows are the tests' business"""
    e = lambda *people: [list(p) for p in people]
    out = {}
    # three people who stay where they are: without the cut they would be three tracks for the whole clip
    steady = T._people([[0, 1, 2]] * 10)
    z = np.zeros(10, np.uint8)
    for name, at in (("mid", [4]), ("first_of_window", [5]), ("last_of_window", [4]), ("clip_start", [0]), ("consecutive", [3, 4, 5]),
                     ("clip_start_and_mid", [0, 6])):
        c = z.copy()
        c[at] = 1
        out[name] = (T.make_clip(steady, iou_min=0.1, sim_min=0.4, max_age=3), c)
    # a cut at a frame without faces: the tracks end although max_age would have carried them over it
    gap = T._people(e([0, 1], [0, 1], [], [0, 1], [1, 0], [0]))
    out["faceless"] = (T.make_clip(gap, iou_min=0.1, sim_min=0.4, max_age=3), np.array([0, 0, 1, 0, 0, 0], np.uint8))
    # more than 64 detections on each side of a cut: the dropped count carries on
    rng = np.random.default_rng(8)
    crowd = T._people([rng.permutation(66).tolist(), rng.permutation(66).tolist(), rng.permutation(65).tolist(), rng.permutation(65).tolist()])
    out["crowd"] = (T.make_clip(crowd, iou_min=0.1, sim_min=0.4, max_age=3), np.array([0, 0, 1, 0], np.uint8))
    # one face per frame that drifts (sim 0 from frame to frame): the runs of the drift state machine, per shot
    drift = [[(T.person_boxes(0), T.onehot([t % 2])[0])] for t in range(60)]
    c = np.zeros(60, np.uint8)
    c[[20, 42]] = 1
    out["one_face_drift"] = (T.make_clip(drift), c)
    return out
