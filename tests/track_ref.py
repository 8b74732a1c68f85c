"""Reference of the face tracker (trl_track_update / trl_track_scores, csrc/trl_tracks.h) and the built clips its tests share.
numpy / Python only: no GPU, no oracle.

The rules ("Tracks").  An update takes a window of n consecutive sampled frames of one clip: ``counts[n]``,
and the window's detections as flat rows, frame by frame: ``boxes[m][4]`` (x1, y1, x2, y2) and optionally ``emb[m][512]``.  Frame t
of the window has absolute index ``frames_seen + t``.  A tracker has 64 slots; track ids are 0, 1, 2, ... in order of creation over
the clip; a frame's detections past its first 64 get track -1 and add to ``dropped``.

    dot512   per lane l an 8-step fmaf chain over elements l + 64 i, then the xor butterfly 32..1 of plain float32 adds
    sim      dot512(det, trk) / (sqrt(dot512(det, det)) * sqrt(dot512(trk, trk))), trk = the track's last matched detection
    iou      torchvision's order in float32: area = (x2-x1)*(y2-y1); w = max(min(x2,x2')-max(x1,x1'), 0), h likewise;
             inter = w*h; iou = inter / (area + area' - inter)

Per frame f, in order:
 1. ageing: a track is live iff f - last_frame - 1 <= max_age; the others end and free their slots
 2. a (live track, detection) pair is admissible iff (iou_min <= 0 or iou >= iou_min) and (no embeddings or sim >= sim_min), in
    float32, NaN failing both; its key is sim with embeddings, iou without; a NaN key is never admissible
 3. greedy matching: repeatedly the admissible pair of an unmatched track and an unmatched detection with the largest key, ties to
    the lower track id, then the lower detection index (-0 == +0)
 4. a matched track takes the detection's box and embedding, last_frame = f, n_obs += 1, and with embeddings makes one step of
    model.py's state machine with the pair's sim (run = run + 1 if sim < 0.99f else 0; run > 15: hits += 1, flag = 1); the
    detection's output sim is the pair's, 2.0 without embeddings
 5. unmatched detections in ascending index each start a track with the next id, in the free slot of the lowest index, else in the
    slot of the track not matched or created in this frame with the smallest last_frame (ties: smallest id), which ends; output
    sim 2.0, flag 0
 6. every track touched writes its table row {first_frame, last_frame, n_obs, run, hits, slot (-1 once ended), 0, 0}

A track's score is drift_ref.score(hits, run, frame_count, fps); the clip's is the maximum, at the lowest id among equals.
"""
from __future__ import annotations

import numpy as np

import drift_ref as D
from front_ref import fma32

F32 = np.float32
SLOTS = 64
NO_SIM = F32(2.0)
INT32_MAX = 2 ** 31 - 1
STATE_BYTES = 135200
# the state's header as int32 words (csrc/trl_tracks.h: TrlTkHead): frames_seen is words 0-1
HEAD_NEXT_ID, HEAD_DROPPED, HEAD_TABLE_OVERFLOW = 2, 3, 4
_LANE = np.arange(64)


# ---- arithmetic -------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf for float32 arrays; where an operand or the result is not finite, the plain expression (NaN and inf come out the same
    under any rounding, and front_ref.fma32 is defined for finite values only)."""
    with np.errstate(all="ignore"):
        plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
        ok = np.isfinite(plain) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
        out = plain.copy()
        if ok.any():
            out[ok] = fma32(a[ok], b[ok], c[ok])
    return out


def dot512(a, b):
    """trl_wave_dot512 for (k, 512) float32 arrays (or two rows) -> (k,) float32."""
    a = np.asarray(a, F32).reshape(-1, 512)
    b = np.asarray(b, F32).reshape(-1, 512)
    s = np.zeros((len(a), 64), F32)
    for i in range(8):
        s = _fma(a[:, 64 * i:64 * i + 64], b[:, 64 * i:64 * i + 64], s)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            s = (s + s[:, _LANE ^ off]).astype(F32)
    return s[:, 0]


def cosine(dot, n2a, n2b):
    with np.errstate(all="ignore"):
        return F32(F32(dot) / F32(np.sqrt(F32(n2a)) * np.sqrt(F32(n2b))))


def pair_sims(emb):
    """All detection-pair similarities of a clip, (m, m) float32: [i, j] = sim(det i, trk j)."""
    emb = np.asarray(emb, F32)
    m = len(emb)
    n2 = dot512(emb, emb)
    out = np.empty((m, m), F32)
    for i in range(m):
        d = dot512(np.broadcast_to(emb[i], (m, 512)), emb)
        with np.errstate(all="ignore"):
            out[i] = d / (np.sqrt(n2[i]) * np.sqrt(n2))
    return out


def iou(a, b) -> np.float32:
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(all="ignore"):
        area_a = F32(F32(a[2] - a[0]) * F32(a[3] - a[1]))
        area_b = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
        x1, y1 = (a[0] if a[0] > b[0] else b[0]), (a[1] if a[1] > b[1] else b[1])
        x2, y2 = (a[2] if a[2] < b[2] else b[2]), (a[3] if a[3] < b[3] else b[3])
        w, h = F32(x2 - x1), F32(y2 - y1)
        w = w if w > 0 else F32(0)
        h = h if h > 0 else F32(0)
        inter = F32(w * h)
        return F32(inter / F32(F32(area_a + area_b) - inter))


def pair_key(iou_v, sim, has_emb, iou_min, sim_min):
    """The key, or None when the pair is not admissible."""
    iou_min, sim_min = F32(iou_min), F32(sim_min)
    if not (iou_min <= 0 or iou_v >= iou_min):
        return None
    if not has_emb:
        return None if np.isnan(iou_v) else F32(iou_v)
    return F32(sim) if sim >= sim_min else None


def greedy(keys):
    """keys: {(track id, det): key}, admissible pairs only -> {det: track id}."""
    match, left = {}, dict(keys)
    while left:
        # the largest key (+0 == -0 as floats), then the lower id, then the lower detection
        t, d = min(left, key=lambda p: (-float(left[p]) + 0.0, p[0], p[1]))
        match[d] = t
        left = {p: k for p, k in left.items() if p[0] != t and p[1] != d}
    return match


# ---- the tracker ------------------------------------------------------------------------------------------------------------------
class Track:
    def __init__(self, tid, slot, f, box, row):
        self.id, self.slot, self.first_frame, self.last_frame = tid, slot, f, f
        self.n_obs, self.run, self.hits = 1, 0, 0
        self.box, self.row = np.asarray(box, F32), row


class Tracker:
    """The rules, one frame at a time.  ``sim_of(det_row, trk_row)`` gives a pair's similarity from GLOBAL detection rows (rows are
    numbered over the whole clip), or is None for the embeddings-off mode."""

    def __init__(self, iou_min, sim_min, max_age, sim_of=None, table_cap=None):
        self.iou_min, self.sim_min, self.max_age, self.sim_of = F32(iou_min), F32(sim_min), int(max_age), sim_of
        self.table_cap = table_cap
        self.slots = [None] * SLOTS
        self.frames_seen = self.next_id = self.dropped = self.table_overflow = self.rows_seen = 0
        self.table = {}                       # id -> [first_frame, last_frame, n_obs, run, hits, slot, 0, 0]
        self.evicted = []                     # ids in the order eviction ended them

    def _row(self, t, slot):
        if self.table_cap is None or t.id < self.table_cap:
            self.table[t.id] = [t.first_frame, t.last_frame, t.n_obs, t.run, t.hits, slot, 0, 0]

    def frame(self, boxes):
        """One frame with these detections -> (track, sim, flag) per detection."""
        f, row0 = self.frames_seen, self.rows_seen
        c = len(boxes)
        nd = min(c, SLOTS)
        track, sim, flag = [-1] * c, [NO_SIM] * c, [0] * c
        self.dropped += c - nd
        for s, t in enumerate(self.slots):                                      # 1
            if t is not None and not (f - t.last_frame - 1 <= self.max_age):
                self._row(t, -1)
                self.slots[s] = None
        keys, by_id = {}, {t.id: t for t in self.slots if t is not None}
        for t in by_id.values():                                                # 2
            for d in range(nd):
                i = iou(t.box, boxes[d])
                s = self.sim_of(row0 + d, t.row) if self.sim_of is not None else None
                k = pair_key(i, s, self.sim_of is not None, self.iou_min, self.sim_min)
                if k is not None:
                    keys[(t.id, d)] = k
        match = greedy(keys)                                                    # 3
        for d, tid in match.items():                                            # 4
            t = by_id[tid]
            t.box, t.row, t.last_frame, t.n_obs = np.asarray(boxes[d], F32), row0 + d, f, t.n_obs + 1
            track[d] = tid
            if self.sim_of is not None:
                k = keys[(tid, d)]
                t.run = t.run + 1 if k < F32(D.THR_SIM) else 0
                if t.run > D.THR_FRAMES:
                    t.hits += 1
                    flag[d] = 1
                sim[d] = k
        for d in range(nd):                                                     # 5
            if d in match:
                continue
            free = [s for s, t in enumerate(self.slots) if t is None]
            if free:
                s = free[0]
            else:
                old = min((t for t in self.slots if t.last_frame != f), key=lambda t: (t.last_frame, t.id))
                s = old.slot
                self._row(old, -1)
                self.evicted.append(old.id)
            t = Track(self.next_id, s, f, boxes[d], row0 + d)
            self.next_id += 1
            if self.table_cap is not None and t.id >= self.table_cap:
                self.table_overflow += 1
            self.slots[s] = t
            track[d] = t.id
        for s, t in enumerate(self.slots):                                      # 6
            if t is not None and t.last_frame == f:
                self._row(t, s)
        self.frames_seen += 1
        self.rows_seen += c
        return track, sim, flag

    def table_array(self, cap=None):
        cap = self.next_id if cap is None else cap
        out = np.zeros((cap, 8), np.int32)
        for i, r in self.table.items():
            if i < cap:
                out[i] = r
        return out

    def scores(self, frame_count, fps, cap=None):
        """-> (score per row of a table of `cap` rows, summary [clip score, its id, next_id, dropped])."""
        cap = self.next_id if cap is None else cap
        tab = self.table_array(cap)
        sc = np.zeros(cap, np.int32)
        for i in range(min(cap, self.next_id)):
            sc[i] = D.score(int(tab[i, 4]), int(tab[i, 3]), frame_count, fps)[0]
        k = min(cap, self.next_id)
        best = int(np.argmax(sc[:k])) if k else -1
        return sc, [int(sc[best]) if k else 0, best, self.next_id, self.dropped]


def lazy_sims(emb):
    """sim_of(det row, track row) that computes a pair when it is first asked for: for clips with few pairs per frame."""
    emb = np.asarray(emb, F32)
    n2, seen = dot512(emb, emb), {}

    def sim_of(d, t):
        if (d, t) not in seen:
            seen[(d, t)] = cosine(dot512(emb[d], emb[t])[0], n2[d], n2[t])
        return seen[(d, t)]
    return sim_of


def run_clip(counts, boxes, emb=None, iou_min=0.0, sim_min=-np.inf, max_age=INT32_MAX, table_cap=None, sims=None, lazy=False):
    """A whole clip -> dict(track, sim, flag arrays over the rows named by counts, tracker).  ``sims``: pair_sims(emb) computed
    before (shared between tests); rows past the sum of counts get -1 / 2.0 / 0."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    m = len(boxes)
    if emb is not None and sims is None and not lazy:
        sims = pair_sims(emb)
    sim_of = (lambda d, t: sims[d, t]) if sims is not None else lazy_sims(emb) if emb is not None else None
    tr = Tracker(iou_min, sim_min, max_age, sim_of, table_cap)
    track, sim, flag = np.full(m, -1, np.int32), np.full(m, NO_SIM, F32), np.zeros(m, np.uint8)
    off = 0
    for c in counts:
        c = int(c)
        t, s, fl = tr.frame(boxes[off:off + c])
        track[off:off + c], sim[off:off + c], flag[off:off + c] = t, s, fl
        off += c
    return {"track": track, "sim": sim, "flag": flag, "tracker": tr}


# ---- built inputs: every similarity exact, every IoU a known fraction --------------------------------------------------------------
def onehot(idx, scale=1.0):
    """(len(idx), 512) rows with one non-zero element each: rows with equal idx have similarity exactly 1, others exactly 0."""
    idx = np.asarray(idx, np.int64)
    e = np.zeros((len(idx), 512), F32)
    e[np.arange(len(idx)), idx] = scale
    return e


def dyadic(a, b, i=0, j=1):
    """A row a e_i + b e_j with small integers a, b: dots and squared norms are exact integers."""
    e = np.zeros(512, F32)
    e[i], e[j] = a, b
    return e


def grid_box(x, y, w=10, h=10):
    return [float(x), float(y), float(x + w), float(y + h)]


def person_boxes(k):
    """Box of person k on a grid where different people never overlap: IoU exactly 1 with itself and 0 with any other."""
    return grid_box(20 * (k % 16), 20 * (k // 16))


def make_clip(frames, emb_off=False, **rules):
    """frames: per frame a list of (box, embedding row).  -> dict(counts, boxes, emb | None, iou_min, sim_min, max_age)."""
    counts = np.array([len(fr) for fr in frames], np.int32)
    rows = [r for fr in frames for r in fr]
    boxes = np.array([r[0] for r in rows], F32).reshape(-1, 4)
    emb = None if emb_off else np.array([r[1] for r in rows], F32).reshape(-1, 512)
    out = {"counts": counts, "boxes": boxes, "emb": emb, "iou_min": 0.0, "sim_min": -np.inf, "max_age": INT32_MAX}
    out.update(rules)
    return out


def _people(frames_of_people, size=None):
    """frames_of_people: per frame the people in detection order.  Person k: one-hot row k, box person_boxes(k); ``size(k, t)``
    widens the box (an IoU below 1 with the person's own last box, still 0 with everybody else's)."""
    out = []
    for t, people in enumerate(frames_of_people):
        fr = []
        for k in people:
            b = person_boxes(k)
            if size is not None:
                b = [b[0], b[1], b[0] + size(k, t), b[1] + size(k, t)]
            fr.append((b, onehot([k])[0]))
        out.append(fr)
    return out


def cases():
    """{name: clip}: the built clips of tests/test_tracks_cpu.py (the host build of trl_tracks.h) and tests/test_gpu_tracks.py."""
    nan = float("nan")
    c = {}
    # two and three people whose largest face (the first row of a frame: detect's order) alternates
    big = lambda k, t: 10 + 2 * ((k + t) % 2)                       # 10 or 12 wide: IoU 100/144 with the own last box
    c["alternate2"] = make_clip(_people([[0, 1] if t % 2 else [1, 0] for t in range(24)], big), iou_min=0.1, sim_min=0.4, max_age=3)
    c["alternate3"] = make_clip(_people([[(t + i) % 3 for i in range(3)] for t in range(24)], big), iou_min=0.1, sim_min=0.4, max_age=3)
    c["alternate2_emb_off"] = make_clip(_people([[0, 1] if t % 2 else [1, 0] for t in range(24)], big), emb_off=True, iou_min=0.1, max_age=3)
    # crossing: from frame 3 on each of two people stands in the other's last box -- the IoU says "swap", the similarity "stay"
    e0, e1 = onehot([0])[0], onehot([1])[0]
    a, b = grid_box(0, 0), grid_box(6, 0)                           # IoU 40/160 with each other
    cross = [[(a, e0), (b, e1)]] * 3 + [[(b, e0), (a, e1)]] * 3 + [[(a, e0), (b, e1)]] * 2
    c["crossing_sim"] = make_clip(cross)                                # key = sim: the tracks follow the embeddings
    c["crossing_iou"] = make_clip(cross, emb_off=True)                  # key = iou: the tracks follow the boxes
    c["crossing_gate"] = make_clip(cross, iou_min=0.5, sim_min=0.5)     # the pair with the right face fails the IoU test: new tracks
    c["crossing_sim_min"] = make_clip(cross, sim_min=0.5, iou_min=0.2)
    # ties: equal embeddings and equal boxes -- every key is equal, the lower track id takes the lower detection
    same = (grid_box(0, 0), e0)
    c["ties"] = make_clip([[same] * 2, [same] * 3, [same] * 5, [same] * 2, [same] * 5], max_age=0)
    c["ties_emb_off"] = make_clip([[same] * 2, [same] * 3, [same] * 5, [same] * 2, [same] * 5], emb_off=True, max_age=0)
    # dyadic rows: sims 1, 0.6, 0.8, 0 exactly up to the rounding both sides share; two detections prefer the same track
    d34, d43 = dyadic(3, 4), dyadic(4, 3)
    c["dyadic"] = make_clip([[(a, dyadic(5, 0)), (b, dyadic(0, 5))], [(a, d34), (b, d43)], [(b, d43), (a, d34)], [(a, dyadic(1, 0))]])
    # rows that are never admissible: a NaN element, a zero row, (without embeddings) a zero-area box against itself
    bad = np.zeros(512, F32)
    bad_nan = onehot([0])[0].copy(); bad_nan[9] = nan
    flat = [5.0, 5.0, 5.0, 9.0]
    c["never"] = make_clip([[(a, e0), (b, bad), (grid_box(40, 0), bad_nan)]] * 4)
    c["never_zero_area"] = make_clip([[(a, e0), (flat, e1)]] * 4, emb_off=True)
    c["never_zero_area_gate"] = make_clip([[(a, e0), (flat, e1)]] * 4, iou_min=0.25)
    # ageing: person 0 is missed for exactly max_age frames (the track goes on) and then for max_age + 1 (a new track)
    for name, age in (("age0", 0), ("age2", 2), ("age_never", INT32_MAX)):
        k = min(age, 2)
        seq = [[0, 1]] + [[1]] * k + [[0, 1]] + [[1]] * (k + 1) + [[0, 1], [], [], [0], []] + [[]] * 3 + [[1, 0]]
        c[name] = make_clip(_people(seq), iou_min=0.1, sim_min=0.4, max_age=age)
    c["all_empty"] = make_clip([[]] * 5, max_age=1)
    # slots: 64 faces in every frame, in another order each time
    rng = np.random.default_rng(5)
    c["crowd64"] = make_clip(_people([rng.permutation(64).tolist() for _ in range(3)]), iou_min=0.1, sim_min=0.4, max_age=3)
    c["counts_63_64_65"] = make_clip(_people([rng.permutation(n).tolist() for n in (63, 64, 65, 66, 63)]), iou_min=0.1, sim_min=0.4, max_age=3)
    c["counts_emb_off"] = make_clip(_people([rng.permutation(n).tolist() for n in (65, 63, 64)]), emb_off=True, iou_min=0.1, max_age=3)
    # a crowd that turns over: 0..63, then 32..63 only, then 40 strangers: the tracks last seen at frame 0 go first, by id
    c["turnover"] = make_clip(_people([list(range(64)), list(range(32, 64))[::-1], list(range(100, 140)), list(range(140, 204))]),
                          iou_min=0.1, sim_min=0.4)
    # three people held by their boxes; the second and third change their face in every frame (sim exactly 0: 39 drift steps, 24
    # hits each) -- per-track scores that differ, and two equal ones for the clip's "lowest id among equals"
    steady = [[(person_boxes(0), e0), (person_boxes(1), onehot([10 + t % 2])[0]), (person_boxes(2), onehot([20 + t % 2])[0])]
              for t in range(40)]
    c["drifters"] = make_clip(steady, iou_min=0.5)
    # a slot reused after ageing
    c["slot_reuse"] = make_clip(_people([[0, 1], [1], [1, 0], [], [1, 0, 2]]), iou_min=0.1, sim_min=0.4, max_age=0)
    return c
