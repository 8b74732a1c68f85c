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


def iou_contracted(a, b, fused_area=None, fused_inter=True) -> np.float32:
    """NOT the tracker's IoU: what a compiler may make of iou() when it is free to contract (no -ffp-contract=off).  With
    ``fused_inter`` the denominator's subtraction takes w * h unrounded, fmaf(-w, h, area_a + area_b); with ``fused_area`` = 0 / 1
    the sum of the areas takes box a's / box b's area unrounded.  The dense clips' IoU gates stand on pairs for which every one of
    CONTRACTIONS differs from iou(), so that a build that contracts gives another answer."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    one = lambda v: F32(np.asarray(v).reshape(-1)[0])
    wa, ha, wb, hb = F32(a[2] - a[0]), F32(a[3] - a[1]), F32(b[2] - b[0]), F32(b[3] - b[1])
    area_a, area_b = F32(wa * ha), F32(wb * hb)
    w = max(F32(min(a[2], b[2]) - max(a[0], b[0])), F32(0))
    h = max(F32(min(a[3], b[3]) - max(a[1], b[1])), F32(0))
    total = F32(area_a + area_b) if fused_area is None else one(fma32(wa, ha, area_b)) if fused_area == 0 else one(fma32(wb, hb, area_a))
    return F32(F32(w * h) / (one(fma32(-w, h, total)) if fused_inter else F32(total - F32(w * h))))


CONTRACTIONS = ((None, True), (0, True), (1, True), (0, False), (1, False))      # (fused_area, fused_inter)


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
        self.ended = [None] * SLOTS           # per free slot the track that ageing ended there: the slot keeps its fields
        self.log = None                       # a list: every pair looked at, (frame, id, track row, det row, iou, sim | None, key | None)

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
                self.slots[s], self.ended[s] = None, t
        keys, by_id = {}, {t.id: t for t in self.slots if t is not None}
        for t in by_id.values():                                                # 2
            for d in range(nd):
                i = iou(t.box, boxes[d])
                s = self.sim_of(row0 + d, t.row) if self.sim_of is not None else None
                k = pair_key(i, s, self.sim_of is not None, self.iou_min, self.sim_min)
                if k is not None:
                    keys[(t.id, d)] = k
                if self.log is not None:
                    self.log.append((f, t.id, t.row, row0 + d, i, s, k))
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
            self.slots[s], self.ended[s] = t, None
            track[d] = t.id
        for s, t in enumerate(self.slots):                                      # 6
            if t is not None and t.last_frame == f:
                self._row(t, s)
        self.frames_seen += 1
        self.rows_seen += c
        return track, sim, flag

    def snapshot(self):
        """The state block's content after this frame, without embeddings: head [frames_seen, next_id, dropped, table_overflow],
        per slot [used, id, first_frame, last_frame, n_obs, run, hits, row] (row: the GLOBAL detection row whose embedding and n2
        are the slot's; a slot never used: zeros and row -1; a slot freed by ageing keeps the ended track's fields), and the boxes."""
        ints, box = np.zeros((SLOTS, 8), np.int64), np.zeros((SLOTS, 4), F32)
        ints[:, 7] = -1
        for s in range(SLOTS):
            t = self.slots[s] or self.ended[s]
            if t is not None:
                ints[s] = [self.slots[s] is not None, t.id, t.first_frame, t.last_frame, t.n_obs, t.run, t.hits, t.row]
                box[s] = t.box
        return {"head": [self.frames_seen, self.next_id, self.dropped, self.table_overflow], "slots": ints, "box": box}

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


def run_clip(counts, boxes, emb=None, iou_min=0.0, sim_min=-np.inf, max_age=INT32_MAX, table_cap=None, sims=None, lazy=False, record=False):
    """A whole clip -> dict(track, sim, flag arrays over the rows named by counts, tracker).  ``sims``: pair_sims(emb) computed
    before (shared between tests); rows past the sum of counts get -1 / 2.0 / 0.  ``record``: the tracker keeps its log of pairs,
    and "states"[k] is its snapshot() after k frames."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    m = len(boxes)
    if emb is not None and sims is None and not lazy:
        sims = pair_sims(emb)
    sim_of = (lambda d, t: sims[d, t]) if sims is not None else lazy_sims(emb) if emb is not None else None
    tr = Tracker(iou_min, sim_min, max_age, sim_of, table_cap)
    if record:
        tr.log = []
    states = [tr.snapshot()] if record else None
    track, sim, flag = np.full(m, -1, np.int32), np.full(m, NO_SIM, F32), np.zeros(m, np.uint8)
    off = 0
    for c in counts:
        c = int(c)
        t, s, fl = tr.frame(boxes[off:off + c])
        track[off:off + c], sim[off:off + c], flag[off:off + c] = t, s, fl
        off += c
        if record:
            states.append(tr.snapshot())
    return {"track": track, "sim": sim, "flag": flag, "tracker": tr, "states": states}


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


# ---- dense inputs: every element of an embedding non-zero, no box coordinate an integer --------------------------------------------
# Nothing here is exact by construction: the similarities and IoUs are whatever float32 gives, and the reference above is the
# judge.  tests/test_tracks_cpu.py holds the reference to float64 / rational arithmetic on these clips and asserts what each clip
# is meant to contain.  Person k has a unit base vector; a detection's embedding is (base + noise N(0, 1)/sqrt(512)) * scale, so two
# detections of one person have a similarity near 1 / (1 + noise^2) and two people one near 0; a power-of-two scale changes no
# similarity but moves the slot's n2 by orders of magnitude.  A clip also carries "person": the person of every row.
DENSE = ("dense8", "dense8_emb_off", "dense_crowd", "dense_drift")
GATES = (("dense8", "iou_min"), ("dense8", "sim_min"), ("dense8_emb_off", "iou_min"))
SIDES = ("below", "at", "above")
GATE_NAMES = tuple(f"{n}:{g}:{side}" for n, g in GATES for side in SIDES)
SCALES = (2.0 ** -20, 1.0, 2.0 ** 20)
DENSE8_ABSENT = {1: (3, 7, 8, 13, 14, 15), 4: (5, 10, 11, 17, 18, 19)}      # each misses 1, 2 and 3 consecutive frames
DENSE8_JUMP = (5, 12)                                                        # person 5 stands somewhere else from frame 12 on
DENSE8_STEP = {2: (0, -24), 3: (0, 24), 7: (24, 0)}                          # they make this step before every even frame
_CACHE = {}


def _unit(rng):
    v = rng.standard_normal(512)
    return v / np.linalg.norm(v)


def dense_row(rng, base, noise, scale):
    return ((base + noise * rng.standard_normal(512) / np.sqrt(512.0)) * scale).astype(F32)


def dense_box(rng, cx, cy, size):
    """A rectangle about (cx + 1/3, cy + 1/7), its sides within 3 % of `size`."""
    w, h = size * (1 + 0.03 * rng.uniform(-1, 1, 2))
    cx, cy = cx + 1 / 3, cy + 1 / 7
    return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], F32)


def _dense_clip(rng, frames_of_people, centre, base, noise, scale, size, **rules):
    """frames_of_people: per frame the people present; their order within the frame is shuffled here.  centre(k, t) -> (cx, cy),
    base(k, t) -> the person's unit vector at frame t, noise[k], scale[k]."""
    counts, boxes, emb, person = [], [], [], []
    for t, people in enumerate(frames_of_people):
        people = [people[i] for i in rng.permutation(len(people))]
        counts.append(len(people))
        for k in people:
            boxes.append(dense_box(rng, *centre(k, t), size))
            emb.append(dense_row(rng, base(k, t), noise[k], scale[k]))
            person.append(k)
    out = {"counts": np.array(counts, np.int32), "boxes": np.array(boxes, F32).reshape(-1, 4), "emb": np.array(emb, F32).reshape(-1, 512),
           "person": np.array(person, np.int64), "iou_min": 0.3, "sim_min": 0.4, "max_age": 2}
    out.update(rules)
    return out


def _drifting(rng, n, start, pair_speed, own_speed):
    """centre(k, t) of n people who stand in pairs (2j, 2j + 1): a pair drifts together, each of the two a little on its own."""
    v = np.repeat(rng.uniform(-pair_speed, pair_speed, ((n + 1) // 2, 2)), 2, axis=0)[:n] + rng.uniform(-own_speed, own_speed, (n, 2))
    return lambda k, t: (start(k)[0] + v[k, 0] * t, start(k)[1] + v[k, 1] * t)


def dense_cases():
    """{name: clip}, built once: the arrays are shared and read-only."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    c = {}
    # 8 people in four pairs of overlapping neighbours (22 of 60 pixels apart: an IoU near 0.45), 24 frames.  Everybody drifts by
    # under a pixel a frame (an IoU near 0.95 with the own last box); three people also step 24 pixels before every even frame:
    # matched pairs with an IoU below one half, the only ones whose bits a contracted denominator can change (above one half
    # area_a + area_b - inter is exact, and the unrounded w * h rounds back to it) -- the IoU gates stand on one of them.
    rng = np.random.default_rng(812)
    bases = [_unit(rng) for _ in range(8)]
    drift = _drifting(rng, 8, lambda k: (100 + 200 * (k // 2) + 22 * (k % 2), 400), 0.8, 0.15)
    jk, jt = DENSE8_JUMP
    step = lambda k, t, i: DENSE8_STEP.get(k, (0, 0))[i] * (t // 2)            # an IoU near 0.43 with the own last box
    centre = lambda k, t: (drift(k, t)[0] + step(k, t, 0), drift(k, t)[1] + step(k, t, 1) + (300 if k == jk and t >= jt else 0))
    frames = [[k for k in range(8) if t not in DENSE8_ABSENT.get(k, ())] for t in range(24)]
    c["dense8"] = _dense_clip(rng, frames, centre, lambda k, t: bases[k], [0.5] * 8, rng.permutation(np.resize(SCALES, 8)), 60.0)
    c["dense8_emb_off"] = dict(c["dense8"], emb=None, sim_min=-np.inf)
    # 66 people in each of 4 frames, rows of neighbours 24 of 50 pixels apart; then 40 strangers where people 0..39 stood
    rng = np.random.default_rng(6640)
    bases = [_unit(rng) for _ in range(106)]
    drift = _drifting(rng, 66, lambda k: (60 + 24 * (k % 11), 60 + 70 * (k // 11)), 0.5, 0.1)
    frames = [list(range(66))] * 4 + [list(range(66, 106))]
    c["dense_crowd"] = _dense_clip(rng, frames, lambda k, t: drift(k % 66, t), lambda k, t: bases[k], [0.5] * 106, rng.choice(SCALES, 106), 50.0)
    # 3 people, 40 frames: 0 steady (every sim >= 0.99), 1 with sims on both sides of 0.99f, 2 turning by 0.2 rad a frame
    # (every sim < 0.99).  0 and 1 overlap, so their cross pairs are looked at; sim_min = -inf admits them, the keys decide.
    rng = np.random.default_rng(340)
    bases = [_unit(rng) for _ in range(3)]
    other = _unit(rng)
    other = other - (other @ bases[2]) * bases[2]
    other /= np.linalg.norm(other)
    turn = lambda k, t: bases[k] if k < 2 else np.cos(0.2 * t) * bases[2] + np.sin(0.2 * t) * other
    drift = _drifting(rng, 3, lambda k: (100 + 22 * k + 300 * (k // 2), 100), 0.8, 0.15)
    c["dense_drift"] = _dense_clip(rng, [[0, 1, 2]] * 40, drift, turn, [0.05, 0.1005, 0.02], [1.0, SCALES[2], SCALES[0]], 60.0,
                                   sim_min=-np.inf)
    for clip in c.values():
        for v in clip.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    _CACHE["cases"] = c
    return c


def dense_clip(name):
    """A dense clip or one of its gate variants ("dense8:iou_min:above")."""
    base = name.split(":")[0]
    return dense_cases()[name] if name == base else gate_variants(base)[name]


def dense_sims(name):
    """pair_sims of the clip's embeddings (a gate variant has its clip's), computed once; None without embeddings."""
    base = name.split(":")[0]
    if ("sims", base) not in _CACHE:
        emb = dense_cases()[base]["emb"]
        _CACHE[("sims", base)] = None if emb is None else pair_sims(emb)
    return _CACHE[("sims", base)]


def dense_ref(name):
    """The reference's answer for a dense clip or gate variant, with the log of pairs and the state after every frame; computed
    once per session and never changed."""
    c = dense_clip(name)                                  # (building a clip's gate variants computes their references)
    if ("ref", name) not in _CACHE:
        r = run_clip(c["counts"], c["boxes"], c["emb"], c["iou_min"], c["sim_min"], c["max_age"], sims=dense_sims(name), record=True)
        for a in (r["track"], r["sim"], r["flag"]):
            a.setflags(write=False)
        _CACHE[("ref", name)] = r
    return _CACHE[("ref", name)]


def matched_pairs(ref):
    """The log entries of the pairs that were matched (a new track's id is not in its frame's log)."""
    return [e for e in ref["tracker"].log if e[6] is not None and ref["track"][e[3]] == e[1]]


def _gate_pair_works(refs, e):
    """At v and below it the pair (det row e[3], track row e[2]) matches and the two runs agree; above v it does not match and
    the clip has more tracks."""
    below, at, above = refs
    same = lambda r: r["track"][e[3]] == r["track"][e[2]]
    return (same(below) and same(at) and not same(above) and np.array_equal(below["track"], at["track"])
            and above["tracker"].next_id > at["tracker"].next_id)


def gate_variants(name):
    """{"name:gate:side": clip} for the gates of a dense clip: the gate set to v's lower neighbour, to v, and to v's upper
    neighbour, v being the gated value (iou for iou_min, sim for sim_min) of a pair that the reference's own run of the clip
    matches.  The pair is the one with the smallest v for which the three clips do what _gate_pair_works says -- and, for
    iou_min, whose IoU has other bits in every form of iou_contracted: a kernel built with contraction puts such a pair on the
    other side of the gate in the "at" or the "above" clip.  A variant carries "pair" = (det row, track row)."""
    if ("gates", name) not in _CACHE:
        c, out = dense_cases()[name], {}
        for gate in (g for n, g in GATES if n == name):
            col = 4 if gate == "iou_min" else 5
            for e in sorted(matched_pairs(dense_ref(name)), key=lambda e: (float(e[col]), e[3])):
                v = F32(e[col])
                boxes = c["boxes"][e[2]], c["boxes"][e[3]]
                if not 0 < v < 1 or (gate == "iou_min" and any(iou_contracted(*boxes, *form) == v for form in CONTRACTIONS)):
                    continue
                names = [f"{name}:{gate}:{side}" for side in SIDES]
                clips = [dict(c, **{gate: F32(value), "pair": (e[3], e[2])}) for value in (np.nextafter(v, F32(0)), v, np.nextafter(v, F32(1)))]
                refs = [run_clip(k["counts"], k["boxes"], k["emb"], k["iou_min"], k["sim_min"], k["max_age"], sims=dense_sims(name), record=True)
                        for k in clips]
                if _gate_pair_works(refs, e):
                    break
            else:
                raise AssertionError(f"{name}: no matched pair serves as the {gate} gate")
            for n, k, r in zip(names, clips, refs):
                for a in (r["track"], r["sim"], r["flag"]):
                    a.setflags(write=False)
                out[n], _CACHE[("ref", n)] = k, r
        _CACHE[("gates", name)] = out
    return _CACHE[("gates", name)]


def state_block(snap, emb):
    """The state block (csrc/trl_tracks.h: TrlTkHead, 64 TrlTkSlot, 64 embeddings) that Tracker.snapshot() stands for, as
    (bytes, compared): uint8 and bool arrays of STATE_BYTES.  Every byte is compared but the embedding blocks of slots freed by
    ageing, which keep whatever the ended track left there.  src is -1 in every slot after an update."""
    buf, compared = np.zeros(STATE_BYTES, np.uint8), np.ones(STATE_BYTES, bool)
    buf[:8].view(np.int64)[0] = snap["head"][0]
    buf[8:20].view(np.int32)[:] = snap["head"][1:]
    ints, rows = snap["slots"], snap["slots"][:, 7]
    words = buf[32:32 + 64 * SLOTS].view(np.int32).reshape(SLOTS, 16)
    words[:, :7] = ints[:, :7]
    words[:, 7] = -1
    words[:, 8:12] = np.asarray(snap["box"], F32).view(np.int32)
    if emb is not None:
        used, held = ints[:, 0] == 1, rows >= 0
        words[held, 12] = dot512(emb[rows[held]], emb[rows[held]]).view(np.int32)
        blocks = buf[32 + 64 * SLOTS:].view(F32).reshape(SLOTS, 512)
        blocks[used] = emb[rows[used]]
        compared[32 + 64 * SLOTS:].reshape(SLOTS, 2048)[held & ~used] = False
    return buf, compared
