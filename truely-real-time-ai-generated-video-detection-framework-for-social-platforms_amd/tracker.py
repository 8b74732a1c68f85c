"""Face tracks on the GPU: which face of this sampled frame is which face of the last one, and the drift score per person.

    trk = FaceTracker(iou_min=0.1, sim_min=0.4, max_age=3)
    for window in clip:                                           # consecutive windows of ONE clip
        d = engine.extract_faces(window, keep_all=True)
        out = trk.update(d["box"], d["counts"], engine.facenet_embed(d["faces"].permute(0, 2, 3, 1)))
    trk.tracks(frame_count, fps)                                  # per track: id, first_frame, last_frame, n_obs, run, hits, score
    trk.score(frame_count, fps)                                   # the clip's multi-face score: the maximum over its tracks

``FaceTracker(templates=True)`` also pools every track's embeddings into one exact template (pool.py): ``trk.templates()``, and
``trk.identify_tracks(gallery)`` names each track once instead of each frame.  ``FaceTracker(best_shots=True)`` keeps, per track,
the row of the largest ``quality`` (quality.py) and its face: ``trk.best_shots()``, the thumbnail of a report or an enrolment.
``update(..., cuts=)`` takes the cut flags of a ``ShotDetector`` (shots.py) and ends every track at a shot boundary: a track is
one person in ONE shot.  ``Engine.track_faces(frames, tracker)`` is the three calls of the loop body.  ``run()`` / ``analyze_video`` do not use this: they
keep the reference's largest-face drift (``Engine.drift_update``), in which two people in one clip read as drift.

The rules ("Tracks"; csrc/trl_tracks.h is their code, tests/track_ref.py their reference).  One update takes a
window of n consecutive sampled frames: ``counts[n]`` and the window's detections as flat rows, frame by frame in detect's order --
``boxes[m][4]`` (x1, y1, x2, y2) and optionally ``emb[m][512]`` -- the layout of ``extract_faces(keep_all=True)``.  Frame t of the
window has absolute index ``frames_seen + t``.  A tracker has 64 slots; track ids are 0, 1, 2, ... in order of creation over the
clip; a frame's detections past its first 64 get track -1 and are counted as dropped.

    sim    the drift kernels' cosine: dot512(det, trk) / (sqrtf(dot512(det, det)) * sqrtf(dot512(trk, trk))), dot512 one wave's
           fmaf chains and xor butterfly; trk is the embedding of the track's last matched detection
    iou    torchvision's box_iou in float32, one rounding per operation

Per frame f, in order:
 1. ageing: a track is live iff ``f - last_frame - 1 <= max_age`` (``2**31 - 1``: always); the others end, their slots are free
 2. a (live track, detection) pair is admissible iff ``iou_min <= 0 or iou >= iou_min`` and, with embeddings, ``sim >= sim_min``
    (float32; NaN fails both; ``sim_min = -inf`` passes everything but NaN).  Its key is sim with embeddings, iou without.
 3. greedy matching: repeatedly the admissible pair of an unmatched track and an unmatched detection with the largest key; ties to
    the lower track id, then the lower detection index
 4. a matched track takes the detection's box and embedding, ``last_frame = f``, ``n_obs += 1``, and with embeddings makes one
    step of model.py's state machine with the pair's sim: ``run = run + 1 if sim < 0.99f else 0; run > 15: hits += 1, flag = 1``.
    The detection's ``sim`` is the pair's (2.0 without embeddings).
 5. unmatched detections, in ascending index, each start a track with the next id in the free slot of the lowest index -- without
    one, in the slot of the track not matched or created in this frame with the smallest last_frame (ties: smallest id), which
    ends.  Output ``sim = 2.0`` ("no comparison", the drift kernels' sentinel), ``flag = 0``.
 6. every track touched writes its row of the track table

A track's score is model.py:86-95 with the track's run and hits and the clip's frame_count and fps; the clip's is the maximum.  A
clip with at most one face per frame, ``iou_min = 0``, ``sim_min = -inf``, ``max_age = 2**31 - 1`` and no NaN similarity has one
track with, bit for bit, ``Engine.drift_update``'s sims, flags, run, hits and score.

The defaults of ``iou_min``, ``sim_min`` and ``max_age`` are PLACEHOLDERS, not calibrated figures: no real checkpoint has been
measured.  ``FaceGallery.calibrate`` on labelled embeddings of the checkpoint in use is the way to a ``sim_min``."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._tensors import cuda_device, grown, ptr, stream, table, vector

SLOTS = 64
STATE_BYTES = 135200
INT32_MAX = 2 ** 31 - 1
TABLE_COLUMNS = ("first_frame", "last_frame", "n_obs", "run", "hits", "slot")


class FaceTracker:
    """The tracks of ONE clip (``reset()`` starts another).  State, table and outputs live on the device; ``update`` queues one
    kernel on the current stream and does not synchronise."""

    def __init__(self, iou_min: float = 0.1, sim_min: float = 0.4, max_age: int = 3, device=None, templates: bool = False,
                 best_shots: bool = False):
        if not (0 <= int(max_age) <= INT32_MAX):
            raise ValueError("max_age must be in 0 .. 2**31 - 1")
        if np.isnan(iou_min) or np.isnan(sim_min):
            raise ValueError("iou_min / sim_min must not be NaN")
        self.iou_min, self.sim_min, self.max_age = float(iou_min), float(sim_min), int(max_age)
        self.lib = _lib.load()
        self.device = cuda_device(device, "a FaceTracker lives on a GPU")
        self._state = torch.zeros((STATE_BYTES // 8,), dtype=torch.int64, device=self.device)
        self._table = torch.zeros((256, 8), dtype=torch.int32, device=self.device)
        self._id_bound = 0                                # next_id <= this: a row starts at most one track
        self._pool = None
        if templates:                                     # one pooled template per track id (pool.py); it grows with the table
            from .pool import EmbeddingPool
            self._pool = EmbeddingPool(self._table.shape[0], self.device)
        self._best = None
        if best_shots:                                    # the best row per track id (quality.py); it grows with the table too
            from .quality import BestShots
            self._best = BestShots(self._table.shape[0], self.device)

    def reset(self) -> None:
        """Forget the clip: the next update is a clip's first window.  No synchronisation."""
        self._state.zero_()
        self._table.zero_()
        self._id_bound = 0
        if self._pool is not None:
            self._pool.reset()
        if self._best is not None:
            self._best.reset()

    def update(self, boxes, counts, emb=None, weights=None, quality=None, faces=None, cuts=None) -> dict:
        """The clip's next window: ``boxes`` (m, 4), ``counts`` (n,), ``emb`` (m, 512) or None (every window of a clip alike).
        -> ``track`` (m,) int32, ``sim`` (m,) float32, ``flag`` (m,) uint8 on the device.  A tracker made with ``templates=True``
        needs ``emb`` and then pools the window's rows by the track ids just written (rows without a track are ignored), each
        weighed by ``weights`` (m,) in (0, 1] -- ``face_quality``'s ``quality``, for one -- or 1.  A tracker made with
        ``best_shots=True`` needs ``quality`` (m,) for every window and keeps, per track id, the row of the largest quality and --
        when ``faces`` (m, 3, S, S) come with every window -- that row's face.  ``cuts`` (n,) uint8 -- ``ShotDetector.update``'s
        ``cut`` -- ends every track at the frames it flags, before ageing and pairing, exactly as an aged-out track ends; the
        frame's faces all start new tracks.  None: no cuts."""
        if self._best is None and (quality is not None or faces is not None):
            raise ValueError("quality and faces belong to the best shots: make the tracker with best_shots=True")
        if self._best is not None and quality is None:
            raise ValueError("a tracker with best_shots=True needs the quality of every window")
        if self._pool is None and weights is not None:
            raise ValueError("weights belong to the templates: make the tracker with templates=True")
        if self._pool is not None and emb is None:
            raise ValueError("a tracker with templates=True needs the embeddings of every window")
        d = self.device
        boxes = table(boxes, 4, d, "boxes")
        counts = torch.as_tensor(counts).to(d, torch.int32).reshape(-1).contiguous()
        m, n = boxes.shape[0], counts.shape[0]
        if emb is not None:
            emb = torch.as_tensor(emb).to(d, torch.float32).contiguous()
            if tuple(emb.shape) != (m, 512):
                raise ValueError(f"expected ({m}, 512) embeddings, got {tuple(emb.shape)}")
        cuts = vector(cuts, n, torch.uint8, d, "cuts")
        if self._id_bound + m > self._table.shape[0]:    # grow geometrically; the copy stays on the device
            self._table = grown(self._table, max(2 * self._table.shape[0], self._id_bound + m))
        self._id_bound += m
        track = torch.empty((m,), dtype=torch.int32, device=d)
        sim = torch.empty((m,), dtype=torch.float32, device=d)
        flag = torch.empty((m,), dtype=torch.uint8, device=d)
        _lib.check(self.lib.trl_track_update_cuts(ptr(self._state), ptr(boxes), ptr(counts), ptr(cuts), n, m,
                                                  ptr(emb), self.iou_min, self.sim_min,
                                                  self.max_age, ptr(track), ptr(sim), ptr(flag), ptr(self._table), self._table.shape[0],
                                                  stream(self.device)))
        if self._pool is not None:
            if self._pool.num_groups < self._table.shape[0]:
                self._pool.grow(self._table.shape[0])
            self._pool.add(emb, track, weights)
        if self._best is not None:
            if self._best.num_groups < self._table.shape[0]:
                self._best.grow(self._table.shape[0])
            if faces is not None and faces.dim() == 4 and faces.permute(0, 2, 3, 1).is_contiguous():
                faces = faces.permute(0, 2, 3, 1)          # (extract_faces' view of NHWC rows: kept as they lie, without a copy)
                self._best_nhwc = True
            elif faces is not None:
                self._best_nhwc = False
            self._best.add(quality, track, faces)
        return {"track": track, "sim": sim, "flag": flag}

    def _num_tracks(self) -> int:
        """The number of tracks created so far: one synchronisation."""
        cap = self._table.shape[0]
        score = torch.empty((cap,), dtype=torch.int32, device=self.device)
        summary = torch.empty((4,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.trl_track_scores(ptr(self._state), ptr(self._table), cap, 1, 1, ptr(score), ptr(summary), stream(self.device)))
        return int(summary[2].item())

    def templates(self, unit: bool = True) -> dict:
        """``templates=True``: the pooled embeddings of the clip's tracks so far, ``EmbeddingPool.result``'s dict with row = track
        id -- ``template``, ``count``, ``weight``, ``cohesion`` (1: every frame of the track the same face; low: a contaminated
        track), ``skipped``.  The bits are ``pool_embeddings(all rows, all track ids)``', however the clip was cut into windows.
        One synchronisation (the number of tracks)."""
        if self._pool is None:
            raise ValueError("make the tracker with templates=True")
        r, n = self._pool.result(unit), self._num_tracks()
        return {k: (v if k == "skipped" else v[:n]) for k, v in r.items()}

    def best_shots(self) -> dict:
        """``best_shots=True``: per track of the clip so far, ``track`` (T,) its id, ``row`` (T,) int32 the absolute detection row
        over the clip -- the rows of every update, in order -- with the largest quality (ties: the earlier row; -1: no row with a
        quality that is not NaN), ``quality`` (T,) that quality (NaN for none) and, when the updates brought faces, ``face``
        (T, 3, S, S), that row's face.  However the clip was cut into windows.  One synchronisation (the number of tracks)."""
        if self._best is None:
            raise ValueError("make the tracker with best_shots=True")
        r, n = self._best.read(), self._num_tracks()
        out = {"track": torch.arange(n, dtype=torch.int32, device=self.device), "row": r["row"][:n], "quality": r["quality"][:n]}
        if "face" in r:
            out["face"] = r["face"][:n].permute(0, 3, 1, 2) if getattr(self, "_best_nhwc", False) else r["face"][:n]
        return out

    def identify_tracks(self, gallery, threshold: float | None = None):
        """"Who is track 3?", once per track: ``gallery.identify`` of the tracks' templates -> (labels, score), entry = track id;
        a track without a contributing row is None."""
        t = self.templates()
        return gallery.identify(t["template"], threshold, valid=t["count"] > 0)

    def _scores(self, frame_count: int, fps: int) -> np.ndarray:
        """[summary (4), table rows (bound x 8), scores (bound)] as one host array: one synchronisation."""
        cap, k = self._table.shape[0], self._id_bound
        score = torch.empty((cap,), dtype=torch.int32, device=self.device)
        summary = torch.empty((4,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.trl_track_scores(ptr(self._state), ptr(self._table), cap, int(frame_count), int(fps), ptr(score),
                                             ptr(summary), stream(self.device)))
        return torch.cat([summary, self._table[:k].reshape(-1), score[:k]]).cpu().numpy()

    def tracks(self, frame_count: int, fps: int) -> dict:
        """Every track of the clip so far, as host arrays indexed by track id: ``id``, ``first_frame``, ``last_frame``, ``n_obs``,
        ``run``, ``hits``, ``slot`` (-1 once ended), ``score``; and ``clip_score``, ``clip_track`` (-1 without a track),
        ``dropped``.  One synchronisation."""
        a, k = self._scores(frame_count, fps), self._id_bound
        n = int(a[2])
        table, score = a[4:4 + 8 * k].reshape(k, 8)[:n], a[4 + 8 * k:][:n]
        out = {"id": np.arange(n, dtype=np.int32), "score": score.copy()}
        out.update({name: table[:, c].copy() for c, name in enumerate(TABLE_COLUMNS)})
        out.update(clip_score=int(a[0]), clip_track=int(a[1]), dropped=int(a[3]))
        return out

    def score(self, frame_count: int, fps: int) -> int:
        """The clip's multi-face score: the maximum of its tracks' scores, 0 without a track.  One synchronisation."""
        return int(self._scores(frame_count, fps)[0])
