"""Face quality on the GPU: how good is each detected face, and which frame shows a person best.

    q = face_quality(frames, frame_of, boxes, points)     # per face row: quality in [0, 1] and the measures behind it
    pool.add(emb, ids, weights=q["quality"])              # ... a weight for EmbeddingPool / FaceGallery.templates / FaceTracker

    best = BestShots(num_groups, face_shape=(3, 160, 160))
    best.add(q["quality"], ids, faces)                    # any number of calls
    best.read()                                           # per group: the best row seen, its quality, its face

Every measure is an integer sum over the source pixels of the face's rectangle or a short float chain of ``+ - * / sqrt`` in a
fixed order ("Face quality"; csrc/trl_quality.h is the rule's code, tests/quality_ref.py its reference), so a
result is the same bits for any banding, stream or workspace.  Per face row, on the u8 BGR frames:

    rectangle   X0 = clamp(floor(x1), 0, W), X1 = clamp(ceil(x2), 0, W), the same for y; no face (``status`` 0, every value 0) for
                a frame index outside 0 .. n - 1, a NaN or infinite coordinate or an empty rectangle
    luma        Y = (1868 B + 9617 G + 4899 R + 8192) >> 14                   OpenCV's 8-bit COLOR_BGR2GRAY as recalled: unpinned
    Laplacian   L = up + down + left + right - 4 centre, neighbours inside the rectangle by reflect-101
                                                                               cv2.Laplacian(ksize=1) as recalled: unpinned
    raw         (m, 8) int64: N, sum Y, sum Y^2, sum L, sum L^2, n_dark (Y <= 15), n_bright (Y >= 240), w;  hist (m, 256) int32
    sharpness   the variance of the Laplacian, float32(SL2 / N - (SL / N)^2) in float64
    mean_luma, dark_frac, bright_frac, contrast = p95 - p05 (p05: the smallest v with 20 cum(v) >= N; p95: >= 19 N)
    pose        RATIOS from the five O-Net points, no atan: iod the eye distance, roll = dy / iod of the eyes, yaw = 2 t - 1 with t
                the nose's position along the eye line (0 frontal, -1 / +1 the nose over an eye), pitch = 2 u - 1 with u its
                position along eye-mid -> mouth-mid; NaN for a non-finite point or coincident eyes, and without points
    quality     q_sharp * q_expo * q_pose * q_size: min(max(0, sharpness) / sharp_ref, 1); max(0, 1 - (dark_frac + bright_frac) / clip_ref)
                * min(contrast / contrast_ref, 1); max(0, 1 - |yaw| / yaw_ref) * max(0, 1 - |pitch| / pitch_ref) (0 for a NaN pose, 1
                without points); min(min(w, h) / size_ref, 1)

The defaults of ``QualityParams`` are PLACEHOLDERS, not calibrated figures: no labelled set of good and bad faces has been
measured.  A row without a face has quality 0, which ``EmbeddingPool`` skips (and counts) as a weight."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._tensors import cuda_device, grown, ptr, stream, table, vector

FEATURES = ("quality", "sharpness", "mean_luma", "dark_frac", "bright_frac", "contrast", "yaw", "pitch", "roll", "iod", "p05", "p95")
RAW = ("n", "sum_y", "sum_y2", "sum_l", "sum_l2", "n_dark", "n_bright", "width")
MAX_DIM = 16384


@dataclass(frozen=True)
class QualityParams:
    """The references of the composite (csrc/trl_quality.h).  PLACEHOLDERS, not calibrated figures.  Each is a divisor: finite
    and > 0."""
    sharp_ref: float = 100.0          # variance of the Laplacian that counts as fully sharp
    clip_ref: float = 0.5             # fraction of clipped pixels at which the exposure term reaches 0
    contrast_ref: float = 64.0        # p95 - p05 that counts as full contrast
    yaw_ref: float = 1.0              # |yaw| at which the pose term reaches 0
    pitch_ref: float = 1.0
    size_ref: float = 80.0            # min(w, h) in source pixels that counts as full size

    def __post_init__(self):
        for k, v in self.__dict__.items():
            if not (np.isfinite(np.float32(v)) and np.float32(v) > 0):
                raise ValueError(f"QualityParams.{k} must be finite and > 0, not {v!r}")

    def _struct(self) -> _lib.TrlQualityParams:
        return _lib.TrlQualityParams(*(float(getattr(self, n)) for n, _ in _lib.TrlQualityParams._fields_))


def face_quality(frames, frame_of, boxes, points=None, params: QualityParams | None = None, return_hist: bool = False,
                 max_band_rows: int = 0, device=None, _workspace: torch.Tensor | None = None) -> dict:
    """``frames`` (n, H, W, 3) uint8 BGR, ``frame_of`` (m,) the frame of each face row (-1: none), ``boxes`` (m, 4) x1, y1, x2, y2,
    ``points`` (m, 10) x0..x4, y0..y4 or None -- the rows of ``Engine.extract_faces(keep_all=True, quality=True)``.  Returns device
    tensors: ``quality``, ``sharpness``, ``mean_luma``, ``dark_frac``, ``bright_frac``, ``contrast``, ``yaw``, ``pitch``, ``roll``,
    ``iod`` (m,) float32 (views of ``feat`` (m, 12), which also holds p05 and p95), ``raw`` (m, 8) int64, ``status`` (m,) int32 and,
    with ``return_hist``, ``hist`` (m, 256) int32.  ``max_band_rows`` is a test knob: every value gives the same bits.  No
    synchronisation."""
    lib = _lib.load()
    if device is None:
        device = frames.device if isinstance(frames, torch.Tensor) and frames.device.type == "cuda" else None
    device = cuda_device(device, "embeddings are pooled on a GPU")
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 (n, H, W, 3) BGR")
    fr = frames.to(device).contiguous()
    n, H, W, _ = fr.shape
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError(f"frames of {H} x {W}: H and W must be in 1 .. {MAX_DIM}")
    if int(max_band_rows) < 0:
        raise ValueError("max_band_rows must be 0 (the library's choice) or positive")
    boxes = table(boxes, 4, device, "boxes")
    m = boxes.shape[0]
    frame_of = vector(frame_of, m, torch.int32, device, "frame_of")
    if points is not None:
        points = table(points, 10, device, "points")
        if points.shape[0] != m:
            raise ValueError(f"points must have {m} rows, not {points.shape[0]}")
    params = params or QualityParams()
    prm = params._struct()
    need = lib.trl_quality_workspace(m)
    if not need:
        raise ValueError(f"at most 2**24 face rows, not {m}")
    ws = torch.empty((need // 8,), dtype=torch.int64, device=device) if _workspace is None else _workspace
    raw = torch.empty((m, 8), dtype=torch.int64, device=device)
    feat = torch.empty((m, 12), dtype=torch.float32, device=device)
    status = torch.empty((m,), dtype=torch.int32, device=device)
    hist = torch.empty((m, 256), dtype=torch.int32, device=device) if return_hist else None
    _lib.check(lib.trl_face_quality(ptr(fr), n, H, W, ptr(frame_of), ptr(boxes), ptr(points), m, C.byref(prm), int(max_band_rows),
                                    ptr(ws), ws.numel() * ws.element_size(), ptr(raw), ptr(feat), ptr(hist), ptr(status),
                                    stream(device)))
    out = {name: feat[:, i] for i, name in enumerate(FEATURES[:10])}
    out.update(feat=feat, raw=raw, status=status)
    if return_hist:
        out["hist"] = hist
    return out


class BestShots:
    """Per group 0 .. num_groups - 1 the best row seen: the largest quality, ties to the earlier row, NaN never.  Rows arrive in
    any number of ``add`` calls; a row's index is its absolute position over all calls (``rows_seen`` is kept on the host, so no
    call synchronises).  With faces, the best row's face is kept beside it."""

    def __init__(self, num_groups: int, device=None, face_shape=None):
        self.lib = _lib.load()
        self.device = cuda_device(device, "embeddings are pooled on a GPU")
        if not (0 <= int(num_groups) <= 2 ** 31 - 1):
            raise ValueError(f"num_groups must be in 0 .. 2**31 - 1, not {num_groups}")
        self.num_groups = int(num_groups)
        self.rows_seen = 0
        self.face_shape = None if face_shape is None else tuple(int(v) for v in face_shape)
        self._keys = torch.zeros((max(self.num_groups, 1),), dtype=torch.int64, device=self.device)
        self._faces = None
        self._alloc_faces()

    def _alloc_faces(self):
        if self.face_shape is not None:
            self._faces = torch.zeros((max(self.num_groups, 1),) + self.face_shape, dtype=torch.float32, device=self.device)

    def reset(self) -> None:
        """Forget every row (the faces' storage is kept: a group without a best row has no face to speak of)."""
        self._keys.zero_()
        self.rows_seen = 0

    def grow(self, num_groups: int) -> None:
        """Make room for groups up to ``num_groups - 1``: a device copy; the new groups have no best row."""
        g = self.num_groups
        if int(num_groups) < g:
            raise ValueError(f"{g} groups cannot shrink to {int(num_groups)}")
        if int(num_groups) == g:
            return
        self.num_groups = int(num_groups)
        self._keys = grown(self._keys[:g], self.num_groups)
        if self._faces is not None:
            self._faces = grown(self._faces[:g], self.num_groups)

    def add(self, quality, gid, faces=None) -> None:
        """m more rows: ``quality`` (m,) float32, ``gid`` (m,) integer group ids (outside 0 .. num_groups - 1: ignored), ``faces``
        (m, *face_shape) float32 or None.  The first call's faces give ``face_shape`` when the constructor did not."""
        q = torch.as_tensor(quality).detach().to(self.device, torch.float32).reshape(-1).contiguous()
        m = q.shape[0]
        gid = vector(gid, m, torch.int32, self.device, "gid")
        if self.rows_seen + m > 2 ** 31 - 1:
            raise ValueError("BestShots takes at most 2**31 - 1 rows")
        floats = 0
        if faces is not None:
            faces = torch.as_tensor(faces).detach().to(self.device, torch.float32).contiguous()
            if self.face_shape is None and self.rows_seen == 0:
                self.face_shape = tuple(faces.shape[1:])
                self._alloc_faces()
            if self.face_shape is None or faces.shape[0] != m or tuple(faces.shape[1:]) != self.face_shape:
                raise ValueError(f"faces must be ({m}, *{self.face_shape}) from the first row on, got {tuple(faces.shape)}")
            floats = int(np.prod(self.face_shape))
        elif self._faces is not None and m:
            raise ValueError("these BestShots keep faces: every add needs them")
        _lib.check(self.lib.trl_best_update(ptr(self._keys), self.num_groups, ptr(q), ptr(gid), m, self.rows_seen,
                                            ptr(faces if floats else None), floats, ptr(self._faces if floats and m else None),
                                            stream(self.device)))
        self.rows_seen += m

    def read(self) -> dict:
        """``row`` (G,) int32 (-1: none), ``quality`` (G,) float32 (NaN: none) and, with faces, ``face`` (G, *face_shape): device
        tensors; the face of a group without a best row is whatever its slot held (zeros on a fresh object)."""
        g, d = self.num_groups, self.device
        row = torch.empty((g,), dtype=torch.int32, device=d)
        quality = torch.empty((g,), dtype=torch.float32, device=d)
        _lib.check(self.lib.trl_best_read(ptr(self._keys), g, ptr(row), ptr(quality), stream(d)))
        out = {"row": row, "quality": quality}
        if self._faces is not None:
            out["face"] = self._faces[:g]
        return out
