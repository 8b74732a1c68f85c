"""Shot boundaries on the GPU: where does the scene change, so that a face track is one person in ONE shot.

    det = ShotDetector()
    trk = FaceTracker()
    for window in clip:                                   # consecutive windows of ONE clip, frames already on the device
        s = det.update(window)                            # sig (n, 16, 3, 32), dist (n,), cut (n,), shot (n,): device tensors
        trk.update(box, counts, emb, cuts=s["cut"])       # ... or Engine.track_faces(window, trk, shots=det) for both

Every quantity is an integer count or one double division ("Shots"; csrc/trl_shots.h is the rule's code,
tests/shots_ref.py its reference), so a result is the same bits for any banding, stream, workspace or split of a clip into windows.

    signature   of a frame u8 (H, W, 3), channels as stored, 4 <= H, W <= 16384: ``sig[16][3][32]`` int32.  Region r = 4 i + j covers
                rows H i // 4 .. H (i + 1) // 4 - 1 and columns W j // 4 .. W (j + 1) // 4 - 1; ``sig[r][c][v >> 3] += 1`` for every
                pixel of the region and every channel c
    distance    per region the 1-D earth mover's distance in bins, d_r = sum_c sum_{k < 31} |Ca[c][k] - Cb[c][k]| over the cumulative
                counts; the regions by (d_r, r) ascending, the first 16 - drop kept (the most-changed regions are a moving person,
                not a cut); dist = float32(float64(sum of kept d_r) / float64(sum of kept 93 N_r)) in [0, 1]
    cuts        dist of a clip's first frame is 2.0 ("no comparison"); ``cut[t] = dist[t] != 2.0 and dist[t] >= threshold and
                t - last_cut >= min_shot`` (the first cut is never suppressed); ``shot[t]`` = the cuts at frames <= t

NOT detected: dissolves and fades (no two consecutive frames are far apart); a flash cuts at its first frame, and only ``min_shot``
keeps its last frame from cutting again.  The defaults of ``ShotParams`` are PLACEHOLDERS, not calibrated figures: no labelled set
of edited clips has been measured.  ``run()`` / ``analyze_video`` do not use this: they keep the reference's semantics."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._tensors import cuda_device, ptr, stream

MIN_DIM, MAX_DIM, MAX_FRAMES = 4, 16384, 65535
STATE_BYTES = 6176
SIG_SHAPE = (16, 3, 32)


@dataclass(frozen=True)
class ShotParams:
    """The cut rule's parameters (csrc/trl_shots.h).  PLACEHOLDERS, not calibrated figures."""
    threshold: float = 0.12           # dist at and above which a frame starts a shot
    drop: int = 4                     # most-changed regions left out of the distance, 0 .. 15
    min_shot: int = 1                 # frames a shot lasts at least

    def __post_init__(self):
        if not np.isfinite(np.float32(self.threshold)):
            raise ValueError(f"ShotParams.threshold must be finite, not {self.threshold!r}")
        if not 0 <= int(self.drop) <= 15:
            raise ValueError(f"ShotParams.drop must be in 0 .. 15, not {self.drop!r}")
        if not 1 <= int(self.min_shot) <= 2 ** 31 - 1:
            raise ValueError(f"ShotParams.min_shot must be >= 1, not {self.min_shot!r}")

    def _struct(self) -> _lib.TrlShotsParams:
        return _lib.TrlShotsParams(float(self.threshold), int(self.drop), int(self.min_shot))


def _check_dims(H: int, W: int) -> None:
    if not (MIN_DIM <= H <= MAX_DIM and MIN_DIM <= W <= MAX_DIM):
        raise ValueError(f"frames of {H} x {W}: H and W must be in {MIN_DIM} .. {MAX_DIM}")


def frame_signatures(frames, max_band_rows: int = 0, device=None, _workspace: torch.Tensor | None = None) -> torch.Tensor:
    """``frames`` (n, H, W, 3) uint8 -> (n, 16, 3, 32) int32 on the device.  A device tensor is read where it lies -- a contiguous
    view at any byte offset included -- and a host array is uploaded.  ``max_band_rows`` is a test knob: every value gives the same
    bits.  No synchronisation."""
    lib = _lib.load()
    if device is None:
        device = frames.device if isinstance(frames, torch.Tensor) and frames.device.type == "cuda" else None
    device = cuda_device(device, "frame signatures are computed on a GPU")
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be uint8 (n, H, W, 3)")
    fr = frames.to(device).contiguous()
    n, H, W, _ = fr.shape
    _check_dims(H, W)
    if n > MAX_FRAMES:
        raise ValueError(f"at most {MAX_FRAMES} frames a call, not {n}")
    if int(max_band_rows) < 0:
        raise ValueError("max_band_rows must be 0 (the library's choice) or positive")
    need = lib.trl_shots_workspace(n, H, W, int(max_band_rows))
    ws = torch.empty((need // 8,), dtype=torch.int64, device=device) if _workspace is None else _workspace
    sig = torch.empty((n,) + SIG_SHAPE, dtype=torch.int32, device=device)
    _lib.check(lib.trl_frame_signatures(ptr(fr), n, H, W, int(max_band_rows), ptr(ws), ws.numel() * ws.element_size(), ptr(sig),
                                        stream(device)))
    return sig


def _signatures(x, device) -> torch.Tensor:
    x = torch.as_tensor(x).to(device, torch.int32)
    if x.dim() < 3 or tuple(x.shape[-3:]) != SIG_SHAPE:
        raise ValueError(f"signatures must be (..., 16, 3, 32), got {tuple(x.shape)}")
    return x.reshape((-1,) + SIG_SHAPE).contiguous()


def signature_distance(a, b, H: int, W: int, drop: int = 4) -> torch.Tensor:
    """Row i of ``a`` against row i of ``b`` -- (p, 16, 3, 32) int32 signatures of H x W frames -> (p,) float32 in [0, 1]."""
    lib = _lib.load()
    device = a.device if isinstance(a, torch.Tensor) and a.device.type == "cuda" else None
    device = cuda_device(device, "frame signatures are compared on a GPU")
    a, b = _signatures(a, device), _signatures(b, device)
    if a.shape != b.shape:
        raise ValueError(f"{a.shape[0]} signatures against {b.shape[0]}")
    _check_dims(int(H), int(W))
    if not 0 <= int(drop) <= 15:
        raise ValueError(f"drop must be in 0 .. 15, not {drop!r}")
    dist = torch.empty((a.shape[0],), dtype=torch.float32, device=device)
    _lib.check(lib.trl_signature_distance(ptr(a), ptr(b), a.shape[0], int(H), int(W), int(drop), ptr(dist), stream(device)))
    return dist


class ShotDetector:
    """The shots of ONE clip (``reset()`` starts another).  The state -- the last signature, the frames seen, the last cut, the
    cuts so far -- lives on the device; ``update`` queues its kernels on the current stream and does not synchronise."""

    def __init__(self, params: ShotParams | None = None, device=None):
        self.params = params or ShotParams()
        self.lib = _lib.load()
        self.device = cuda_device(device, "a ShotDetector lives on a GPU")
        self._state = torch.zeros((STATE_BYTES // 8,), dtype=torch.int64, device=self.device)
        self._size = None

    def reset(self) -> None:
        """Forget the clip: the next update is a clip's first window.  No synchronisation."""
        self._state.zero_()
        self._size = None

    def update(self, frames, max_band_rows: int = 0) -> dict:
        """The clip's next window, (n, H, W, 3) uint8 (n = 0 is legal) -> ``sig`` (n, 16, 3, 32) int32, ``dist`` (n,) float32,
        ``cut`` (n,) uint8, ``shot`` (n,) int32 on the device.  Raises if the frame size is not the clip's."""
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dim() != 4:
            raise ValueError("frames must be uint8 (n, H, W, 3)")
        size = (int(frames.shape[1]), int(frames.shape[2]))
        if self._size is not None and size != self._size:
            raise ValueError(f"frames of {size[0]} x {size[1]} in a clip of {self._size[0]} x {self._size[1]}: reset() starts another clip")
        sig = frame_signatures(frames, max_band_rows, self.device)
        self._size = size
        n, d = sig.shape[0], self.device
        dist = torch.empty((n,), dtype=torch.float32, device=d)
        cut = torch.empty((n,), dtype=torch.uint8, device=d)
        shot = torch.empty((n,), dtype=torch.int32, device=d)
        prm = self.params._struct()
        _lib.check(self.lib.trl_shots_update(ptr(self._state), ptr(sig), n, size[0], size[1], C.byref(prm), ptr(dist), ptr(cut), ptr(shot),
                                             stream(d)))
        return {"sig": sig, "dist": dist, "cut": cut, "shot": shot}


def detect_shots(frames, params: ShotParams | None = None, window: int = 256, device=None) -> dict:
    """A whole clip (n, H, W, 3) uint8, taken ``window`` frames at a time -> ``dist``, ``cut``, ``shot`` (n,) device tensors."""
    if int(window) < 1:
        raise ValueError("window must be >= 1")
    det = ShotDetector(params, device)
    outs = [det.update(frames[i:i + int(window)]) for i in range(0, len(frames), int(window))] or [det.update(frames)]
    return {k: torch.cat([o[k] for o in outs]) for k in ("dist", "cut", "shot")}
