"""Persistent device context of the hot path: weights uploaded once, workspaces reused.

The reference rebuilds ``MTCNN()`` and ``InceptionResnetV1(pretrained="vggface2")`` on every
``run()`` call (server/model.py:18-19); here an :class:`Engine` is created once per GPU and shared
by :class:`mtcnn.MTCNN`, :class:`inception_resnet_v1.InceptionResnetV1` and :func:`model.run`.
PyTorch is used for device memory and streams only; every kernel is in libtruely_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import weights as _weights


# trl_select_faces methods / trl_extract_faces resamplers (include/truely_hip.h)
SELECTION_METHODS = {"largest": 0, "probability": 1, "largest_over_threshold": 2, "center_weighted_size": 3}
RESAMPLERS = {"torch": 0, "pil": 1, "cv2": 2}


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Engine:
    def __init__(self, blob: bytes | None = None, device: int | None = None, pnet_mode: int | None = None,
                 cap_level: int | None = None, cap_frame: int | None = None, min_face_size: int = 20,
                 thresholds=(0.6, 0.7, 0.7), factor: float = 0.709, max_faces: int = 64, embed_mode: int = 0,
                 embed_precision: str | int = 0):
        if not torch.cuda.is_available():
            raise RuntimeError("truely_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.lib = _lib.load()
        cfg = _lib.TrlConfig()
        _lib.check(self.lib.trl_default_config(C.byref(cfg)))
        cfg.device = torch.cuda.current_device() if device is None else int(device)
        cfg.min_face_size = int(min_face_size)
        cfg.thr0, cfg.thr1, cfg.thr2 = (float(t) for t in thresholds)
        cfg.factor = float(factor)
        cfg.max_faces = int(max_faces)
        cfg.embed_mode = int(embed_mode)
        cfg.embed_precision = {"f32": 0, "fp32": 0, "bf16": 1, "fp16": 2, "f16": 2}.get(embed_precision, embed_precision) if isinstance(embed_precision, str) else int(embed_precision)
        if pnet_mode is not None:
            cfg.pnet_mode = int(pnet_mode)
        if cap_level:
            cfg.cap_level = int(cap_level)
        if cap_frame:
            cfg.cap_frame = int(cap_frame)
        self.cfg = cfg
        self.device = torch.device("cuda", cfg.device)
        h = C.c_void_p()
        _lib.check(self.lib.trl_create(C.byref(cfg), C.byref(h)))
        self._h = h
        if blob is None:
            blob = _weights.synthetic_blob(0)   # no checkpoints exist offline
        self._blob = blob
        self._pending = None                 # (outputs, frames) of the call queued by detect_embed_begin
        _lib.check(self.lib.trl_load_weights(self._h, blob, len(blob)))

    def clone(self) -> "Engine":
        """A second context on the same device with the same weights and configuration (its own workspaces: contexts are the
        unit of concurrency -- one batch in flight each)."""
        c = self.cfg
        return Engine(self._blob, device=c.device, pnet_mode=c.pnet_mode, cap_level=c.cap_level, cap_frame=c.cap_frame,
                      min_face_size=c.min_face_size, thresholds=(c.thr0, c.thr1, c.thr2), factor=c.factor, max_faces=c.max_faces,
                      embed_mode=c.embed_mode, embed_precision=c.embed_precision)

    def close(self):
        for name in ("_embedder", "_run_ctx"):            # contexts / buffers cached on this engine by pipeline.Overlapped / model.run
            o = self.__dict__.pop(name, None)
            if o is not None and hasattr(o, "close"):
                o.close()
        if getattr(self, "_h", None):
            self.lib.trl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _frames(self, frames) -> torch.Tensor:
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 (n, H, W, 3) BGR")
        return frames.to(self.device, non_blocking=True).contiguous()

    # server/model.py:47 for a batch
    def mtcnn_detect(self, frames, landmarks: bool = False, select_largest: bool = True):
        """(boxes [n,max_faces,4], probs [n,max_faces], counts [n]) and, with ``landmarks=True``, points [n,max_faces,10]
        (x0..x4, y0..y4) as the fourth element -- `mtcnn.detect(frame, landmarks=True)`.  ``select_largest=False``: the boxes in
        detect_face's order (descending score) instead of largest area first."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        mf = self.cfg.max_faces
        boxes = torch.empty((n, mf, 4), dtype=torch.float32, device=self.device)
        probs = torch.empty((n, mf), dtype=torch.float32, device=self.device)
        counts = torch.empty((n,), dtype=torch.int32, device=self.device)
        if not select_largest:
            points = torch.empty((n, mf, 10), dtype=torch.float32, device=self.device) if landmarks else None
            _lib.check(self.lib.trl_mtcnn_detect_ordered(self._h, _ptr(fr), n, H, W, 1, _ptr(boxes), _ptr(probs), _ptr(points),
                                                         _ptr(counts), self._stream()))
            return (boxes, probs, counts, points) if landmarks else (boxes, probs, counts)
        if landmarks:
            points = torch.empty((n, mf, 10), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.trl_mtcnn_detect_landmarks(self._h, _ptr(fr), n, H, W, _ptr(boxes), _ptr(probs), _ptr(points),
                                                           _ptr(counts), self._stream()))
            return boxes, probs, counts, points
        _lib.check(self.lib.trl_mtcnn_detect(self._h, _ptr(fr), n, H, W, _ptr(boxes), _ptr(probs), _ptr(counts), self._stream()))
        return boxes, probs, counts

    # facenet-pytorch MTCNN.select_boxes on detect's output (device tensors as mtcnn_detect returns them)
    def select_faces(self, boxes: torch.Tensor, probs: torch.Tensor, counts: torch.Tensor, H: int, W: int, method: str = "largest",
                     threshold: float = 0.9, center_weight: float = 2.0) -> torch.Tensor:
        """pick [n] int32: the slot of the box select_boxes keeps in each frame, -1 for none.  boxes [n,max_faces,4], probs
        [n,max_faces], counts [n] in detect's order; ties go to the last tied box.  No host synchronisation."""
        mf = self.cfg.max_faces
        boxes = boxes.to(self.device, torch.float32).contiguous()
        probs = probs.to(self.device, torch.float32).contiguous()
        counts = counts.to(self.device, torch.int32).contiguous()
        n = counts.shape[0]
        if tuple(boxes.shape) != (n, mf, 4) or tuple(probs.shape) != (n, mf):
            raise ValueError(f"boxes / probs must be ({n}, {mf}, 4) / ({n}, {mf})")
        pick = torch.empty((n,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.trl_select_faces(self._h, n, _ptr(boxes), _ptr(probs), _ptr(counts), int(H), int(W), SELECTION_METHODS[method],
                                             float(threshold), float(center_weight), _ptr(pick), self._stream()))
        return pick

    # facenet-pytorch extract_face for given boxes: faces [m, 3, S, S] f32 (a view of NHWC storage) + status [m] (1 face, 0 frame
    # index -1, -1 empty crop)
    def extract_boxes(self, frames, frame_of: torch.Tensor, boxes: torch.Tensor, image_size: int = 160, margin: int = 0,
                      resample: str = "torch", post_process: bool = True):
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        frame_of = frame_of.to(self.device, torch.int32).contiguous()
        boxes = boxes.to(self.device, torch.float32).reshape(-1, 4).contiguous()
        m, S = frame_of.shape[0], int(image_size)
        if boxes.shape[0] != m:
            raise ValueError("one box per row of frame_of")
        out = torch.empty((m, S, S, 3), dtype=torch.float32, device=self.device)
        status = torch.empty((m,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.trl_extract_faces(self._h, _ptr(fr), n, H, W, _ptr(frame_of), _ptr(boxes), m, S, int(margin),
                                              RESAMPLERS[resample], int(bool(post_process)), _ptr(out), _ptr(status), self._stream()))
        return out.permute(0, 3, 1, 2), status

    def extract_faces(self, frames, image_size: int = 160, margin: int = 0, resample: str = "torch", post_process: bool = True,
                      keep_all: bool = False, select_largest: bool = True, selection_method: str | None = None, quality: bool = False,
                      quality_params=None) -> dict:
        """facenet-pytorch ``MTCNN(image_size, margin, post_process, select_largest, selection_method, keep_all)(frames)`` for a
        batch, device-resident.  resample: the input kind crop_resize sees ('torch' tensor, 'pil' image, 'cv2' numpy array).
        Returns device tensors: ``faces`` [m, 3, S, S] f32 (a permuted view of NHWC rows, the layout facenet_embed reads),
        ``frame`` [m] (frame of each row, -1 for none), ``box`` [m, 4], ``prob`` [m], ``status`` [m] (1 face, 0 none, -1 empty crop:
        the library raises), and ``valid`` [n] uint8 (keep_all=False: row i is frame i) or ``counts`` [n] (keep_all=True: the
        rows of every face, frame by frame in detect's order).  keep_all=False makes no host synchronisation after detect's;
        keep_all=True makes one, for the number of faces.  ``quality=True``: detection runs with landmarks, and the dict gains
        ``points`` [m, 10] and ``face_quality``'s entries for the rows (quality.py: ``quality`` [m] in [0, 1], ``sharpness``, ...,
        ``feat``, ``raw``; its ``status`` as ``quality_status``); a row without a face has quality 0."""
        fr = self._frames(frames)
        n = fr.shape[0]
        H, W = fr.shape[1], fr.shape[2]
        points = None
        if quality:
            boxes, probs, counts, points = self.mtcnn_detect(fr, landmarks=True, select_largest=select_largest)
        else:
            boxes, probs, counts = self.mtcnn_detect(fr, select_largest=select_largest)
        d = self.device
        if keep_all:
            total = int(counts.sum().item())                  # the one synchronisation: the face count sizes the outputs
            c64 = counts.long()
            frame = torch.repeat_interleave(torch.arange(n, device=d), c64, output_size=total)
            slot = torch.arange(total, device=d) - (torch.cumsum(c64, 0) - c64)[frame]
            box, prob, frame_of = boxes[frame, slot], probs[frame, slot], frame.int()
            pts = points[frame, slot] if quality else None
        else:
            method = selection_method or ("largest" if select_largest else "probability")
            pick = self.select_faces(boxes, probs, counts, H, W, method)
            idx, rows = pick.clamp(min=0).long(), torch.arange(n, device=d)
            box, prob = boxes[rows, idx], probs[rows, idx]
            frame_of = torch.where(pick >= 0, rows.int(), torch.full_like(pick, -1))
            pts = points[rows, idx] if quality else None
        faces, status = self.extract_boxes(fr, frame_of, box, image_size, margin, resample, post_process)
        out = {"faces": faces, "frame": frame_of, "box": box, "prob": prob, "status": status}
        if keep_all:
            out["counts"] = counts
        else:
            out["valid"] = (status == 1).to(torch.uint8)
        if quality:
            q = self.face_quality(fr, frame_of, box, pts, params=quality_params)
            q["quality_status"] = q.pop("status")
            out["points"] = pts
            out.update(q)
        return out

    def face_quality(self, frames, frame_of, boxes, points=None, params=None, return_hist: bool = False, max_band_rows: int = 0) -> dict:
        """``quality.face_quality`` on this engine's device: per face row (frame_of [m], boxes [m, 4], points [m, 10] or None) the
        quality in [0, 1] and its measures -- sharpness, exposure, pose, size -- as device tensors.  No synchronisation."""
        from .quality import face_quality
        return face_quality(self._frames(frames), frame_of, boxes, points, params, return_hist, max_band_rows, self.device)

    def track_faces(self, frames, tracker, quality: bool = False, shots=None, **extract_kwargs) -> dict:
        """Every face of a window of sampled frames, embedded and associated with the clip's tracks: ``extract_faces(frames,
        keep_all=True, **extract_kwargs)``, ``facenet_embed`` of its faces, ``tracker.update(box, counts, emb)`` (a
        :class:`~truely_amd.tracker.FaceTracker` that has seen the clip's earlier windows).  Returns the extraction's dict plus
        ``emb`` [m, 512], ``track`` [m], ``sim`` [m], ``flag`` [m].  ``quality=True``: the extraction measures every face
        (``extract_faces(quality=True)``) and its ``quality`` goes to the tracker -- as the rows' weights when it keeps templates,
        and with the faces when it keeps best shots.  ``shots``: a :class:`~truely_amd.shots.ShotDetector` that has seen the
        clip's earlier windows -- ``shots.update(frames)`` runs on the same stream, its ``cut`` goes to the tracker (every track
        ends at a shot boundary) and ``dist``, ``cut``, ``shot`` [n] join the dict.  No synchronisation either way."""
        cut = {}
        if shots is not None:
            frames = self._frames(frames)                 # (uploaded once for both)
            cut = shots.update(frames)
            cut.pop("sig")
        if not quality:
            out = self.extract_faces(frames, keep_all=True, **extract_kwargs)
            emb = self.facenet_embed(out["faces"].permute(0, 2, 3, 1))
            out["emb"] = emb
            out.update(tracker.update(out["box"], out["counts"], emb, cuts=cut.get("cut")))
            out.update(cut)
            return out
        out = self.extract_faces(frames, keep_all=True, quality=True, **extract_kwargs)
        emb = self.facenet_embed(out["faces"].permute(0, 2, 3, 1))
        out["emb"] = emb
        has_best = getattr(tracker, "_best", None) is not None
        out.update(tracker.update(out["box"], out["counts"], emb, weights=out["quality"] if tracker._pool is not None else None,
                                  quality=out["quality"] if has_best else None, faces=out["faces"] if has_best else None,
                                  cuts=cut.get("cut")))
        out.update(cut)
        return out

    # server/model.py:59 for a batch; faces f32 (n, h, w, 3) NHWC in [0,1]
    def facenet_embed(self, faces: torch.Tensor) -> torch.Tensor:
        faces = faces.to(self.device, torch.float32).contiguous()
        n, h, w, _ = faces.shape
        emb = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_facenet_embed(self._h, _ptr(faces), n, h, w, _ptr(emb), self._stream()))
        return emb

    # InceptionResnetV1(classify=True): the trunk up to last_bn, then the checkpoint's logits layer
    @property
    def num_classes(self) -> int:
        """Classes of the loaded checkpoint's logits layer; 0 when the blob holds none."""
        c = C.c_int(0)
        _lib.check(self.lib.trl_facenet_num_classes(self._h, C.byref(c)))
        return int(c.value)

    def facenet_features(self, faces: torch.Tensor, valid: torch.Tensor | None = None) -> torch.Tensor:
        """(n, 512): what ``F.normalize`` and ``logits`` read (last_bn's output); zero rows where ``valid`` is 0."""
        faces = faces.to(self.device, torch.float32).contiguous()
        if valid is not None:
            valid = valid.to(self.device, torch.uint8).contiguous()
        n, h, w, _ = faces.shape
        feat = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_facenet_features(self._h, _ptr(faces), _ptr(valid), n, h, w, _ptr(feat), self._stream()))
        return feat

    def facenet_logits(self, feat: torch.Tensor) -> torch.Tensor:
        """(n, C) = feat @ W + b in f32, one fma chain over ascending k per logit."""
        feat = feat.to(self.device, torch.float32).contiguous()
        if feat.dim() != 2 or feat.shape[1] != 512:
            raise ValueError("expected (n, 512) features")
        n, nc = feat.shape[0], self.num_classes
        out = torch.empty((n, nc), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_facenet_logits(self._h, _ptr(feat), n, _ptr(out), nc, self._stream()))
        return out

    def _call_outputs(self, n: int, crop: bool, faces: torch.Tensor | None = None, valid: torch.Tensor | None = None) -> dict:
        """The outputs of a detect_embed (``emb``) / detect_crop (``faces``) call on n frames: new tensors, or the caller's
        ``faces`` / ``valid`` (checked)."""
        d = self.device
        out = {"box": torch.empty((n, 4), dtype=torch.float32, device=d), "prob": torch.empty((n,), dtype=torch.float32, device=d),
               "rect": torch.empty((n, 4), dtype=torch.int32, device=d)}
        if valid is None:
            valid = torch.empty((n,), dtype=torch.uint8, device=d)
        elif valid.shape != (n,) or valid.dtype != torch.uint8 or not valid.is_contiguous():
            raise ValueError("valid must be a contiguous uint8 (n,) tensor")
        out["valid"] = valid
        if crop:
            S = 80 if self.cfg.embed_mode == 0 else 160
            if faces is None:
                faces = torch.empty((n, S, S, 3), dtype=torch.float32, device=d)
            elif faces.shape != (n, S, S, 3) or faces.dtype != torch.float32 or not faces.is_contiguous():
                raise ValueError(f"faces must be a contiguous float32 ({n}, {S}, {S}, 3) tensor")
            out["faces"] = faces
        else:
            out["emb"] = torch.empty((n, 512), dtype=torch.float32, device=d)
        return out

    # server/model.py:47-59 for a batch of sampled frames
    def detect_embed(self, frames):
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        out = self._call_outputs(n, crop=False)
        _lib.check(self.lib.trl_detect_embed(self._h, _ptr(fr), n, H, W, _ptr(out["box"]), _ptr(out["prob"]), _ptr(out["rect"]),
                                             _ptr(out["valid"]), _ptr(out["emb"]), self._stream()))
        return out

    # detect_embed / detect_crop split into "queue" and "finish" (trl_detect_embed_begin / _end): one host thread can keep
    # several engines busy, each on its own stream, without a thread per engine (pipeline.detect_embed_overlapped)
    def detect_embed_begin(self, frames, crop: bool = False, faces: torch.Tensor | None = None, valid: torch.Tensor | None = None):
        """Queue detect_embed (or, with ``crop=True``, detect_crop) on the current stream and return at once; the outputs are
        valid after :meth:`detect_embed_end`.  An engine holds one call in flight.  ``faces`` / ``valid`` (optional, crop mode):
        caller-owned contiguous destination buffers -- a slot of a ring whose neighbours hold other batches' crops, so several
        batches can be embedded in one call without a copy (pipeline.detect_embed_overlapped)."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        out = self._call_outputs(n, crop, faces, valid)
        if crop:
            _lib.check(self.lib.trl_detect_crop_begin(self._h, _ptr(fr), n, H, W, _ptr(out["box"]), _ptr(out["prob"]), _ptr(out["rect"]),
                                                      _ptr(out["valid"]), _ptr(out["faces"]), self._stream()))
        else:
            _lib.check(self.lib.trl_detect_embed_begin(self._h, _ptr(fr), n, H, W, _ptr(out["box"]), _ptr(out["prob"]), _ptr(out["rect"]),
                                                       _ptr(out["valid"]), _ptr(out["emb"]), self._stream()))
        self._pending = (out, fr)            # the frame tensor must outlive the queued kernels
        return out

    def detect_embed_end(self):
        """Finish the call queued by :meth:`detect_embed_begin`: the one host synchronisation, the capacity check and (rarely) the re-run."""
        if self._pending is None:
            raise RuntimeError("detect_embed_end() without a call queued by detect_embed_begin()")
        out, _fr = self._pending
        try:
            _lib.check(self.lib.trl_detect_embed_end(self._h))
        finally:
            self._pending = None
        return out

    # the two halves of detect_embed: callers that embed the faces of several batches in ONE embedder call (pipeline.py)
    def detect_crop(self, frames):
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        out = self._call_outputs(n, crop=True)
        _lib.check(self.lib.trl_detect_crop(self._h, _ptr(fr), n, H, W, _ptr(out["box"]), _ptr(out["prob"]), _ptr(out["rect"]),
                                            _ptr(out["valid"]), _ptr(out["faces"]), self._stream()))
        return out

    def embed_faces(self, faces: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
        """Embeddings of prepared crops (detect_crop's ``faces``), zero rows where ``valid`` is 0."""
        faces = faces.to(self.device, torch.float32).contiguous()
        valid = valid.to(self.device, torch.uint8).contiguous()
        n, h, w, _ = faces.shape
        emb = torch.empty((n, 512), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_facenet_embed_masked(self._h, _ptr(faces), _ptr(valid), n, h, w, _ptr(emb), self._stream()))
        return emb

    # NV12 decoder output -> sampled BGR batch on the device (model.py:43,46)
    def ingest_nv12(self, nv12, H: int, W: int, step: int, planar: bool = False) -> torch.Tensor:
        """``planar``: the frames are I420 (Y, U, V planes) instead of NV12 (Y plane, interleaved UV)."""
        if isinstance(nv12, np.ndarray):
            nv12 = torch.from_numpy(np.ascontiguousarray(nv12))
        nv12 = nv12.to(self.device).contiguous()
        if nv12.dtype != torch.uint8 or nv12.dim() != 2 or nv12.shape[1] != H * W * 3 // 2:
            raise ValueError("nv12 must be uint8 (n, H*W*3/2)")
        n_in = int(nv12.shape[0])
        n_out = (n_in + step - 1) // step
        out = torch.empty((n_out, H, W, 3), dtype=torch.uint8, device=self.device)
        k = C.c_int()
        fn = self.lib.trl_ingest_i420 if planar else self.lib.trl_ingest_nv12
        _lib.check(fn(self._h, _ptr(nv12), n_in, H, W, int(step), _ptr(out), C.byref(k), self._stream()))
        assert k.value == n_out
        return out

    # server/model.py:60-66,86-95
    def drift_score(self, emb: torch.Tensor, valid: torch.Tensor, frame_count: int, fps: int):
        emb = emb.to(self.device, torch.float32).contiguous()
        valid = valid.to(self.device, torch.uint8).contiguous()
        n = int(valid.shape[0])
        sims = torch.empty((n,), dtype=torch.float32, device=self.device)
        flags = torch.empty((n,), dtype=torch.uint8, device=self.device)
        res = torch.zeros((4,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.trl_drift_score(self._h, _ptr(emb), _ptr(valid), n, int(frame_count), int(fps), _ptr(sims), _ptr(flags),
                                            _ptr(res), self._stream()))
        r = res.cpu().tolist()
        return {"score": r[0], "run": r[1], "hits": r[2], "total": r[3], "sims": sims, "flags": flags}

    DRIFT_STATE_BYTES = 2064

    def drift_state(self) -> torch.Tensor:
        """A fresh carry for :meth:`drift_update` (one per clip)."""
        return torch.zeros((self.DRIFT_STATE_BYTES,), dtype=torch.uint8, device=self.device)

    def drift_update(self, state: torch.Tensor, emb: torch.Tensor | None, valid: torch.Tensor | None, frame_count: int, fps: int,
                     want_flags: bool = True, sync: bool = True):
        """model.py:60-66 for the NEXT window of a clip (``trl_drift_update``): ``state`` carries previous embedding / run / hits.
        ``emb`` = None (or empty): only the score for ``frame_count`` is recomputed.  ``sync=False`` returns device tensors only
        (``result`` = [score, run, hits, total]) and does not wait."""
        n = 0 if emb is None else int(emb.shape[0])
        d = self.device
        if n:
            emb = emb.to(d, torch.float32).contiguous(); valid = valid.to(d, torch.uint8).contiguous()
        sims = torch.empty((n,), dtype=torch.float32, device=d)
        flags = torch.empty((n,), dtype=torch.uint8, device=d) if want_flags else None
        res = torch.empty((4,), dtype=torch.int32, device=d)
        _lib.check(self.lib.trl_drift_update(self._h, _ptr(state), _ptr(emb) if n else C.c_void_p(0), _ptr(valid) if n else C.c_void_p(0), n,
                                             int(frame_count), int(fps), _ptr(sims), _ptr(flags), _ptr(res), self._stream()))
        out = {"sims": sims, "flags": flags, "result": res}
        if sync:
            r = res.cpu().tolist()
            out.update(score=r[0], run=r[1], hits=r[2], total=r[3])
        return out

    # ---- inspection hooks (parity tests) ----
    def stage_boxes(self, stage: int, frame: int, max_rows: int | None = None) -> np.ndarray:
        k = C.c_int()
        if max_rows is None:                              # every row the stage produced
            _lib.check(self.lib.trl_debug_stage_boxes(self._h, stage, frame, None, 0, C.byref(k)))
            max_rows = max(1, k.value)
        buf = np.zeros((max_rows, 5), np.float32)
        _lib.check(self.lib.trl_debug_stage_boxes(self._h, stage, frame, buf.ctypes.data_as(C.c_void_p), max_rows, C.byref(k)))
        return buf[:min(k.value, max_rows)].copy()

    def pyramid_level(self, frame, level: int) -> torch.Tensor:
        """Test hook: pyramid level of one frame as the fused PNet kernel reads it, (h, w, 3) float32."""
        fr = self._frames(frame[None] if getattr(frame, "ndim", 4) == 3 else frame)
        _, H, W, _ = fr.shape
        m = 12.0 / self.cfg.min_face_size
        out = torch.empty((int(H * m + 1) * int(W * m + 1) * 3,), dtype=torch.float32, device=self.device)
        h, w = C.c_int(), C.c_int()
        _lib.check(self.lib.trl_debug_pyramid_level(self._h, _ptr(fr), H, W, int(level), _ptr(out), C.byref(h), C.byref(w), self._stream()))
        return out[:h.value * w.value * 3].view(h.value, w.value, 3)

    def pyramid_batch(self, frames):
        """Test hook: the pyramid of an n-frame batch through the production pyramid pass, as the raw workspace
        (n, pyr_stride, 3) float32 -- frame f, level l at [f, pix0:pix0 + h*w], the level's padding up to pix0 + pix_pad -- and the
        per-level layout, a list of dicts {pix0, h, w, pix_pad}."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        stride, L = C.c_longlong(), C.c_int()
        lv = np.zeros((16, 4), np.int32)
        _lib.check(self.lib.trl_debug_pyramid_batch(self._h, _ptr(fr), n, H, W, None, C.byref(stride), lv.ctypes.data_as(C.c_void_p), 16,
                                                    C.byref(L), self._stream()))
        out = torch.empty((n, stride.value, 3), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_pyramid_batch(self._h, _ptr(fr), n, H, W, _ptr(out), C.byref(stride), lv.ctypes.data_as(C.c_void_p), 16,
                                                    C.byref(L), self._stream()))
        levels = [dict(zip(("pix0", "h", "w", "pix_pad"), (int(v) for v in lv[l]))) for l in range(L.value)]
        return out, levels

    PYR_KERNELS = {1: "F", 2: "S4", 3: "S8", 4: "SW4", 5: "SW8", 6: "L0-3", 7: "L0-4", 8: "L0-5", 9: "L1", 10: "L2"}   # TRL_PYR_*

    def pyramid_plan(self):
        """Test hook: what the last pyramid pass of this context chose per level, a list of dicts {kernel ("F", "S4", "S8", "SW4",
        "SW8", "L0-3", "L0-4", "L0-5", "L1", "L2"), row_bands, col_bands, cols_per_band, frames_per_launch, khmax}; [] after a
        refused call."""
        rows = np.zeros((16, 6), np.int32)
        L = C.c_int()
        _lib.check(self.lib.trl_debug_pyramid_plan(self._h, rows.ctypes.data_as(C.c_void_p), 16, C.byref(L)))
        keys = ("row_bands", "col_bands", "cols_per_band", "frames_per_launch", "khmax")
        return [dict(kernel=self.PYR_KERNELS[int(r[0])], **dict(zip(keys, (int(v) for v in r[1:])))) for r in rows[:L.value]]

    FN_FAMILIES = {1: "fn_conv", 2: "fn_conv_split4", 3: "conv_tap", 4: "conv_igemm_vec", 5: "conv_igemm_scalar",
                   6: "conv_splitk4", 7: "conv_splitk4_tap", 8: "conv_tap48", 9: "conv_bf16"}   # TRL_FNK_*
    FN_PLAN_DTYPE = np.dtype([(k, np.int32) for k in ("conv", "family", "bm", "bn", "bk", "pad", "nz", "m", "cout", "k", "precision",
                                                      "has_res")] + [("layer", "S48")])

    def facenet_plan(self):
        """Test hook: one dict per conv launch of this context's last embedder call, in walk order: conv (index), layer, family
        ("fn_conv", "fn_conv_split4", "conv_tap", "conv_igemm_vec", "conv_igemm_scalar", "conv_splitk4", "conv_splitk4_tap",
        "conv_tap48", "conv_bf16"), bm, bn, bk, pad, nz (convs sharing the launch), m, cout, k, precision (0 f32 / 1 bf16 / 2 fp16),
        has_res."""
        return self._plan_rows(self.lib.trl_debug_facenet_plan)

    def mtcnn_plan(self):
        """Test hook: one dict per R-/O-Net tail conv launch of this context's last stage_net() call, chunk after chunk, with the
        keys of facenet_plan (layer = "rnet.conv2", ..., "onet.heads"; conv = row index)."""
        return self._plan_rows(self.lib.trl_debug_mtcnn_plan)

    def _plan_rows(self, fn):
        n = C.c_int()
        _lib.check(fn(self._h, None, 0, C.byref(n)))
        rows = np.zeros(n.value, self.FN_PLAN_DTYPE)
        _lib.check(fn(self._h, rows.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        out = []
        for r in rows:
            d = {k: int(r[k]) for k in self.FN_PLAN_DTYPE.names if k != "layer"}
            d["family"] = self.FN_FAMILIES[d["family"]]
            d["layer"] = r["layer"].decode()
            out.append(d)
        return out

    def facenet_capture(self, conv_index: int):
        """Test hook: the next embedder call on this context copies conv ``conv_index``'s input, residual and output views
        (walk order of facenet_plan; -1 disarms); read them with facenet_captured()."""
        _lib.check(self.lib.trl_debug_facenet_capture(self._h, int(conv_index)))

    def facenet_captured(self):
        """(input, residual or None, output) of the last armed capture: dense NHWC numpy arrays, float32, or uint16 holding the
        bf16 / fp16 bits in reduced-precision mode."""
        out = []
        for v in range(3):
            dims = np.zeros(5, np.int32)
            _lib.check(self.lib.trl_debug_facenet_capture_read(self._h, v, None, 0, dims.ctypes.data_as(C.c_void_p)))
            if dims[3] == 0:
                out.append(None)
                continue
            a = np.empty(tuple(int(d) for d in dims[:4]), np.float32 if dims[4] == 4 else np.uint16)
            _lib.check(self.lib.trl_debug_facenet_capture_read(self._h, v, a.ctypes.data_as(C.c_void_p), a.nbytes,
                                                               dims.ctypes.data_as(C.c_void_p)))
            out.append(a)
        return tuple(out)

    def batch_capacity(self, t2_per_frame: float = 0.0, t3_per_frame: float = 0.0) -> int:
        """Test hook: set the optimistic R-/O-Net candidate capacities (per frame) and return the attempts the last call took."""
        k = C.c_int()
        _lib.check(self.lib.trl_debug_batch_capacity(self._h, float(t2_per_frame), float(t3_per_frame), C.byref(k)))
        return k.value

    def option(self, key: str, value: int):
        """Test hook (``trl_debug_option``): "rnet_chunk" / "onet_chunk" / "pnet_screen" / "pnet_defer" / "pnet_defer_cap" / "pyr_row_bands" /
        "tail_pool" (this context), "no_fnconv" (process-wide)."""
        _lib.check(self.lib.trl_debug_option(self._h, key.encode(), int(value)))

    def nms_tiers(self, small: int = 0, full: int = 0):
        """Test hook: LDS tiers (candidates per list) of the sort + NMS kernels; lists longer than ``full`` take the
        global-memory spill tier.  Results never depend on the tiers."""
        _lib.check(self.lib.trl_debug_nms_tiers(self._h, int(small), int(full)))

    def list_stats(self) -> dict:
        """Candidate-list statistics of the last call (attempts, lists in the spill tier, capacities, largest counts)."""
        t = (C.c_longlong * 8)()
        _lib.check(self.lib.trl_debug_list_stats(self._h, t))
        keys = ("attempts", "spill_lists", "spill_used", "spill_cap", "cap_frame", "slots_per_frame", "max_level_count", "max_frame_total")
        return dict(zip(keys, (int(v) for v in t)))

    def pnet_screen_bound(self):
        """Test hook: (A, B, on) of the fused PNet's fp16 conv3 screen, |d_screen - d_exact| <= A X + B."""
        A, B, on = C.c_float(), C.c_float(), C.c_int()
        _lib.check(self.lib.trl_debug_pnet_screen_bound(self._h, C.byref(A), C.byref(B), C.byref(on)))
        return float(A.value), float(B.value), bool(on.value)

    def pnet_screen_weights(self):
        """Test hook: the sixteen per-channel error weights g of the screen's bound, E = sum of g[channel] |x| over a cell's
        3 x 3 x 16 conv2 inputs + B."""
        g = (C.c_float * 16)()
        _lib.check(self.lib.trl_debug_pnet_screen_weights(self._h, g))
        return [float(v) for v in g]

    def pnet_defer(self) -> dict:
        """Test hook: the fused PNet's confirm queue in the last attempt of the last call -- ``slots`` (0: the exact conv3 chain ran
        inline), ``queued`` M-tiles that asked for a slot, ``mtiles`` of the launch, ``hold`` calls the inline path is kept for."""
        t = (C.c_longlong * 4)()
        _lib.check(self.lib.trl_debug_pnet_defer(self._h, t))
        return dict(zip(("slots", "queued", "mtiles", "hold"), (int(v) for v in t)))

    def pnet_run(self, run: int = 0):
        """Test / tuning hook: tiles per cursor fetch of the fused PNet launch (0 = automatic); > 1 exercises the halo carry."""
        _lib.check(self.lib.trl_debug_pnet_run(self._h, int(run)))

    def stage_totals(self):
        """(boxes that entered R-Net, boxes that entered O-Net) over the whole batch of the last call."""
        t = (C.c_int32 * 2)()
        _lib.check(self.lib.trl_debug_stage_totals(self._h, t))
        return int(t[0]), int(t[1])

    def workspace(self, what: int = 0, n: int = 0, h: int = 0, w: int = 0) -> dict:
        """Test hook (``trl_debug_workspace``): the two workspaces of the context in bytes -- ``scratch_cap``, ``scratch_high`` (the
        high-water offset of the last call that used the scratch), ``arena_cap``, ``arena_off``, ``arena_need`` -- and ``need``, the
        dry-run count of a call that is not run: what=1 facenet_embed on n faces of h x w, what=24 / 48 rnet() / onet() on n crops."""
        o = (C.c_longlong * 6)()
        _lib.check(self.lib.trl_debug_workspace(self._h, int(what), int(n), int(h), int(w), o))
        return dict(zip(("scratch_cap", "scratch_high", "arena_cap", "arena_off", "arena_need", "need"), (int(v) for v in o)))

    def poison_workspaces(self, byte: int = 0xFF):
        """Test hook: fill the activation workspaces with a byte pattern (0xFF = NaNs)."""
        _lib.check(self.lib.trl_debug_poison(self._h, int(byte)))

    def redzone(self, guard: int, byte: int = 0xA5):
        """Test hook (``trl_debug_redzone``): follow every block of the context's two workspaces with ``guard`` bytes of red zone
        (a multiple of 256; 0 = off) filled with ``byte``, and sweep them at every rewind and at the end of every call."""
        _lib.check(self.lib.trl_debug_redzone(self._h, int(guard), int(byte)))

    def redzone_report(self, clear: bool = False, sweep: bool = False) -> dict:
        """``sweeps`` made, guard ``bytes`` checked and ``hits`` (dicts: arena, site, block, block_bytes, gap_off, gap_bytes, first,
        last, count; ``nhits`` counts those past the first 256 too) since ``redzone()`` or the last ``clear``.  ``sweep``: sweep
        both workspaces first (site "report")."""
        o = (C.c_longlong * 4)()
        hits = (_lib.TrlRzHit * 256)()
        _lib.check(self.lib.trl_debug_redzone_report(self._h, (1 if clear else 0) | (2 if sweep else 0), o, hits, 256))
        rows = [dict(arena=int(h.arena), site=h.site.decode(), block=int(h.block), block_bytes=int(h.block_bytes), gap_off=int(h.gap_off),
                     gap_bytes=int(h.gap_bytes), first=int(h.first), last=int(h.last), count=int(h.count)) for h in hits[:int(o[3])]]
        return dict(sweeps=int(o[0]), bytes=int(o[1]), nhits=int(o[2]), hits=rows)

    def redzone_poke(self, arena: int, block: int, offset: int, value: int = 0x3C):
        """Self-test of the sweep: one byte ``value`` at ``offset`` of the gap behind block ``block`` (-1: the tail) of workspace
        ``arena`` (0 = cascade lists, 1 = scratch).  The next sweep reports exactly that byte."""
        _lib.check(self.lib.trl_debug_redzone_poke(self._h, int(arena), int(block), int(offset), int(value)))

    def level_counts(self, frame: int):
        a = np.zeros(32, np.int32); b = np.zeros(32, np.int32)
        L = C.c_int()
        _lib.check(self.lib.trl_debug_level_counts(self._h, frame, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(L)))
        return a[:L.value].tolist(), b[:L.value].tolist()

    CAND_DTYPE = np.dtype([("box", np.float32, 4), ("score", np.float32), ("reg", np.float32, 4), ("cell", np.int32)])

    def level_keep(self, frame: int, level: int):
        """Test hook: (records in APPEND order, pick list) of one (frame, level) of the last call: the pick list holds indices into
        the records, in pick order (descending score) -- the per-level batched_nms(0.5) of detect_face()."""
        k = C.c_int()
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), None, 0, C.byref(k)))
        rec = np.zeros((max(1, k.value),), self.CAND_DTYPE)
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(k)))
        rec = rec[:k.value]
        _lib.check(self.lib.trl_debug_level_keep(self._h, int(frame), int(level), None, 0, C.byref(k)))
        idx = np.zeros((max(1, k.value),), np.int32)
        _lib.check(self.lib.trl_debug_level_keep(self._h, int(frame), int(level), idx.ctypes.data_as(C.c_void_p), len(idx), C.byref(k)))
        return rec, idx[:k.value]

    def level_cands(self, frame: int, level: int) -> np.ndarray:
        """Test hook: the candidate records the PNet kernel appended for (frame, level) in the last call, sorted by cell."""
        k = C.c_int()
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), None, 0, C.byref(k)))
        buf = np.zeros((max(1, k.value),), self.CAND_DTYPE)
        _lib.check(self.lib.trl_debug_level_cands(self._h, int(frame), int(level), buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(k)))
        rows = buf[:min(k.value, len(buf))]
        return rows[np.argsort(rows["cell"], kind="stable")].copy()

    def pnet_level(self, frame, level: int):
        fr = self._frames(frame[None] if frame.ndim == 3 else frame)
        _, H, W, _ = fr.shape
        prob = torch.empty((H * W,), dtype=torch.float32, device=self.device)
        reg = torch.empty((H * W * 4,), dtype=torch.float32, device=self.device)
        oh, ow = C.c_int(), C.c_int()
        _lib.check(self.lib.trl_debug_pnet_level(self._h, _ptr(fr), H, W, level, _ptr(prob), _ptr(reg), C.byref(oh), C.byref(ow), self._stream()))
        k = oh.value * ow.value
        return prob[:k].reshape(oh.value, ow.value), reg[:4 * k].reshape(oh.value, ow.value, 4)

    def rnet(self, crops: torch.Tensor) -> torch.Tensor:
        crops = crops.to(self.device, torch.float32).contiguous()
        out = torch.empty((crops.shape[0], 6), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_rnet(self._h, _ptr(crops), crops.shape[0], _ptr(out), self._stream()))
        return out

    def onet(self, crops: torch.Tensor) -> torch.Tensor:
        crops = crops.to(self.device, torch.float32).contiguous()
        out = torch.empty((crops.shape[0], 16), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_onet(self._h, _ptr(crops), crops.shape[0], _ptr(out), self._stream()))
        return out

    def front_net(self, frame, boxes: np.ndarray, net: int) -> torch.Tensor:
        """Test hook: R-Net (net=24 -> [nb, 6]) or O-Net (net=48 -> [nb, 16]) through the production front kernel + tail on the
        given boxes (x1, y1, x2, y2) of one frame."""
        fr = self._frames(frame[None] if getattr(frame, "ndim", 4) == 3 else frame)
        _, H, W, _ = fr.shape
        b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
        out = torch.empty((len(b), 6 if net == 24 else 16), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_front_net(self._h, _ptr(fr), H, W, b.ctypes.data_as(C.c_void_p), len(b), int(net), _ptr(out), self._stream()))
        return out

    def stage_net(self, frames, recs: np.ndarray, net: int, capacity: int, fill: float | None = None) -> torch.Tensor:
        """Test hook: the production stage-2 / stage-3 loop (chunked front kernel + tail, trl_stage_net) over ``capacity``
        candidate slots, ``len(recs)`` of them live: recs rows (frame, x1, y1, x2, y2).  Returns [capacity, 6] (net=24) or
        [capacity, 16] (net=48); rows past len(recs) are not defined (``fill``, if given, is what the output held before)."""
        fr = self._frames(frames)
        nf, H, W, _ = fr.shape
        r = np.ascontiguousarray(recs, np.float32).reshape(-1, 5)
        shape = (int(capacity), 6 if net == 24 else 16)
        out = torch.empty(shape, dtype=torch.float32, device=self.device) if fill is None else \
            torch.full(shape, fill, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_debug_stage_net(self._h, _ptr(fr), nf, H, W, r.ctypes.data_as(C.c_void_p), len(r), int(net),
                                                int(capacity), _ptr(out), self._stream()))
        return out

    def front_pool(self, frames, win: np.ndarray, net: int, capacity: int | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
        """Test hook (``trl_debug_front``): the front kernel's own output.  ``win`` rows are int32 (frame, y0, x0, ih, iw), the
        crop window itself; the launch covers ``capacity`` slots (default len(win)).  Returns the pooled maps [capacity, 11, 11, 28]
        (net=24) or [capacity, 23, 23, 32] (net=48); maps past len(win) keep what ``out`` held.  A device tensor is passed on as it
        is; its address must be a multiple of 4, as for every call that takes frames."""
        fr = self._frames(frames)
        nf, H, W, _ = fr.shape
        w = np.ascontiguousarray(win, np.int32).reshape(-1, 5)
        cap = len(w) if capacity is None else int(capacity)
        shape = (cap, 11, 11, 28) if net == 24 else (cap, 23, 23, 32)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 {shape} tensor on {self.device}")
        _lib.check(self.lib.trl_debug_front(self._h, _ptr(fr), nf, H, W, w.ctypes.data_as(C.c_void_p), len(w), int(net), cap, _ptr(out),
                                            self._stream()))
        return out

    def lists(self, kind: int, H: int, W: int, caps, counts, rows: np.ndarray, logits: np.ndarray | None = None) -> dict:
        """Test hook (``trl_debug_lists``): the cascade's list kernels on caller-built lists of frames H x W, launched as the
        cascade launches them.  ``caps`` = level capacities then the per-frame capacity.
        kind 1: ``rows`` = CAND_DTYPE records of every (frame, level) in append order, ``counts`` [n][L] -> {"keep": [n][L] pick
        lists (indices into that list's records), "rows1": [n] stage-1 rows}.
        kind 2: ``rows`` = stage-1 rows [total][5] (frame-major), ``counts`` [n], ``logits`` [total][6] -> {"rows2": [n]}.
        kind 3: stage-2 rows, ``logits`` [total][16] -> {"rows3", "pts3": [n] per frame, and the k_select outputs "boxes",
        "probs", "points", "counts", "box0", "prob0", "rect", "valid" as numpy arrays}."""
        caps = np.ascontiguousarray(caps, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        n = counts.shape[0]
        L = counts.shape[1] if kind == 1 else 0
        assert len(caps) == L + 1
        rows = np.ascontiguousarray(rows, self.CAND_DTYPE if kind == 1 else np.float32)
        lg = None if logits is None else np.ascontiguousarray(logits, np.float32)
        capF = int(caps[-1])
        out = {}
        if kind == 3:
            mf = self.cfg.max_faces
            dev = dict(boxes=torch.empty((n, mf, 4), dtype=torch.float32, device=self.device),
                       probs=torch.empty((n, mf), dtype=torch.float32, device=self.device),
                       points=torch.empty((n, mf, 10), dtype=torch.float32, device=self.device),
                       counts=torch.empty((n,), dtype=torch.int32, device=self.device),
                       box0=torch.empty((n, 4), dtype=torch.float32, device=self.device),
                       prob0=torch.empty((n,), dtype=torch.float32, device=self.device),
                       rect=torch.empty((n, 4), dtype=torch.int32, device=self.device),
                       valid=torch.empty((n,), dtype=torch.uint8, device=self.device))
            pts = np.zeros((n, capF, 10), np.float32)
        else:
            dev = dict.fromkeys(("boxes", "probs", "points", "counts", "box0", "prob0", "rect", "valid"))
            pts = None
        _lib.check(self.lib.trl_debug_lists(self._h, int(kind), n, int(H), int(W), caps.ctypes.data_as(C.c_void_p), L,
                                            counts.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                            None if lg is None else lg.ctypes.data_as(C.c_void_p),
                                            None if pts is None else pts.ctypes.data_as(C.c_void_p),
                                            *(_ptr(dev[k]) for k in ("boxes", "probs", "points", "counts", "box0", "prob0", "rect", "valid")),
                                            self._stream()))
        torch.cuda.synchronize(self.device)
        if kind == 1:
            out["keep"] = [[self.level_keep(f, l)[1] for l in range(L)] for f in range(n)]
        out[f"rows{kind}"] = [self.stage_boxes(kind, f) for f in range(n)]
        if kind == 3:
            out["pts3"] = [pts[f, :len(out["rows3"][f])].copy() for f in range(n)]
            out.update({k: v.cpu().numpy() for k, v in dev.items()})
        return out

    def _faces_out(self, out: torch.Tensor | None, n: int, S: int) -> torch.Tensor:
        """The destination of a crop hook: a new tensor, or the caller's (e.g. pre-filled, to see what the kernel wrote)."""
        if out is None:
            return torch.empty((n, S, S, 3), dtype=torch.float32, device=self.device)
        if out.shape != (n, S, S, 3) or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 ({n}, {S}, {S}, 3) tensor on {self.device}")
        return out

    def crop_resize(self, frames, rect: torch.Tensor, valid: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """The default crop alone (model.py:55-58): each frame's rectangle (rect [n,4] = x0, y0, x1, y1) -> 80 x 80, / 255."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        rect = rect.to(self.device, torch.int32).contiguous(); valid = valid.to(self.device, torch.uint8).contiguous()
        if rect.shape != (n, 4) or valid.shape != (n,):
            raise ValueError("rect must be (n, 4) and valid (n,)")
        out = self._faces_out(out, n, 80)
        _lib.check(self.lib.trl_debug_crop_resize(self._h, _ptr(fr), n, H, W, _ptr(rect), _ptr(valid), _ptr(out), self._stream()))
        return out

    def crop_aligned(self, frames, pts: torch.Tensor, valid: torch.Tensor, S: int = 160, rgb: bool = True,
                     out: torch.Tensor | None = None) -> torch.Tensor:
        """Embedding mode 3's crop alone: five-point similarity alignment of each frame's face (pts [n,10] = x0..x4, y0..y4)."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        pts = pts.to(self.device, torch.float32).contiguous(); valid = valid.to(self.device, torch.uint8).contiguous()
        if pts.shape != (n, 10) or valid.shape != (n,):
            raise ValueError("pts must be (n, 10) and valid (n,)")
        out = self._faces_out(out, n, int(S))
        _lib.check(self.lib.trl_debug_crop_aligned(self._h, _ptr(fr), n, H, W, _ptr(pts), _ptr(valid), int(S), int(bool(rgb)), _ptr(out),
                                                   self._stream()))
        return out

    def crop_area(self, frames, rect: torch.Tensor, valid: torch.Tensor, S: int = 160, rgb: bool = False,
                  out: torch.Tensor | None = None) -> torch.Tensor:
        """Embedding mode 1 / 2's crop alone: each frame's rectangle (rect [n,4] = x0, y0, x1, y1) area-pooled to S x S,
        truncated to bytes, (v - 127.5) / 128, channels reversed when ``rgb``."""
        fr = self._frames(frames)
        n, H, W, _ = fr.shape
        rect = rect.to(self.device, torch.int32).contiguous(); valid = valid.to(self.device, torch.uint8).contiguous()
        if rect.shape != (n, 4) or valid.shape != (n,):
            raise ValueError("rect must be (n, 4) and valid (n,)")
        out = self._faces_out(out, n, int(S))
        _lib.check(self.lib.trl_debug_crop_area(self._h, _ptr(fr), n, H, W, _ptr(rect), _ptr(valid), int(S), int(bool(rgb)), _ptr(out),
                                                self._stream()))
        return out

    def levels(self, H: int, W: int) -> int:
        """Number of pyramid levels MTCNN.detect builds for an (H, W) frame (detect_face.py scale loop)."""
        m = 12.0 / self.cfg.min_face_size
        minl, k = min(H, W) * m, 0
        while minl >= 12:
            k += 1
            minl *= self.cfg.factor
        return k

    def pnet_span(self, reset: bool = False):
        """(milliseconds, launches): execution spans of the fused PNet launches of this context since the last reset, summed on
        the device (first workgroup start to last workgroup end: the duration rocprofv3 reports for the kernel)."""
        ms, k = C.c_double(), C.c_int32()
        _lib.check(self.lib.trl_debug_pnet_span(self._h, 1 if reset else 0, C.byref(ms), C.byref(k)))
        return float(ms.value), int(k.value)

    def timings(self):
        t = (C.c_float * 4)()
        _lib.check(self.lib.trl_debug_timings(self._h, t))
        k = C.c_float()
        _lib.check(self.lib.trl_debug_pnet_kernel_ms(self._h, C.byref(k)))
        return {"pnet_ms": t[0], "call_ms": t[1], "pnet_launches": int(t[2]), "pyramid_ms": t[3], "pnet_kernel_ms": float(k.value)}


_default: Engine | None = None


def default_engine() -> Engine:
    """Process-wide engine on the current device (synthetic weights unless TRUELY_WEIGHTS points at a TRLW blob)."""
    global _default
    if _default is None:
        import os
        path = os.environ.get("TRUELY_WEIGHTS")
        blob = open(path, "rb").read() if path else None
        _default = Engine(blob)
    return _default
