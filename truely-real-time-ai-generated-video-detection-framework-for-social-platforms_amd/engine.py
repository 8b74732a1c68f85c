"""Persistent device context of the hot path: weights uploaded once, workspaces reused.

The reference rebuilds ``MTCNN()`` and ``InceptionResnetV1(pretrained="vggface2")`` on every
``run()`` call (server/model.py:18-19); here an :class:`Engine` is created once per GPU and shared
by :class:`mtcnn.MTCNN`, :class:`inception_resnet_v1.InceptionResnetV1` and :func:`model.run`.
PyTorch is used for device memory and streams only; every kernel is in libtruely_hip.so.
"""
from __future__ import annotations

import ctypes as C
import numpy as np
import torch

from . import _lib
from . import weights as _weights
from ._engine_hooks import EngineHooks, _ptr


# trl_select_faces methods / trl_extract_faces resamplers (include/truely_hip.h)
SELECTION_METHODS = {"largest": 0, "probability": 1, "largest_over_threshold": 2, "center_weighted_size": 3}
RESAMPLERS = {"torch": 0, "pil": 1, "cv2": 2}


class Engine(EngineHooks):
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

    def levels(self, H: int, W: int) -> int:
        """Number of pyramid levels MTCNN.detect builds for an (H, W) frame (detect_face.py scale loop)."""
        m = 12.0 / self.cfg.min_face_size
        minl, k = min(H, W) * m, 0
        while minl >= 12:
            k += 1
            minl *= self.cfg.factor
        return k


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
