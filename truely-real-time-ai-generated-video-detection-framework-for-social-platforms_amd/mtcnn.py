"""Drop-in for ``facenet_pytorch.MTCNN`` as the reference uses it:

    mtcnn = MTCNN()                      # server/model.py:18
    boxes, _ = mtcnn.detect(frame)       # server/model.py:47

``detect`` keeps the library's return convention: for one ``(H, W, 3)`` uint8 frame it returns
``(boxes, probs)`` with ``boxes`` a float32 ``(k, 4)`` array sorted largest-area first
(``select_largest=True``) or ``(None, [None])`` when no face is found (``landmarks=True`` adds the ``(k, 5, 2)``
O-Net landmarks as a third element, ``None`` without a face); for a batch
``(n, H, W, 3)`` it returns object arrays of those.  The P/R/O-Net cascade runs in
libtruely_hip.so (see csrc/trl_cascade.hip, csrc/trl_pnet.hip).  ``select_largest=False`` returns the boxes in detect_face's
order (descending score).

Face extraction, the library's most common call, is built too (csrc/trl_extract.hip, Engine.extract_faces):

    mtcnn = MTCNN(image_size=160, margin=0, keep_all=False)
    face = mtcnn(img)                    # (3, 160, 160) f32, standardised, or None
    emb = resnet(face.unsqueeze(0))

with facenet-pytorch 2.6.0's semantics as the feature issue "Add MTCNN face extraction on the GPU" restates them
(tests/extract_ref.py): select_boxes' four methods, extract_face's margin arithmetic, crop_resize by input kind (tensor:
imresample area; PIL image: Image.BILINEAR; numpy array: cv2.INTER_AREA), channel order kept.  One deviation:
'center_weighted_size' uses the frame's width and height for every input kind (the library reads img.width / img.height,
so it works for PIL input only there)."""
from __future__ import annotations

import numpy as np
import torch

from .engine import SELECTION_METHODS, Engine, default_engine


def _kind(img):
    """crop_resize's input kind: 'torch' (tensor), 'pil' (PIL image), 'cv2' (numpy array); a batch takes its first element's."""
    if isinstance(img, (list, tuple)):
        kinds = {_kind(i) for i in img}
        if len(kinds) != 1:
            raise ValueError("a batch mixes input kinds")
        return kinds.pop()
    if isinstance(img, torch.Tensor):
        return "torch"
    if isinstance(img, np.ndarray):
        return "cv2"
    if hasattr(img, "getbands"):
        return "pil"
    raise TypeError(f"unsupported image type {type(img).__name__}")


def _is_batch(img):
    return isinstance(img, (list, tuple)) or (isinstance(img, (np.ndarray, torch.Tensor)) and len(img.shape) == 4)


def _frames(img):
    """(n, H, W, 3) uint8 array or tensor of an image or a batch, as detect reads it."""
    if isinstance(img, torch.Tensor):
        return img if img.dim() == 4 else img[None]
    if isinstance(img, (list, tuple)):
        if img and isinstance(img[0], torch.Tensor):
            return torch.stack(list(img))
        return np.stack([np.asarray(i) for i in img])
    arr = np.asarray(img)
    return arr if arr.ndim == 4 else arr[None]


class MTCNN:
    def __init__(self, image_size=160, margin=0, min_face_size=20, thresholds=(0.6, 0.7, 0.7), factor=0.709,
                 post_process=True, select_largest=True, selection_method=None, keep_all=False, device=None,
                 engine: Engine | None = None):
        if selection_method is None:
            selection_method = "largest" if select_largest else "probability"
        if selection_method not in SELECTION_METHODS:
            raise ValueError(f"selection_method must be one of {sorted(SELECTION_METHODS)}")
        self.image_size, self.margin, self.post_process, self.keep_all = image_size, margin, post_process, keep_all
        self.select_largest, self.selection_method = select_largest, selection_method
        self.min_face_size, self.thresholds, self.factor = min_face_size, list(thresholds), factor
        defaults = (min_face_size == 20 and tuple(thresholds) == (0.6, 0.7, 0.7) and factor == 0.709)
        if engine is not None:
            self.engine = engine
        elif defaults:
            self.engine = default_engine()
        else:   # non-default cascade parameters need their own context (same weights)
            base = default_engine()
            self.engine = Engine(getattr(base, "_blob", None), device=base.cfg.device, min_face_size=min_face_size,
                                 thresholds=tuple(thresholds), factor=factor)

    def eval(self):
        return self

    def to(self, device):
        return self

    def detect(self, img, landmarks: bool = False):
        if isinstance(img, torch.Tensor):
            arr = img
            single = arr.dim() == 3
            if single:
                arr = arr[None]
        elif isinstance(img, (list, tuple)):
            arr = np.stack([np.asarray(i) for i in img]); single = False
        else:
            arr = np.asarray(img)
            single = arr.ndim == 3
            if single:
                arr = arr[None]
        res = self.engine.mtcnn_detect(arr, landmarks=landmarks, select_largest=self.select_largest)
        boxes, probs, counts = res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy()
        # facenet-pytorch returns points as (k, 5, 2) = (x_j, y_j); the device rows are x0..x4, y0..y4
        points = res[3].cpu().numpy().reshape(len(counts), -1, 2, 5).transpose(0, 1, 3, 2) if landmarks else None
        out_b, out_p, out_l = [], [], []
        for i in range(len(counts)):
            k = int(counts[i])
            if k == 0:
                out_b.append(None); out_p.append([None]); out_l.append(None)
            else:
                out_b.append(boxes[i, :k].copy()); out_p.append(probs[i, :k].copy())
                if landmarks:
                    out_l.append(points[i, :k].copy())
        if single:
            return (out_b[0], out_p[0], out_l[0]) if landmarks else (out_b[0], out_p[0])
        if landmarks:
            return np.array(out_b, dtype=object), np.array(out_p, dtype=object), np.array(out_l, dtype=object)
        return np.array(out_b, dtype=object), np.array(out_p, dtype=object)

    # ---- MTCNN.forward (facenet-pytorch 2.6.0) ---------------------------------------------------------------------------------
    def __call__(self, img, save_path=None, return_prob=False):
        return self.forward(img, save_path=save_path, return_prob=return_prob)

    def forward(self, img, save_path=None, return_prob: bool = False):
        """Faces of an image, ``(3, S, S)`` f32 (``(k, 3, S, S)`` with keep_all) or None; a batch (4-D array / tensor or list)
        gives a list of those.  return_prob adds the probabilities: the selected face's as a scalar (None without a face) for
        one image, detect's array with keep_all.  CPU tensors, as the library returns them."""
        if save_path is not None:
            raise NotImplementedError("save_path is not supported")
        frames = _frames(img)
        res = self.engine.extract_faces(frames, image_size=self.image_size, margin=self.margin, resample=_kind(img),
                                        post_process=self.post_process, keep_all=self.keep_all, select_largest=self.select_largest,
                                        selection_method=self.selection_method)
        status = res["status"].cpu().numpy()
        if (status < 0).any():
            raise ValueError("a face box gives an empty crop (tile cannot extend outside image)")
        faces, prob = res["faces"].cpu(), res["prob"].cpu().numpy()
        n = int(frames.shape[0])
        out_f, out_p = [], []
        if self.keep_all:
            counts = res["counts"].cpu().numpy()
            row = 0
            for i in range(n):
                k = int(counts[i])
                out_f.append(faces[row:row + k] if k else None)
                out_p.append(prob[row:row + k].copy() if k else [None])
                row += k
        else:
            for i in range(n):
                ok = status[i] == 1
                out_f.append(faces[i] if ok else None)
                out_p.append(prob[i] if ok else None)   # select_boxes: selected_probs[0][0]
        if not _is_batch(img):
            return (out_f[0], out_p[0]) if return_prob else out_f[0]
        if return_prob:
            return out_f, (np.array(out_p, dtype=object) if any(p is None for p in out_p) or self.keep_all else np.array(out_p))
        return out_f

    def select_boxes(self, all_boxes, all_probs, all_points, imgs, method: str = "probability", threshold: float = 0.9,
                     center_weight: float = 2.0):
        """facenet-pytorch's select_boxes on detect's output (on the device, trl_select_faces): the kept box, prob and points of
        every image ((1, 4), (1,), (1, 5, 2) arrays, None / [None] without one); one image gives its own, its prob a scalar."""
        batch = _is_batch(imgs)
        if not batch:
            all_boxes, all_probs, all_points = [all_boxes], [all_probs], [all_points]
        fr = _frames(imgs)
        H, W = int(fr.shape[1]), int(fr.shape[2])
        n, mf = len(all_boxes), self.engine.cfg.max_faces
        boxes = np.zeros((n, mf, 4), np.float32)
        probs = np.zeros((n, mf), np.float32)
        counts = np.zeros((n,), np.int32)
        for i, (b, p) in enumerate(zip(all_boxes, all_probs)):
            if b is not None:
                k = min(len(b), mf)
                boxes[i, :k], probs[i, :k], counts[i] = np.asarray(b, np.float32)[:k, :4], np.asarray(p, np.float32)[:k], k
        pick = self.engine.select_faces(torch.from_numpy(boxes), torch.from_numpy(probs), torch.from_numpy(counts), H, W, method,
                                        threshold, center_weight).cpu().numpy()
        sb, sp, sl = [], [], []
        for i in range(n):
            j = int(pick[i])
            if j < 0:
                sb.append(None); sp.append([None]); sl.append(None)
                continue
            sb.append(np.asarray(all_boxes[i])[[j]]); sp.append(np.asarray(all_probs[i])[[j]])
            sl.append(np.asarray(all_points[i])[[j]] if all_points[i] is not None else None)
        if batch:
            return np.array(sb, dtype=object), np.array(sp, dtype=object), np.array(sl, dtype=object)
        return sb[0], sp[0][0], sl[0]

    def extract(self, img, batch_boxes, save_path=None):
        """facenet-pytorch's extract: every box of an image (keep_all) or its first, cropped with the margin and resampled to
        image_size by the input kind; a batch gives a list."""
        if save_path is not None:
            raise NotImplementedError("save_path is not supported")
        batch = _is_batch(img)
        if not batch:
            batch_boxes = [batch_boxes]
        frames = _frames(img)
        rows, boxes = [], []
        for i, b in enumerate(batch_boxes):
            if b is None:
                continue
            b = np.asarray(b, np.float32).reshape(-1, 4)
            b = b if self.keep_all else b[:1]
            rows += [i] * len(b)
            boxes.append(b)
        faces = status = None
        if rows:
            faces, status = self.engine.extract_boxes(frames, torch.tensor(rows, dtype=torch.int32), torch.from_numpy(np.concatenate(boxes)),
                                                      self.image_size, self.margin, _kind(img), self.post_process)
            faces, status = faces.cpu(), status.cpu().numpy()
            if (status < 0).any():
                raise ValueError("a face box gives an empty crop (tile cannot extend outside image)")
        out, r = [], 0
        for b in batch_boxes:
            if b is None:
                out.append(None)
                continue
            k = len(np.asarray(b).reshape(-1, 4)) if self.keep_all else 1
            out.append(faces[r:r + k] if self.keep_all else faces[r])
            r += k
        return out if batch else out[0]
