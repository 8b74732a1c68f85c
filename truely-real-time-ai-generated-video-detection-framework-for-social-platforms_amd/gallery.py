"""Embedding match on the GPU: the step after ``InceptionResnetV1`` -- "whose face is this?".

    g = FaceGallery(metric="cosine")
    g.add(resnet(enrolled_faces), names)              # (m, 512) embeddings, m labels
    who, score = g.identify(resnet(faces), threshold=0.6)

The gallery lives in device memory as a k-major ``[512][ld]`` float32 matrix with each row's squared norm beside it
(csrc/trl_gallery.hip).  ``search`` streams it once and keeps each query's k best matches; the (n, m) score matrix is never
written.  ``scores`` / ``pairwise`` write that matrix for small problems (facenet-pytorch's README ends in such a table:
``(e1 - e2).norm()``).  Scores are defined bit for bit: one float32 fma chain over ascending k per dot
product, then

    cosine      dot / (sqrt(n2 q) * sqrt(n2 g))                    larger is better; a zero row gives NaN
    euclidean   sqrt(max(n2 q + n2 g - 2 dot, 0))                  smaller is better

and matches are ordered better score first, equal scores to the lower gallery index, NaN last.  Embeddings never visit the host."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

METRICS = {"cosine": 0, "euclidean": 1}
MAX_K = 16
DIM = 512


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _metric(metric) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, not {metric!r}")
    return METRICS[metric]


def _rows(x, device) -> torch.Tensor:
    """(n, 512) float32, contiguous, on `device` (a host array or tensor is uploaded once)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x, np.float32))                 # (a copy: the caller's array may be read-only)
    x = x.detach().to(device, torch.float32)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or x.shape[1] != DIM:
        raise ValueError(f"expected (n, {DIM}) embeddings, got {tuple(x.shape)}")
    return x.contiguous()


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class FaceGallery:
    """Enrolled embeddings with a label each.  ``add`` appends; rows are never removed or changed."""

    def __init__(self, metric: str = "cosine", device=None, capacity: int = 1024):
        self.metric = metric
        self._metric = _metric(metric)
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("a FaceGallery lives on a GPU")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._m = 0
        self._labels: list = []
        self._alloc(max(int(capacity), 1))

    def _alloc(self, capacity: int):
        ld = (capacity + 31) // 32 * 32
        self._mat = torch.zeros((DIM, ld), dtype=torch.float32, device=self.device)      # (padding columns stay zero)
        self._n2 = torch.zeros((ld,), dtype=torch.float32, device=self.device)

    @property
    def ld(self) -> int:
        return self._mat.shape[1]

    def __len__(self) -> int:
        return self._m

    @property
    def labels(self) -> list:
        return list(self._labels)

    def add(self, embeddings, labels) -> None:
        """Append m embeddings, (m, 512), with their m labels (any objects)."""
        rows = _rows(embeddings, self.device)
        labels = list(labels)
        m = rows.shape[0]
        if len(labels) != m:
            raise ValueError(f"{m} embeddings but {len(labels)} labels")
        if self._m + m > self.ld:                        # grow geometrically; the copy stays on the device
            old_mat, old_n2, old_ld = self._mat, self._n2, self.ld
            self._alloc(max(2 * old_ld, self._m + m))
            self._mat[:, :old_ld].copy_(old_mat)
            self._n2[:old_ld].copy_(old_n2)
        _lib.check(self.lib.trl_gallery_pack(_ptr(rows), m, _ptr(self._mat), self.ld, _ptr(self._n2), self._m, _stream(self.device)))
        self._m += m
        self._labels.extend(labels)

    def rows(self) -> torch.Tensor:
        """The enrolled embeddings, (m, 512), read back out of the stored matrix."""
        return self._mat[:, :self._m].t().contiguous()

    def scores(self, emb) -> torch.Tensor:
        """(n, len(self)) scores of every query against every enrolled row."""
        q = _rows(emb, self.device)
        n, m = q.shape[0], self._m
        out = torch.empty((n, m), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_gallery_scores(_ptr(q), n, _ptr(self._mat), self.ld, _ptr(self._n2), m, self._metric, _ptr(out), m,
                                               _stream(self.device)))
        return out

    def search(self, emb, k: int = 5, valid=None, max_strip_cols: int = 0):
        """(index (n, k) int32, score (n, k) float32), best match first.  Slots past the gallery, and every slot of a row whose
        ``valid`` entry is zero, hold index -1 and score NaN."""
        q = _rows(emb, self.device)
        n, m, k = q.shape[0], self._m, int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be 1..{MAX_K}")
        if valid is not None:
            if isinstance(valid, np.ndarray):
                valid = torch.from_numpy(valid)
            valid = (valid.to(self.device) != 0).to(torch.uint8).contiguous()
            if valid.shape != (n,):
                raise ValueError(f"valid must have shape ({n},)")
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        score = torch.empty((n, k), dtype=torch.float32, device=self.device)
        need = self.lib.trl_gallery_search_workspace(n, m, k, max_strip_cols)
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
        _lib.check(self.lib.trl_gallery_search(_ptr(q), _ptr(valid), n, _ptr(self._mat), self.ld, _ptr(self._n2), m, self._metric, k,
                                               _ptr(score), _ptr(idx), _ptr(ws), need, max_strip_cols, _stream(self.device)))
        return idx, score

    def identify(self, emb, threshold: float | None = None, valid=None):
        """(labels, score): per query the label of its best match and that match's score, (n,) on the device.  The label is None
        when there is no match (an empty gallery, an invalid row, a NaN score) or the match fails ``threshold`` (cosine: score <
        threshold; euclidean: score > threshold)."""
        idx, score = self.search(emb, k=1, valid=valid)
        idx, score = idx[:, 0], score[:, 0]
        ok = (idx >= 0) & ~torch.isnan(score)
        if threshold is not None:
            ok &= (score >= threshold) if self._metric == 0 else (score <= threshold)
        picks = torch.where(ok, idx, torch.full_like(idx, -1)).tolist()          # n integers to the host: the labels live there
        return [self._labels[i] if i >= 0 else None for i in picks], score


def pairwise(a, b=None, metric: str = "euclidean", device=None) -> torch.Tensor:
    """(len(a), len(b)) scores between two sets of embeddings (b = a when omitted): facenet-pytorch's distance table."""
    if device is None:
        device = a.device if isinstance(a, torch.Tensor) and a.device.type == "cuda" else None
    rows_b = a if b is None else b
    g = FaceGallery(metric=metric, device=device, capacity=max(len(rows_b), 1))
    g.add(rows_b, range(len(rows_b)))
    return g.scores(a)
