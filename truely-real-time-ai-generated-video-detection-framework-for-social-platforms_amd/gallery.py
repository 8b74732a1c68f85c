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

and matches are ordered better score first, equal scores to the lower gallery index, NaN last.  ``cluster`` /
``cluster_embeddings`` answer the question that needs no enrolled identities -- "which of these faces are the same person?" --
with DBSCAN over the same scores, from a link bitmap instead of the score matrix, and past 65,536 rows from the range search's
neighbour lists (``method``).  ``score_histogram`` / ``roc`` / ``calibrate`` find
the threshold both take: exact counts of same-label and different-label pairs per score bin, again without the score matrix, and
from them the accept rates at every candidate threshold (``roc_from_counts``, ``threshold_at_far``).  ``range_search`` /
``range_count`` apply such a threshold to the whole gallery: every enrolled row that passes it, per query, as CSR lists in ascending
gallery index -- two streamed passes, count then store, and still no score matrix.  A gallery that enrols several rows per person
(a few photos, every good frame of a clip) has ``identities``: the distinct labels in order of first enrolment.
``search_identities`` / ``identify_topk`` give the k best distinct identities per query, each with its best row -- "the five most
likely people", not five rows of one -- in one streamed pass as well.  ``templates`` pools each identity's rows into one exact
template (pool.py) and returns the gallery of those, one row per person; ``representatives`` names each identity's most typical
enrolled row.  Embeddings never visit the host."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._tensors import DIM, cuda_device, grown, ptr, rows, stream, vector

METRICS = {"cosine": 0, "euclidean": 1}
MAX_K = 16
MAX_CLUSTER_ROWS = 65536                 # the link bitmap's limit (n * n / 8 bytes: 512 MB there); cluster(method="auto") takes lists beyond
MAX_CLUSTER_LIST_ROWS = 1 << 24
CLUSTER_METHODS = ("auto", "bitmap", "lists")
MAX_EDGES = 1023
TEMPLATE_CHUNK = 8192                    # gallery columns turned into rows at a time by templates(): 16 MB


def _metric(metric) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, not {metric!r}")
    return METRICS[metric]


class FaceGallery:
    """Enrolled embeddings with a label each.  ``add`` appends; rows are never removed or changed.  ``search`` / ``identify`` give
    the k best matches, ``search_identities`` / ``identify_topk`` the k best distinct labels (``identities``), ``range_search``
    every match within a threshold, ``cluster`` groups, ``calibrate`` the threshold."""

    def __init__(self, metric: str = "cosine", device=None, capacity: int = 1024):
        self.metric = metric
        self._metric = _metric(metric)
        self.lib = _lib.load()
        self.device = cuda_device(device, "a FaceGallery lives on a GPU")
        self._m = 0
        self._labels: list = []
        self._identities: list = []                      # the distinct labels in order of first enrolment
        self._identity_of: dict = {}                     # label -> its position there: the row's group id
        self._unhashable: list = []                      # positions of the identities that cannot be keys of that dict
        self._alloc(max(int(capacity), 1))

    def _alloc(self, capacity: int):
        ld = (capacity + 31) // 32 * 32
        self._mat = torch.zeros((DIM, ld), dtype=torch.float32, device=self.device)      # (padding columns stay zero)
        self._n2 = torch.zeros((ld,), dtype=torch.float32, device=self.device)
        self._gid = torch.full((ld,), -1, dtype=torch.int32, device=self.device)         # each row's group id, beside the matrix

    @property
    def ld(self) -> int:
        return self._mat.shape[1]

    def __len__(self) -> int:
        return self._m

    @property
    def labels(self) -> list:
        return list(self._labels)

    @property
    def identities(self) -> list:
        """The distinct labels (equal by ``==`` / hash) in order of first enrolment.  A row's group id is its label's position here."""
        return list(self._identities)

    def add(self, embeddings, labels) -> None:
        """Append m embeddings, (m, 512), with their m labels (any objects)."""
        emb = rows(embeddings, self.device)
        labels = list(labels)
        m = emb.shape[0]
        if len(labels) != m:
            raise ValueError(f"{m} embeddings but {len(labels)} labels")
        if self._m + m > self.ld:                        # grow geometrically; the copy stays on the device
            ld = (max(2 * self.ld, self._m + m) + 31) // 32 * 32
            self._mat, self._n2, self._gid = grown(self._mat, ld, dim=1), grown(self._n2, ld), grown(self._gid, ld, fill=-1)
        _lib.check(self.lib.trl_gallery_pack(ptr(emb), m, ptr(self._mat), self.ld, ptr(self._n2), self._m, stream(self.device)))
        ids = []
        for l in labels:
            try:
                i = self._identity_of.get(l)
            except TypeError:                            # an unhashable label (add takes any object): found by == alone, slowly
                i = next((j for j in self._unhashable if self._identities[j] == l), None)
            if i is None:
                i = len(self._identities)
                self._identities.append(l)
                try:
                    self._identity_of[l] = i
                except TypeError:
                    self._unhashable.append(i)
            ids.append(i)
        if m:
            self._gid[self._m:self._m + m].copy_(torch.tensor(ids, dtype=torch.int32), non_blocking=False)
        self._m += m
        self._labels.extend(labels)

    def rows(self) -> torch.Tensor:
        """The enrolled embeddings, (m, 512), read back out of the stored matrix."""
        return self._mat[:, :self._m].t().contiguous()

    def scores(self, emb) -> torch.Tensor:
        """(n, len(self)) scores of every query against every enrolled row."""
        q = rows(emb, self.device)
        n, m = q.shape[0], self._m
        out = torch.empty((n, m), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_gallery_scores(ptr(q), n, ptr(self._mat), self.ld, ptr(self._n2), m, self._metric, ptr(out), m,
                                               stream(self.device)))
        return out

    def search(self, emb, k: int = 5, valid=None, max_strip_cols: int = 0):
        """(index (n, k) int32, score (n, k) float32), best match first.  Slots past the gallery, and every slot of a row whose
        ``valid`` entry is zero, hold index -1 and score NaN."""
        q = rows(emb, self.device)
        n, m, k = q.shape[0], self._m, int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be 1..{MAX_K}")
        valid = _valid(valid, n, self.device)
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        score = torch.empty((n, k), dtype=torch.float32, device=self.device)
        need = self.lib.trl_gallery_search_workspace(n, m, k, max_strip_cols)
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
        _lib.check(self.lib.trl_gallery_search(ptr(q), ptr(valid), n, ptr(self._mat), self.ld, ptr(self._n2), m, self._metric, k,
                                               ptr(score), ptr(idx), ptr(ws), need, max_strip_cols, stream(self.device)))
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

    def search_identities(self, emb, k: int = 5, valid=None, gallery_valid=None, max_strip_cols: int = 0):
        """(group (n, k) int32, index (n, k) int32, score (n, k) float32) on the device: per query the k best DISTINCT identities,
        best first, each with its best enrolled row -- ``identities[group]`` is the label, ``index`` that row, ``score`` its score
        (``scores``' bits).  The enrolled rows are taken in ``search``'s order and a row is kept iff no earlier row has its label;
        rows whose ``gallery_valid`` entry is zero are left out.  Slots past the last identity, and every slot of a row whose
        ``valid`` entry is zero, hold -1 / -1 / NaN.  The gallery is streamed once; the call does not synchronise."""
        q = rows(emb, self.device)
        n, m, k = q.shape[0], self._m, int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be 1..{MAX_K}")
        valid, gv = _valid(valid, n, self.device), _valid(gallery_valid, m, self.device)
        gid = self._gid[:m]
        if gv is not None:
            gid = torch.where(gv != 0, gid, torch.full_like(gid, -1))         # (on the device: a masked row is an excluded row)
        group = torch.empty((n, k), dtype=torch.int32, device=self.device)
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        score = torch.empty((n, k), dtype=torch.float32, device=self.device)
        need = self.lib.trl_gallery_search_groups_workspace(n, m, k, max_strip_cols)
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
        _lib.check(self.lib.trl_gallery_search_groups(ptr(q), ptr(valid), n, ptr(self._mat), self.ld, ptr(self._n2), ptr(gid), m,
                                                      self._metric, k, ptr(score), ptr(idx), ptr(group), ptr(ws), need, max_strip_cols,
                                                      stream(self.device)))
        return group, idx, score

    def identify_topk(self, emb, k: int = 5, threshold: float | None = None, valid=None, gallery_valid=None) -> list:
        """Per query a list of ``(label, score)`` pairs, best first: its at most k best distinct identities, each with the score of
        its best enrolled row.  Entries that are empty, whose score is NaN, or that fail ``threshold`` by identify's convention
        (cosine: score < threshold; euclidean: score > threshold) are dropped, so a list may be shorter than k, or empty."""
        group, _idx, score = self.search_identities(emb, k=k, valid=valid, gallery_valid=gallery_valid)
        ok = (group >= 0) & ~torch.isnan(score)
        if threshold is not None:
            ok &= (score >= threshold) if self._metric == 0 else (score <= threshold)
        picks = torch.where(ok, group, torch.full_like(group, -1)).tolist()   # n x k integers and scores to the host: the labels live there
        scores = score.tolist()
        return [[(self._identities[g], s) for g, s in zip(gs, ss) if g >= 0] for gs, ss in zip(picks, scores)]

    def _pooled(self, weights, gallery_valid, unit: bool, representative: bool, max_state_bytes: int) -> dict:
        """The enrolled rows pooled per identity (pool.py).  The k-major matrix is read in column chunks, each turned into rows once,
        with the n2 the gallery keeps: no second copy of the gallery, no second n2 pass."""
        from . import pool
        m, G = self._m, len(self._identities)
        gv = _valid(gallery_valid, m, self.device)
        gid = self._gid[:m]
        if gv is not None:
            gid = torch.where(gv != 0, gid, torch.full_like(gid, -1))         # (search_identities' fold: a masked row is an excluded row)
        w = vector(weights, m, torch.float32, self.device, "weights")

        def blocks():
            for a in range(0, m, TEMPLATE_CHUNK):
                b = min(a + TEMPLATE_CHUNK, m)
                yield a, self._mat[:, a:b].t().contiguous(), self._n2[a:b]

        return pool._pool_blocks(self.device, blocks, m, gid, w, G, unit, representative, max_state_bytes, 0)

    def templates(self, weights=None, gallery_valid=None, unit: bool = True, representative: bool = False,
                  max_state_bytes: int = 256 << 20):
        """``(gallery, info)``: one template per identity.  ``gallery`` is a new ``FaceGallery`` of this metric and device that
        holds, in ``identities`` order and labelled with the identity, the template of every identity with ``count > 0`` -- a
        gallery with 20 rows per person becomes one a twentieth as wide to ``search`` / ``identify``.  ``info`` is
        ``pool_embeddings``' dict over every identity (row g is ``identities[g]``): ``template``, ``count``, ``weight``,
        ``cohesion``, ``skipped`` and, with ``representative=True``, ``representative`` (the enrolled row closest to its
        identity's template, -1 without one) and ``rep_score``.  ``weights`` (len(self),) in (0, 1] weigh the rows; rows whose
        ``gallery_valid`` entry is zero are left out, as in ``search_identities``.  ``count`` is read back to pick the rows: one
        synchronisation."""
        info = self._pooled(weights, gallery_valid, unit, representative, max_state_bytes)
        keep = torch.nonzero(info["count"] > 0)[:, 0]
        picks = keep.tolist()
        g = FaceGallery(metric=self.metric, device=self.device, capacity=max(len(picks), 1))
        g.add(info["template"][keep], [self._identities[i] for i in picks])
        return g, info

    def representatives(self, weights=None, gallery_valid=None, unit: bool = True) -> torch.Tensor:
        """(len(identities),) int32 on the device: per identity its enrolled row closest to the identity's own template
        (``templates(representative=True)``'s ``representative``); -1 for an identity without a contributing row.  No
        synchronisation."""
        return self._pooled(weights, gallery_valid, unit, True, 256 << 20)["representative"]

    def cluster(self, threshold: float, min_samples: int = 1, valid=None, return_info: bool = False, max_strip_cols: int = 0,
                method: str = "auto", max_links: int | None = None):
        """DBSCAN labels of the enrolled rows, (len(self),) int32 on the device: "which of these are the same person?".
        ``pool_embeddings(emb, labels)`` with these labels gives one template per cluster (noise, -1, is ignored there).

        Rows i != j are linked when their score passes ``threshold`` (identify's convention: cosine ``score >= threshold``,
        euclidean ``score <= threshold``, both in float32; a NaN score never links).  A row with at least ``min_samples`` rows in
        its neighbourhood, itself included, is a core row; clusters are the connected components of the links among core rows,
        numbered in ascending order of their smallest core member; a row that is not core takes the smallest number among its
        core neighbours' clusters, and -1 (noise) without one.  Rows whose ``valid`` entry is zero link to nothing and get -1.
        ``min_samples=1`` is plain threshold connected components.  This is ``sklearn.cluster.DBSCAN(metric="precomputed")``
        exactly.  The n x n scores are never written.

        ``method``: where the links are kept.  ``"bitmap"``: n * n / 8 bytes, one pass over the rows; ``ValueError`` past
        65,536 rows (``MAX_CLUSTER_ROWS``).  ``"lists"``: ``range_search(emb=None)``'s neighbour lists, 8 bytes per link and two
        passes over the rows, up to 16,777,216 rows; ``max_links`` is that search's ``max_results``: ``ValueError``, naming the
        total, before anything is allocated for more links than that.  ``"auto"``: the bitmap up to its limit, lists beyond.  Labels,
        core and degree are the same bits either way.

        With ``return_info`` a dict: ``labels``, ``core`` (n,) uint8, ``degree`` (n,) int32 (links + 1; 0 for an invalid row),
        ``n_clusters`` and ``rounds`` (ints), ``method`` (the one taken) and, for lists, ``links`` (the total length of the lists:
        each linked pair counts twice).  The call synchronises the current stream."""
        n = self._m
        if method not in CLUSTER_METHODS:
            raise ValueError(f"method must be one of {CLUSTER_METHODS}, not {method!r}")
        if method == "auto":
            method = "bitmap" if n <= MAX_CLUSTER_ROWS else "lists"
        if method == "bitmap" and n > MAX_CLUSTER_ROWS:
            raise ValueError(f"cluster(method='bitmap') takes at most {MAX_CLUSTER_ROWS} rows, not {n}")
        if method == "lists" and n > MAX_CLUSTER_LIST_ROWS:
            raise ValueError(f"cluster takes at most {MAX_CLUSTER_LIST_ROWS} rows, not {n}")
        threshold, min_samples = float(threshold), int(min_samples)
        valid = _valid(valid, n, self.device)
        degree = torch.empty((n,), dtype=torch.int32, device=self.device)
        labels = torch.empty((n,), dtype=torch.int32, device=self.device)
        core = torch.empty((n,), dtype=torch.uint8, device=self.device)
        count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        rounds = C.c_int(0)
        s = stream(self.device)
        info = {"labels": labels, "core": core, "degree": degree}
        if method == "bitmap":
            words = (n + 31) // 32
            adj = torch.empty((n, words), dtype=torch.int32, device=self.device)
            need = self.lib.trl_cluster_workspace(n)
            ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
            q = self.rows() if n else None
            _lib.check(self.lib.trl_cluster_links(ptr(q), ptr(valid), n, ptr(self._mat), self.ld, ptr(self._n2), self._metric,
                                                  threshold, ptr(adj), words, ptr(degree), max_strip_cols, s))
            _lib.check(self.lib.trl_cluster_labels(ptr(adj), words, ptr(degree), n, min_samples, ptr(labels), ptr(core), ptr(count),
                                                   ptr(ws), need, C.byref(rounds), s))
        else:
            offsets, index, _score = self.range_search(None, threshold, valid=valid, max_results=max_links, max_strip_cols=max_strip_cols)
            del _score                                   # (the fill pass writes the scores; the labels do not read them)
            info["links"] = index.shape[0]
            if not index.shape[0]:
                index = torch.empty((1,), dtype=torch.int32, device=self.device)          # (an empty tensor has no address)
            need = self.lib.trl_cluster_lists_workspace(n)
            ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
            _lib.check(self.lib.trl_cluster_labels_lists(ptr(offsets), ptr(index), ptr(valid), n, min_samples, 0, ptr(degree),
                                                         ptr(labels), ptr(core), ptr(count), ptr(ws), need, C.byref(rounds), s))
        if not return_info:
            return labels
        info.update(n_clusters=int(count.item()), rounds=rounds.value, method=method)
        return info

    def score_histogram(self, emb=None, labels=None, edges=None, valid=None, gallery_valid=None, max_strip_cols: int = 0) -> dict:
        """Exact pair counts per score bin, same-label ("genuine") and different-label ("impostor") pairs apart: what a
        threshold for ``identify`` / ``cluster`` is read from.  The gallery is streamed once; no score matrix is written.

        ``emb`` (n, 512) with its n ``labels`` is compared against every enrolled row.  With ``emb=None`` the gallery is compared
        against itself and each unordered pair (i < j) is counted once.  Labels are equal by ``==`` / hash.  ``edges``: E
        candidate thresholds, 1 <= E <= 1023, strictly ascending, no NaN (default: 1,001 steps over -1..1 for cosine, over 0..2
        for euclidean).  A score's bin is the number of edges <= it (cosine) or < it (euclidean), so the pairs that cosine
        ``score >= edges[e]`` accepts are bins e + 1 .. E, and those that euclidean ``score <= edges[e]`` accepts bins 0 .. e:
        exactly, in float32.  ``valid`` masks the query rows and ``gallery_valid`` the enrolled rows (with ``emb=None`` they are the
        same rows: give either one).

        Returns ``edges`` (E,) float32, ``genuine`` and ``impostor`` (E + 1,) int64, and ``nan`` (2,) int64 -- the pairs whose
        score is NaN, impostor then genuine -- all on the device."""
        m = self._m
        ids: dict = {}
        gid = [ids.setdefault(l, len(ids)) for l in self._labels]
        if emb is None:
            if labels is not None:
                raise ValueError("labels belong to emb; the gallery's rows carry their own")
            if valid is not None and gallery_valid is not None:
                raise ValueError("with emb=None the query rows are the gallery's: give valid or gallery_valid, not both")
            q, n, qid, pairs = (self.rows() if m else None), m, gid, 1
            qv = gv = _valid(valid if gallery_valid is None else gallery_valid, m, self.device)
        else:
            q = rows(emb, self.device)
            n, pairs = q.shape[0], 0
            if labels is None:
                raise ValueError("emb needs its labels")
            labels = list(labels)
            if len(labels) != n:
                raise ValueError(f"{n} embeddings but {len(labels)} labels")
            qid = [ids.setdefault(l, len(ids)) for l in labels]
            qv, gv = _valid(valid, n, self.device), _valid(gallery_valid, m, self.device)
        edges = _edges(edges, self._metric, self.device)
        E = edges.shape[0]
        qid_t = torch.tensor(qid, dtype=torch.int32, device=self.device)
        gid_t = qid_t if emb is None else torch.tensor(gid, dtype=torch.int32, device=self.device)
        counts = torch.empty((2, E + 2), dtype=torch.int64, device=self.device)
        need = self.lib.trl_gallery_hist_workspace(n, m, E, max_strip_cols)
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
        _lib.check(self.lib.trl_gallery_hist(ptr(q), ptr(qv), ptr(qid_t), n, ptr(self._mat), self.ld, ptr(self._n2), ptr(gv),
                                             ptr(gid_t), m, self._metric, pairs, ptr(edges), E, ptr(counts), ptr(ws), need,
                                             max_strip_cols, stream(self.device)))
        return {"edges": edges, "genuine": counts[1, :E + 1], "impostor": counts[0, :E + 1], "nan": counts[:, E + 1]}

    def _range_pass1(self, emb, threshold, valid, gallery_valid, max_strip_cols):
        """Pass 1 of the range search queued on the current stream: (the arguments both passes share, offsets, workspace)."""
        m = self._m
        if threshold is None:
            raise ValueError("a range search needs its threshold")
        if emb is None:
            if valid is not None and gallery_valid is not None:
                raise ValueError("with emb=None the query rows are the gallery's: give valid or gallery_valid, not both")
            q, n, self_pairs = (self.rows() if m else None), m, 1
            qv = gv = _valid(valid if gallery_valid is None else gallery_valid, m, self.device)
        else:
            q = rows(emb, self.device)
            n, self_pairs = q.shape[0], 0
            qv, gv = _valid(valid, n, self.device), _valid(gallery_valid, m, self.device)
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device=self.device)
        need = self.lib.trl_gallery_range_workspace(n, m, max_strip_cols)
        ws = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
        args = (ptr(q), ptr(qv), n, ptr(self._mat), self.ld, ptr(self._n2), ptr(gv), m, self._metric, float(threshold), self_pairs)
        _lib.check(self.lib.trl_gallery_range_count(*args, ptr(offsets), ptr(ws), need, max_strip_cols, stream(self.device)))
        return args, (q, qv, gv), offsets, ws, need

    def range_count(self, emb=None, threshold: float | None = None, valid=None, gallery_valid=None, max_strip_cols: int = 0) -> torch.Tensor:
        """(n,) int64 on the device: how many enrolled rows each query matches (``range_search``'s rule and arguments).  The gallery
        is streamed once; the call does not synchronise."""
        _args, _keep, offsets, _ws, _need = self._range_pass1(emb, threshold, valid, gallery_valid, max_strip_cols)
        return offsets[1:] - offsets[:-1]

    def range_search(self, emb=None, threshold: float | None = None, valid=None, gallery_valid=None, max_results: int | None = None,
                     max_strip_cols: int = 0):
        """Every enrolled row within ``threshold`` of each query, as CSR lists: ``(offsets (n + 1,) int64, index (total,) int32,
        score (total,) float32)`` on the device.  Query r's matches are ``index[offsets[r]:offsets[r + 1]]`` in ascending gallery
        index, with their scores (``scores``' bits) beside them.

        A pair matches by identify's convention -- cosine ``score >= threshold``, euclidean ``score <= threshold``, in float32; a
        NaN score never matches -- when the query's ``valid`` entry and the enrolled row's ``gallery_valid`` entry are non-zero.
        With ``emb=None`` the gallery is searched against itself and a row does not match itself: near-duplicate enrolments,
        exactly the rows of ``cluster``'s link bitmap at the same threshold (``valid`` and ``gallery_valid`` are then the same
        rows: give either one).  Neither the (n, m) scores nor n x m bits are written: the gallery is streamed twice, once to
        count and once to store.

        The total is read back to size the outputs, so the call synchronises the current stream.  ``max_results``: raise
        ``ValueError`` (naming the total, before anything is allocated for it) when there are more matches than that."""
        args, _keep, offsets, ws, need = self._range_pass1(emb, threshold, valid, gallery_valid, max_strip_cols)
        total = int(offsets[-1].item())
        if max_results is not None and total > int(max_results):
            raise ValueError(f"range_search found {total} matches, more than max_results = {int(max_results)}")
        index = torch.empty((total,), dtype=torch.int32, device=self.device)
        score = torch.empty((total,), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trl_gallery_range_fill(*args, ptr(offsets), ptr(ws), need, total, ptr(index), ptr(score), max_strip_cols,
                                                   stream(self.device)))
        return offsets, index, score

    def roc(self, emb=None, labels=None, edges=None, valid=None, gallery_valid=None, max_strip_cols: int = 0) -> dict:
        """``score_histogram`` turned into rates: ``edges`` (E,) float32, ``tar`` and ``far`` (E,) float64, host arrays --
        the share of genuine / impostor pairs that each edge, used as the threshold, accepts (``roc_from_counts``)."""
        h = self.score_histogram(emb, labels, edges, valid, gallery_valid, max_strip_cols)
        tar, far = roc_from_counts(h["genuine"], h["impostor"], h["nan"], self.metric)
        return {"edges": h["edges"].cpu().numpy(), "tar": tar, "far": far}

    def calibrate(self, far: float = 1e-3, emb=None, labels=None, edges=None, valid=None, gallery_valid=None,
                  max_strip_cols: int = 0) -> dict:
        """The loosest of ``edges`` whose false accept rate is at most ``far``: ``{"threshold", "tar", "far"}`` (floats; the rates
        are those measured at the threshold).  ``ValueError`` when no edge qualifies (``threshold_at_far``)."""
        r = self.roc(emb, labels, edges, valid, gallery_valid, max_strip_cols)
        thr, t, f = threshold_at_far(r["edges"], r["tar"], r["far"], far, self.metric)
        return {"threshold": thr, "tar": t, "far": f}


def _valid(valid, n: int, device):
    """None, or the mask as (n,) uint8 on `device`."""
    if valid is None:
        return None
    if isinstance(valid, np.ndarray):
        valid = torch.from_numpy(valid)
    valid = (valid.to(device) != 0).to(torch.uint8).contiguous()
    if valid.shape != (n,):
        raise ValueError(f"valid must have shape ({n},)")
    return valid


def _edges(edges, metric: int, device) -> torch.Tensor:
    """The candidate thresholds as (E,) float32 on `device`, checked: 1..MAX_EDGES of them, strictly ascending, no NaN."""
    if edges is None:
        edges = np.linspace(-1.0, 1.0, 1001) if metric == 0 else np.linspace(0.0, 2.0, 1001)
    if isinstance(edges, torch.Tensor):
        edges = edges.detach().cpu().numpy()
    e = np.array(edges, np.float32).reshape(-1)
    if not 1 <= len(e) <= MAX_EDGES:
        raise ValueError(f"edges must hold 1..{MAX_EDGES} values, not {len(e)}")
    if np.isnan(e).any() or not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be strictly ascending float32 values without NaN")
    return torch.from_numpy(e).to(device)


def _host(x, dtype) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype)


def roc_from_counts(genuine, impostor, nan, metric: str = "cosine"):
    """(tar, far), float64 arrays of length E, from ``score_histogram``'s counts (numpy arrays or tensors): the share of the
    genuine / impostor pairs that threshold ``edges[e]`` accepts -- cosine ``score >= edges[e]`` (bins e + 1 .. E), euclidean
    ``score <= edges[e]`` (bins 0 .. e).  Integer cumulative sums, then one division by the class total; that total includes the
    class's NaN scores (``nan``: impostor, genuine), which no threshold accepts.  A class without pairs gives NaN."""
    cosine = _metric(metric) == 0
    nan = _host(nan, np.int64)
    out = []
    for counts, lost in ((genuine, nan[1]), (impostor, nan[0])):
        c = _host(counts, np.int64)
        accepted = np.cumsum(c[::-1])[::-1][1:] if cosine else np.cumsum(c)[:-1]
        total = int(c.sum()) + int(lost)
        out.append(accepted / np.float64(total) if total else np.full(len(c) - 1, np.nan))
    return out[0], out[1]


def threshold_at_far(edges, tar, far, target: float, metric: str = "cosine"):
    """(threshold, tar, far): the loosest edge whose false accept rate is at most ``target`` -- the smallest such edge for cosine,
    the largest for euclidean -- with the rates at it.  ``ValueError`` when no edge qualifies (a NaN rate never does)."""
    cosine = _metric(metric) == 0
    edges, tar, far = _host(edges, np.float32), _host(tar, np.float64), _host(far, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.nonzero(far <= target)[0]
    if not len(ok):
        raise ValueError(f"no edge has a false accept rate <= {target}")
    e = int(ok.min() if cosine else ok.max())
    return float(edges[e]), float(tar[e]), float(far[e])


def cluster_embeddings(emb, threshold: float, metric: str = "cosine", min_samples: int = 1, valid=None, device=None,
                       return_info: bool = False, method: str = "auto", max_links: int | None = None):
    """``FaceGallery.cluster`` for loose embeddings, (n, 512): the faces of a clip, an enrolment set to de-duplicate.  ``method``
    and ``max_links`` are ``cluster``'s.  ``pool_embeddings(emb, labels)`` with the labels gives one template per cluster."""
    if device is None:
        device = emb.device if isinstance(emb, torch.Tensor) and emb.device.type == "cuda" else None
    g = FaceGallery(metric=metric, device=device, capacity=max(len(emb), 1))
    g.add(emb, range(len(emb)))
    return g.cluster(threshold, min_samples=min_samples, valid=valid, return_info=return_info, method=method, max_links=max_links)


def pairwise(a, b=None, metric: str = "euclidean", device=None) -> torch.Tensor:
    """(len(a), len(b)) scores between two sets of embeddings (b = a when omitted): facenet-pytorch's distance table."""
    if device is None:
        device = a.device if isinstance(a, torch.Tensor) and a.device.type == "cuda" else None
    rows_b = a if b is None else b
    g = FaceGallery(metric=metric, device=device, capacity=max(len(rows_b), 1))
    g.add(rows_b, range(len(rows_b)))
    return g.scores(a)
