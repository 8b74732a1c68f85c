"""Reference of the gallery range search (trl_gallery_range_count / trl_gallery_range_fill, include/truely_hip.h) as plain loops over a
score matrix of gallery_ref's.

    match(r, c)  <=>  qvalid[r] != 0  and  gvalid[c] != 0  and  (not skip_self or c != r)
                      and (cosine: score >= thr | euclidean: score <= thr)        float32 comparisons; NaN never matches

The result is the CSR triple: offsets (n + 1,) int64 with offsets[0] = 0, index (total,) int32 -- row r's matching columns in
ascending order at offsets[r] .. -- and score (total,) float32, the matrix's own entries."""
from __future__ import annotations

import numpy as np

import gallery_ref as G
from gallery_ref import same_bits, scores_ref, table_scores  # noqa: F401  (re-exported for the tests)

F32 = np.float32
LOOSE_THR = {G.COSINE: -2.0, G.EUCLIDEAN: 1e30}          # nearly every pair whose score is not NaN matches


def _match(metric: int, score, thr) -> bool:
    return bool(F32(score) >= F32(thr)) if metric == G.COSINE else bool(F32(score) <= F32(thr))


def match_ref(metric: int, score, thr) -> bool:
    """One float32 comparison; False for a NaN score."""
    with np.errstate(invalid="ignore"):
        return _match(metric, score, thr)


def range_ref(scores: np.ndarray, metric: int, thr: float, qvalid=None, gvalid=None, skip_self: bool = False):
    """scores (n, m) float32 -> (offsets (n + 1,) int64, index (total,) int32, score (total,) float32)."""
    s = np.asarray(scores, F32)
    n, m = s.shape
    assert not skip_self or n == m
    offsets = np.zeros(n + 1, np.int64)
    index, score = [], []
    thr = F32(thr)
    with np.errstate(invalid="ignore"):
        for r in range(n):
            if qvalid is None or qvalid[r] != 0:
                row = s[r]
                for c in range(m):
                    if gvalid is not None and gvalid[c] == 0:
                        continue
                    if skip_self and c == r:
                        continue
                    if _match(metric, row[c], thr):
                        index.append(c)
                        score.append(row[c])
            offsets[r + 1] = len(index)
    return offsets, np.array(index, np.int32), np.array(score, F32)


def unpack(offsets: np.ndarray, index: np.ndarray, n: int, m: int) -> np.ndarray:
    """The CSR lists as an (n, m) bool matrix; asserts that every list is strictly ascending and inside 0..m - 1."""
    assert offsets.shape == (n + 1,) and offsets[0] == 0 and offsets[n] == len(index)
    out = np.zeros((n, m), bool)
    for r in range(n):
        row = index[offsets[r]:offsets[r + 1]]
        assert (np.diff(row) > 0).all() and (len(row) == 0 or (row[0] >= 0 and row[-1] < m)), r
        out[r, row] = True
    return out
