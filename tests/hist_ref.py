"""Reference of the score histograms (trl_gallery_hist, csrc/trl_gallery_bins.h) and the inputs its tests share.

    score(i, j)   gallery_ref.scores_ref's
    bin           cosine: #{e : edges[e] <= score} = searchsorted(edges, score, "right")
                  euclidean: #{e : edges[e] < score} = searchsorted(edges, score, "left");  a NaN score: slot E + 1
    counted       query row i and gallery row j both valid and, in upper mode, j > i
    class         1 (genuine) when qid[i] == gid[j], else 0 (impostor)
    counts        (2, E + 2) int64: [class][bin]

so that at every edge e   cosine: #{score >= edges[e]} = sum(counts[bins e + 1 .. E])   euclidean: #{score <= edges[e]} =
sum(counts[bins 0 .. e]).  The rates and the threshold rule of gallery.py (roc_from_counts, threshold_at_far) are restated here as
plain loops over Python integers."""
from __future__ import annotations

import functools

import numpy as np

import cluster_ref as CR
import gallery_ref as G

F32 = np.float32


def bins_ref(scores: np.ndarray, metric: int, edges: np.ndarray) -> np.ndarray:
    """The bin of every score; E + 1 for NaN (numpy would sort NaN behind the last edge: they are masked out first)."""
    s, e = np.asarray(scores, F32), np.asarray(edges, F32)
    nan = np.isnan(s)
    b = np.searchsorted(e, np.where(nan, F32(0), s), side="right" if metric == G.COSINE else "left")
    return np.where(nan, len(e) + 1, b)


def hist_ref(scores: np.ndarray, metric: int, edges: np.ndarray, qid, gid, qvalid=None, gvalid=None, upper: bool = False) -> np.ndarray:
    """scores (n, m) -> counts (2, E + 2) int64."""
    s = np.asarray(scores, F32)
    n, m = s.shape
    E = len(edges)
    keep = np.ones((n, m), bool)
    if qvalid is not None:
        keep &= (np.asarray(qvalid) != 0)[:, None]
    if gvalid is not None:
        keep &= (np.asarray(gvalid) != 0)[None, :]
    if upper:
        assert n == m
        keep &= np.arange(m)[None, :] > np.arange(n)[:, None]
    genuine = np.asarray(qid)[:, None] == np.asarray(gid)[None, :]
    b = bins_ref(s, metric, edges)
    out = np.zeros((2, E + 2), np.int64)
    for cls in (0, 1):
        out[cls] = np.bincount(b[keep & (genuine == bool(cls))], minlength=E + 2)
    return out


def roc_ref(genuine, impostor, nan, metric: int):
    """(tar, far), lists of E floats (NaN for a class without pairs): per edge the accepted pairs, summed one bin at a time."""
    out = []
    for counts, lost in ((genuine, nan[1]), (impostor, nan[0])):
        counts = [int(c) for c in counts]
        E = len(counts) - 1
        total = sum(counts) + int(lost)
        rates = []
        for e in range(E):
            acc = 0
            for b in range(E + 1):
                if (b > e) if metric == G.COSINE else (b <= e):
                    acc += counts[b]
            rates.append(acc / total if total else float("nan"))
        out.append(rates)
    return out[0], out[1]


def threshold_ref(edges, tar, far, target: float, metric: int):
    """(edge, tar, far) at the loosest edge with far <= target, or None."""
    best = None
    for e in range(len(edges)):
        if far[e] <= target:                              # (False for NaN)
            if best is None or (metric == G.COSINE and edges[e] < edges[best]) or (metric == G.EUCLIDEAN and edges[e] > edges[best]):
                best = e
    return None if best is None else (float(edges[best]), tar[best], far[best])


# ---- ids -------------------------------------------------------------------------------------------------------------------------
def gallery_ids() -> np.ndarray:
    """row % 7, the duplicate rows forced to one id (their tied scores are genuine)."""
    ids = (np.arange(G.M_TABLE) % 7).astype(np.int32)
    ids[list(G.DUPS)] = ids[G.DUP_OF]
    return ids


def query_ids() -> np.ndarray:
    """row % 7; the query rows that copy the duplicated gallery row take its id."""
    ids = (np.arange(G.N_TABLE) % 7).astype(np.int32)
    ids[[0, 32]] = gallery_ids()[G.DUP_OF]
    return ids


# ---- edge sets -------------------------------------------------------------------------------------------------------------------
RANGE = {G.COSINE: (-1.0, 1.0), G.EUCLIDEAN: (0.0, 40.0)}        # (the table's euclidean scores: ~1.4 between unit rows, ~32 otherwise)
PLAIN_SETS = ("ONE", "TWO", "E63", "E64", "E1023", "INF")


@functools.lru_cache(maxsize=None)
def ties(metric: int) -> np.ndarray:
    """Edges that the table's scores HIT: about 300 distinct finite values of the 257 x 257 reference scores -- the duplicated
    row's (each is met at least ten times: five rows, five columns), the near pairs' rows', 0 and 1 -- each with its float32
    neighbours on either side."""
    s = CR.table_scores(metric)
    vals = [F32(0.0), F32(1.0)]
    vals += list(s[G.DUP_OF])
    for a, b in G.NEAR_PAIRS:
        vals += [s[a, b], s[a, a], s[b, b]] + list(s[a, 64:80]) + list(s[b, 64:80])
    v = np.unique(np.array([x for x in vals if np.isfinite(x)], F32))
    assert 250 <= len(v) <= 340, len(v)
    e = np.unique(np.concatenate([v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))]).astype(F32))[:1023]
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def edge_set(name: str, metric: int) -> np.ndarray:
    lo, hi = RANGE[metric]
    span = hi - lo
    if name == "TIES":
        return ties(metric)
    e = {"ONE": [lo + 0.55 * span], "TWO": [lo + 0.5 * span, lo + 0.8 * span],
         "E63": np.linspace(lo, hi, 63), "E64": np.linspace(lo, hi, 64), "E1023": np.linspace(lo, hi, 1023),
         "INF": [-np.inf, lo, lo + 0.5 * span, lo + 0.52 * span, hi, np.inf]}[name]
    e = np.array(e, F32)
    assert (e[1:] > e[:-1]).all()
    e.setflags(write=False)
    return e


def with_thresholds(metric: int) -> np.ndarray:
    """E64 and cluster_ref.TABLE_THR's values, as float32: an edge set that holds the thresholds the clustering tests use."""
    e = np.unique(np.concatenate([edge_set("E64", metric), np.array(CR.TABLE_THR[metric], F32)]))
    e.setflags(write=False)
    return e
