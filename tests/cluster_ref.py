"""Reference of the embedding clustering (trl_cluster_links / trl_cluster_labels) and the inputs its tests share.

Input: n embeddings of 512 float32, a metric, a finite float32 threshold thr, min_samples >= 1, an optional valid mask.

    score(i, j)   gallery_ref.scores_ref's, row i as the query and row j as the gallery row; symmetric bit for bit
    link(i, j)    i != j, both rows valid, and  cosine: score >= thr   euclidean: score <= thr   (a NaN score never links)
    degree(i)     1 + the number of links of i for a valid row (a row counts itself whatever its own score is), 0 for an invalid one
    core(i)       degree(i) >= min_samples  (an invalid row never is)
    clusters      the connected components of the link graph restricted to core rows, numbered 0, 1, ... in ascending order of
                  their smallest core member
    border rows   a valid row that is not core and has a core neighbour takes the smallest number among those neighbours' clusters
    every other row (noise, invalid rows) gets -1

which is sklearn.cluster.DBSCAN(metric="precomputed") on D = where(link, 0, 1) with a zero diagonal and eps = 0.5, without its
dependence on visiting order (tests/test_cluster_cpu.py compares the two).  Nothing here uses scipy or scikit-learn.

The bitmap: bit b of word adj[i, w] (uint32) <=> link(i, 32 w + b); bits at columns >= n are zero."""
from __future__ import annotations

import functools

import numpy as np

import gallery_ref as G

F32 = np.float32
MAX_N = 65536


def links_ref(scores: np.ndarray, metric: int, thr: float, valid: np.ndarray | None = None) -> np.ndarray:
    """scores (n, n) float32 -> link (n, n) bool."""
    s = np.asarray(scores, F32)
    n = s.shape[0]
    assert s.shape == (n, n)
    with np.errstate(invalid="ignore"):
        link = (s >= F32(thr)) if metric == G.COSINE else (s <= F32(thr))          # (False for NaN either way)
    link = link & ~np.eye(n, dtype=bool)
    if valid is not None:
        ok = np.asarray(valid) != 0
        link = link & ok[:, None] & ok[None, :]
    return link


def degree_ref(link: np.ndarray, valid: np.ndarray | None = None) -> np.ndarray:
    d = link.sum(axis=1).astype(np.int32) + 1
    if valid is not None:
        d = np.where(np.asarray(valid) != 0, d, 0).astype(np.int32)
    return d


def labels_ref(link: np.ndarray, degree: np.ndarray, min_samples: int):
    """link (n, n) bool, symmetric with an empty diagonal; degree (n,), 0 = invalid row -> (labels int32, core uint8, count)."""
    n = link.shape[0]
    assert min_samples >= 1 and np.array_equal(link, link.T) and not np.diagonal(link).any()
    core = (degree > 0) & (degree >= min_samples)
    labels = np.full(n, -1, np.int32)
    count = 0
    for i in range(n):                                   # ascending: a new component is met at its smallest core member
        if not core[i] or labels[i] >= 0:
            continue
        labels[i] = count
        todo = [i]
        while todo:
            j = todo.pop()
            for t in np.nonzero(link[j] & core & (labels < 0))[0]:
                labels[t] = count
                todo.append(int(t))
        count += 1
    for i in np.nonzero(~core & (degree > 0))[0]:
        nb = link[i] & core
        if nb.any():
            labels[i] = labels[nb].min()
    return labels, core.astype(np.uint8), count


def pack_bitmap(link: np.ndarray, pitch_words: int | None = None) -> np.ndarray:
    """link (n, n) bool -> (n, pitch_words) uint32, words past ceil(n / 32) zero."""
    n = link.shape[0]
    words = (n + 31) // 32
    pitch = words if pitch_words is None else pitch_words
    bits = np.zeros((n, words * 32), np.uint64)
    bits[:, :n] = link
    w = (bits.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    out = np.zeros((n, pitch), np.uint32)
    out[:, :words] = w
    return out


def unpack_bitmap(adj: np.ndarray, n: int) -> np.ndarray:
    words = (n + 31) // 32
    a = np.ascontiguousarray(adj[:n, :words]).astype(np.uint32)
    bits = (a[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(n, words * 32)[:, :n].astype(bool)


# ---- the table: gallery_ref.tables()[0] against itself -----------------------------------------------------------------------------
N_TABLE = G.M_TABLE
INVALID = (31, 32, 40, 41, 200)         # rows on both sides of the 32-row tile edge, and three more
TABLE_THR = {G.COSINE: (0.12, 0.999), G.EUCLIDEAN: (1.3, 31.0)}
MIN_SAMPLES = (1, 2, 3, 4, 6)


@functools.lru_cache(maxsize=None)
def table_scores(metric: int) -> np.ndarray:
    """(257, 257): the gallery table's rows against themselves.  The leading n x n block is the scores of its first n rows."""
    g, _q = G.tables()
    s = G.scores_ref(g, g, metric)
    s.setflags(write=False)
    return s


def mask(n: int, invalid=INVALID) -> np.ndarray:
    v = np.ones(n, np.uint8)
    v[[r for r in invalid if r < n]] = 0
    return v


@functools.lru_cache(maxsize=None)
def table_links(metric: int, thr: float, n: int = N_TABLE, invalid: tuple = ()):
    """(link (n, n), degree (n,)) of the table's first n rows, rows `invalid` masked out; read-only."""
    valid = mask(n, invalid) if invalid else None
    link = links_ref(table_scores(metric)[:n, :n], metric, thr, valid)
    deg = degree_ref(link, valid)
    link.setflags(write=False)
    deg.setflags(write=False)
    return link, deg


# ---- hand-made graphs: (link (n, n) bool, degree (n,) int32), every row valid unless said ------------------------------------------
def graph(n: int, edges) -> tuple:
    link = np.zeros((n, n), bool)
    for a, b in edges:
        assert a != b
        link[a, b] = link[b, a] = True
    return link, degree_ref(link)


def empty_graph(n: int):
    return graph(n, [])


def clique(n: int, members=None):
    members = list(range(n)) if members is None else list(members)
    return graph(n, [(a, b) for i, a in enumerate(members) for b in members[i + 1:]])


def star(n: int, centre: int):
    """With min_samples = n the centre (degree n) is the only core row and every other row is a border row."""
    return graph(n, [(centre, r) for r in range(n) if r != centre])


def two_cliques_and_bridge(size: int = 5):
    """Rows 1 .. size and size + 1 .. 2 size are cliques; row 0 links to one member of each and to nothing else.  With
    min_samples = 4 row 0 (degree 3) is a border row of both clusters: it takes the lower number.  The clique that holds the
    smaller row index is cluster 0 whichever of them row 0 is wired to first."""
    n = 2 * size + 1
    a, b = list(range(1, size + 1)), list(range(size + 1, n))
    edges = [(x, y) for grp in (a, b) for i, x in enumerate(grp) for y in grp[i + 1:]]
    return graph(n, edges + [(0, b[-1]), (0, a[-1])])


def pendant_of_border():
    """A 4-clique 0..3, row 4 linked to row 3 only, row 5 linked to row 4 only.  With min_samples = 4: the clique rows are core
    (degree 4; row 3 has 5), row 4 (degree 3) is a border row, row 5's only neighbour is not core: noise."""
    link, deg = clique(6, range(4))
    link = link.copy()
    for a, b in ((3, 4), (4, 5)):
        link[a, b] = link[b, a] = True
    return link, degree_ref(link)


def bit_reverse(bits: int) -> np.ndarray:
    i = np.arange(1 << bits)
    r = np.zeros_like(i)
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def path(order) -> tuple:
    """A path that visits the rows in `order`: order[t] -- order[t + 1]."""
    order = np.asarray(order)
    n = len(order)
    link = np.zeros((n, n), bool)
    link[order[:-1], order[1:]] = True
    link[order[1:], order[:-1]] = True
    return link, degree_ref(link)
