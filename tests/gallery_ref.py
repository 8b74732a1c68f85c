"""Reference of the embedding match (csrc/trl_gallery.hip) and the inputs its tests share.

For a query row q and a gallery row g of 512 float32:

    dot(q, g) = chain(0; k = 0..511 ascending: acc = fmaf(q[k], g[k], acc))          one float32 fma chain
    n2(x)     = dot(x, x)
    cosine    = dot / (sqrtf(n2 q) * sqrtf(n2 g))                                     larger is better, a zero row gives NaN
    euclidean = s = n2 q + n2 g; d2 = fmaf(-2, dot, s); d2 < 0 ? 0 : d2; sqrtf(d2)    smaller is better (NaN stays NaN)

restated on front_ref.fma32 (the exact float32 fma; a step with an infinite or NaN operand is taken in float64, as
logits_ref.logits_ref does).  numpy's float32 sqrt, multiply, add and divide round once, as the device's do.

The order of matches is the explicit sort key (is_nan, -score | +score, index): not-NaN before NaN, better score first, the
lower gallery index among equal scores (floats: -0 == +0) and among NaN.  Slots past the gallery, and every slot of a row whose
valid entry is 0, are (index -1, score NaN)."""
from __future__ import annotations

import functools

import numpy as np

from front_ref import fma32
from logits_ref import gamma, logits_ref, same_bits  # noqa: F401  (re-exported for the tests)

F32 = np.float32
K = 512
COSINE, EUCLIDEAN = 0, 1
METRICS = {"cosine": COSINE, "euclidean": EUCLIDEAN}
U = 2.0 ** -24


def _fma_any(a, b, c):
    """fma32 where all operands are finite, the float64 expression elsewhere (no rounding is left to get wrong there)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        out = fma32(a, b, c)
        bad = ~(np.isfinite(a) & np.isfinite(b) & np.isfinite(c))
        if bad.any():
            plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
            out = np.where(bad, plain, out)
    return out.astype(F32)


def dot_ref(q: np.ndarray, g: np.ndarray) -> np.ndarray:
    """q (n, 512), g (m, 512) -> (n, m): the chain, which is logit[r][c] with w = g^T and a zero bias."""
    g = np.asarray(g, F32)
    return logits_ref(q, np.ascontiguousarray(g.T), np.zeros(g.shape[0], F32))


def n2_ref(x: np.ndarray) -> np.ndarray:
    """x (r, 512) -> (r,): the chain of each row with itself."""
    x = np.asarray(x, F32)
    acc = np.zeros(x.shape[0], F32)
    for k in range(K):
        acc = _fma_any(x[:, k], x[:, k], acc)
    return acc


def scores_from(dot: np.ndarray, qn2: np.ndarray, gn2: np.ndarray, metric: int) -> np.ndarray:
    dot, qn2, gn2 = np.asarray(dot, F32), np.asarray(qn2, F32), np.asarray(gn2, F32)
    with np.errstate(all="ignore"):
        if metric == COSINE:
            den = np.sqrt(qn2)[:, None] * np.sqrt(gn2)[None, :]
            out = dot / den
        else:
            s = qn2[:, None] + gn2[None, :]
            d2 = _fma_any(F32(-2.0), dot, s)
            d2 = np.where(d2 < 0, F32(0), d2)
            out = np.sqrt(d2)
    assert out.dtype == F32
    return out


def scores_ref(q: np.ndarray, g: np.ndarray, metric: int, block: int = 4096) -> np.ndarray:
    """(n, m) scores; gallery rows are taken `block` at a time."""
    q, g = np.asarray(q, F32), np.asarray(g, F32)
    qn2 = n2_ref(q)
    out = np.empty((q.shape[0], g.shape[0]), F32)
    for c0 in range(0, g.shape[0], block):
        gb = g[c0:c0 + block]
        out[:, c0:c0 + block] = scores_from(dot_ref(q, gb), qn2, n2_ref(gb), metric)
    return out


def order_ref(scores: np.ndarray, metric: int) -> np.ndarray:
    """Indices of one row of scores in match order: sort key (is_nan, -score | +score, index)."""
    s = np.asarray(scores, F32)
    nan = np.isnan(s)
    key = np.where(nan, F32(0), -s if metric == COSINE else s)
    return np.lexsort((np.arange(len(s)), key, nan))           # (the last key is the primary one)


def topk_ref(scores: np.ndarray, metric: int, k: int, valid: np.ndarray | None = None):
    """scores (n, m) -> (index (n, k) int32, score (n, k) float32)."""
    n, m = scores.shape
    idx = np.full((n, k), -1, np.int32)
    sc = np.full((n, k), np.nan, F32)
    for r in range(n):
        if valid is not None and not valid[r]:
            continue
        o = order_ref(scores[r], metric)[:k]
        idx[r, :len(o)] = o
        sc[r, :len(o)] = scores[r, o]
    return idx, sc


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
M_TABLE, N_TABLE = 257, 65
DUP_OF, DUPS = 2, (2, 33, 129, 200, 256)        # one row five times: in three 128-column groups, so in three 128-column strips
NEG_OF_DUP = 7
ZERO_G, NAN_G, INF_G, MIXINF_G = 3, 9, 10, 11
NEAR_PAIRS = ((14, 15), (60, 61), (126, 130))   # rows one or two ulps apart in one element: cosines that differ in the last bit, or tie


@functools.lru_cache(maxsize=None)
def tables():
    """(gallery (257, 512), queries (65, 512)), read-only.  Gallery: random normal rows; rows 16..30 and 140..180 L2-normalised; a
    zero row; one-hot rows; the duplicates; a negated duplicate; rows holding NaN and +-inf; rows in the subnormal range; the near
    pairs.  Queries: random normal and normalised rows, and at fixed places (inside the first tile, on both sides of the 32-row
    tile edge, the lone row of the third tile) the duplicated gallery row, its negation, a zero row, one-hot rows, NaN, inf and
    subnormal rows, and near-copies of gallery rows."""
    rng = np.random.default_rng(20260)
    g = rng.standard_normal((M_TABLE, K)).astype(F32)
    for r in list(range(16, 31)) + list(range(140, 181)):
        g[r] = g[r] / np.sqrt((g[r] * g[r]).sum(dtype=F32))
    for r in DUPS:
        g[r] = g[DUP_OF]
    g[NEG_OF_DUP] = -g[DUP_OF]
    g[ZERO_G] = 0
    g[5] = 0; g[5, 0] = 1
    g[6] = 0; g[6, 511] = -2
    g[NAN_G, 100] = np.nan
    g[INF_G, 7] = np.inf
    g[MIXINF_G, 7] = np.inf; g[MIXINF_G, 300] = -np.inf
    g[12] = (rng.standard_normal(K) * 2.0 ** -126).astype(F32)
    g[13, ::3] = (rng.standard_normal(len(g[13, ::3])) * 2.0 ** -140).astype(F32)
    g[128] = 0; g[128, 255] = 3
    for a, b in NEAR_PAIRS:
        g[b] = g[a]
        g[b, 17] = np.nextafter(g[b, 17], F32(np.inf))
    g[61, 400] = np.nextafter(g[61, 400], F32(-np.inf))
    q = rng.standard_normal((N_TABLE, K)).astype(F32)
    for r in range(8, 16):
        q[r] = q[r] / np.sqrt((q[r] * q[r]).sum(dtype=F32))
    q[0] = g[DUP_OF]                                       # scores tie across the duplicates; cosine of a row with itself
    q[1] = 0
    q[2] = 0; q[2, 0] = 1
    q[3, 511] = np.nan
    q[4, 7] = np.inf
    q[5] = (rng.standard_normal(K) * 2.0 ** -126).astype(F32)
    q[6] = -g[DUP_OF]
    q[7] = g[14]                                           # the near pair seen from one of its own rows
    q[30] = g[60]
    q[31] = 0
    q[32] = g[DUP_OF]
    q[33] = 0; q[33, 255] = -1
    q[63, 0] = np.nan
    q[64] = g[126]
    g.setflags(write=False)
    q.setflags(write=False)
    return g, q


def zero_sign_rows():
    """(gallery (6, 512), query (1, 512)) whose cosines are, in gallery order: +0, -0.5.., -0, +0, -0, 1: the dots of rows 2 and 4
    are -0 (an underflowing negative first product, then only products that are -0), those of rows 0 and 3 are +0."""
    q = np.zeros((1, K), F32)
    q[0, 0] = 2.0 ** -100; q[0, 1] = 1
    g = np.zeros((6, K), F32)
    g[0, 2] = 3
    g[1, 1] = -1; g[1, 2] = 1.5
    g[2] = -0.0; g[2, 0] = -2.0 ** -100; g[2, 2] = -5
    g[3, 5] = 1
    g[4] = -0.0; g[4, 0] = -2.0 ** -120; g[4, 3] = -7
    g[5, 1] = 2
    return g, q


@functools.lru_cache(maxsize=None)
def table_scores(metric: int) -> np.ndarray:
    """scores_ref of the query table against the gallery table, (65, 257), computed once per metric."""
    g, q = tables()
    s = scores_ref(q, g, metric)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def table_n2() -> np.ndarray:
    r = n2_ref(tables()[0])
    r.setflags(write=False)
    return r
