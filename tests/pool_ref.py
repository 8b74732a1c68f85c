"""Reference of embedding templates (csrc/trl_pool.h, csrc/trl_pool.hip; DESIGN.md section 2, "Templates") and the inputs its tests
share.  The sum is fixed point, so the reference is numpy int64 on gallery_ref's chain.

A state covers groups g0 .. g0 + G - 1; x[i] is a row of 512 float32, gid[i] its int32 id, w[i] its weight (1.0 when absent):

  1. n2_i = gallery_ref.n2_ref(x_i), trl_gallery_pack's bits
  2. row i is IGNORED (counted nowhere) when gid[i] is outside the state's groups
  3. otherwise it CONTRIBUTES iff 0 < w_i <= 1 (NaN fails) and n2_i is finite and >= FLT_MIN; else it is SKIPPED and counted
  4. c = w_i / sqrtf(n2_i); p_k = c * x[i][k]; q_k = int64(rintf(p_k * 2**32)); wq = int64(rintf(w_i * 2**32))
  5. A[g][k] += q_k; W[g] += wq; N[g] += 1                                              integers: any order, any split
  6. t_k = float32(A[g][k]) * 2**-32; Wf = float32(W[g]) * 2**-32; n2t = chain(t); template = t / sqrtf(n2t) (unit) or t / Wf (mean);
     cohesion = sqrtf(n2t) / Wf; count = N[g]; weight = Wf
  7. N[g] == 0: template +0, weight 0, cohesion 0
  8. representative of g against a template row T_g: the contributing row of g with the largest gallery cosine
     chain(x_i, T_g) / (sqrtf(n2_i) * sqrtf(chain(T_g, T_g))) -- gallery_ref.scores_from's bits for query T_g --, ties as floats to the
     lower row, a NaN cosine never chosen; no candidate: index -1, score NaN."""
from __future__ import annotations

import functools

import numpy as np

import gallery_ref as G
import group_ref as GR

F32 = G.F32
K = G.K
U = G.U
FLT_MIN = float(np.finfo(F32).tiny)
IGNORED, SKIPPED, CONTRIBUTES = 0, 1, 2
UNIT, MEAN = 0, 1
TILES = (8, 32)                          # tile_rows the GPU tests force: the smallest the kernels support, and the default


def weights_of(w, m: int) -> np.ndarray:
    return np.ones(m, F32) if w is None else np.asarray(w, F32)


def classify(n2, gid, w, G_: int, g0: int = 0) -> np.ndarray:
    """Rules 2 and 3, row by row -> IGNORED / SKIPPED / CONTRIBUTES."""
    n2, w, gid = np.asarray(n2, F32), np.asarray(w, F32), np.asarray(gid, np.int64)
    with np.errstate(invalid="ignore"):
        ok = (w > 0) & (w <= 1) & np.isfinite(n2) & (n2 >= F32(FLT_MIN))
    inside = (gid >= g0) & (gid < g0 + G_)
    return np.where(inside, np.where(ok, CONTRIBUTES, SKIPPED), IGNORED).astype(np.int32)


def quantise(x, n2, w):
    """Rule 4 for contributing rows: (q (r, 512) int64, wq (r,) int64, p (r, 512) float32)."""
    x, n2, w = np.asarray(x, F32), np.asarray(n2, F32), np.asarray(w, F32)
    c = (w / np.sqrt(n2)).astype(F32)
    p = (c[:, None] * x).astype(F32)
    q = np.rint(p * F32(2.0 ** 32)).astype(np.int64)
    wq = np.rint(w * F32(2.0 ** 32)).astype(np.int64)
    assert c.dtype == F32 and p.dtype == F32
    return q, wq, p


def empty_state(G_: int) -> dict:
    return {"A": np.zeros((G_, K), np.int64), "W": np.zeros(G_, np.int64), "N": np.zeros(G_, np.int64), "skipped": 0}


def accumulate(state: dict, x, gid, w=None, g0: int = 0, n2=None) -> dict:
    """Rules 1-5: the rows added to `state` (in place; also returned)."""
    x = np.asarray(x, F32).reshape(-1, K)
    gid = np.asarray(gid, np.int64)
    w = weights_of(w, len(x))
    n2 = G.n2_ref(x) if n2 is None else np.asarray(n2, F32)
    cls = classify(n2, gid, w, len(state["W"]), g0)
    rows = np.nonzero(cls == CONTRIBUTES)[0]
    q, wq, _p = quantise(x[rows], n2[rows], w[rows])
    g = gid[rows] - g0
    np.add.at(state["A"], g, q)
    np.add.at(state["W"], g, wq)
    np.add.at(state["N"], g, 1)
    state["skipped"] += int((cls == SKIPPED).sum())
    return state


def finish(state: dict, mode: int = UNIT) -> dict:
    """Rules 6 and 7 -> template (G, 512) f32, count (G,) int32, weight, cohesion (G,) f32, skipped."""
    A, W, N = state["A"], state["W"], state["N"]
    t = A.astype(F32) * F32(2.0 ** -32)
    wf = W.astype(F32) * F32(2.0 ** -32)
    with np.errstate(all="ignore"):
        sq = np.sqrt(G.n2_ref(t)) if len(t) else np.zeros(0, F32)
        tmpl = t / sq[:, None] if mode == UNIT else t / wf[:, None]
        coh = sq / wf
    empty = N == 0
    tmpl = np.where(empty[:, None], F32(0), tmpl).astype(F32)
    return {"template": tmpl, "count": N.astype(np.int32), "weight": np.where(empty, F32(0), wf).astype(F32),
            "cohesion": np.where(empty, F32(0), coh).astype(F32), "skipped": int(state["skipped"])}


def pool_ref(x, gid, w, G_: int, mode: int = UNIT, n2=None) -> dict:
    return finish(accumulate(empty_state(G_), x, gid, w, 0, n2), mode)


def representative_ref(x, gid, w, template, n2=None):
    """Rule 8 -> (index (G,) int32, score (G,) float32)."""
    x = np.asarray(x, F32).reshape(-1, K)
    template = np.asarray(template, F32)
    G_ = len(template)
    n2 = G.n2_ref(x) if n2 is None else np.asarray(n2, F32)
    cls = classify(n2, gid, weights_of(w, len(x)), G_)
    index = np.full(G_, -1, np.int32)
    score = np.full(G_, np.nan, F32)
    if not len(x) or not G_:
        return index, score
    s = G.scores_from(G.dot_ref(template, x), G.n2_ref(template), n2, G.COSINE)       # (G, m)
    for g in range(G_):
        best = -1
        for i in np.nonzero((cls == CONTRIBUTES) & (np.asarray(gid) == g))[0]:
            if not np.isnan(s[g, i]) and (best < 0 or s[g, i] > s[g, best]):
                best = i
        if best >= 0:
            index[g], score[g] = best, s[g, best]
    return index, score


def mean64(x, gid, w, G_: int):
    """The float64 sum of w_i x_i / |x_i| per group over the contributing rows (what t approximates), the per-group sum of
    |w_i x_i / |x_i|| per element (for the bound) and the count: (sum (G, 512), abs (G, 512), count (G,))."""
    x = np.asarray(x, F32).reshape(-1, K)
    w = weights_of(w, len(x))
    cls = classify(G.n2_ref(x), gid, w, G_)
    s, a, n = np.zeros((G_, K)), np.zeros((G_, K)), np.zeros(G_, np.int64)
    for i in np.nonzero(cls == CONTRIBUTES)[0]:
        xi = x[i].astype(np.float64)
        v = float(w[i]) * xi / np.sqrt((xi * xi).sum())
        s[gid[i]] += v
        a[gid[i]] += np.abs(v)
        n[gid[i]] += 1
    return s, a, n


def sum_bound(abs_sum, count, t) -> np.ndarray:
    """|t_k - sum_i w_i x_ik / |x_i|| <= this, per group and element; derived, not tuned.  abs_sum (G, 512): the sum of the terms'
    magnitudes; count (G,); t (G, 512): the finished float32 sums.

    One term.  n2 is a chain of 512 fmaf, so n2 = |x|^2 (1 + d1) with |d1| <= gamma_512 (the rows of the tables are far from the
    underflow threshold or are skipped; a product that underflows loses at most 2^-149, which the last term below covers with room).
    sqrtf, the division and the product round once each: p = w x / |x| * (1 + d3)(1 + d4) / (sqrt(1 + d1) (1 + d2)), |d2..4| <= u, so
    |p - v| <= |v| rel with rel = (1 + u)^2 / (sqrt(1 - gamma_512) (1 - u)) - 1, which is gamma_512 / 2 + 3 u to first order.
    p * 2^32 is exact and rintf moves it by at most half a unit: 2^-33.  A result in the subnormal range adds at most 2^-149.
    The sum of the integers is exact, so the terms' errors add: abs_sum * rel + count * (2^-33 + 2^-149).
    The finish rounds the int64 sum S to float32 once, |t - S| <= u |S| <= u |t| / (1 - u); the scaling by 2^-32 is exact."""
    g = G.gamma(K)
    rel = (1 + U) ** 2 / (np.sqrt(1 - g) * (1 - U)) - 1
    return abs_sum * rel + np.asarray(count, np.float64)[:, None] * (2.0 ** -33 + 2.0 ** -149) + U * np.abs(np.asarray(t, np.float64)) / (1 - U)


# ---- shared inputs: gallery_ref.tables()' 257 rows under id patterns and weight sets --------------------------------------------------
M = G.M_TABLE
SKIPPED_ROWS = (G.ZERO_G, G.NAN_G, G.INF_G, G.MIXINF_G, 12)     # zero, NaN, inf, +-inf, subnormal: n2 is 0, NaN, inf, NaN, 0


@functools.lru_cache(maxsize=None)
def gid_tables() -> dict:
    """name -> (gid (257,) int32, G).  group_ref's one / distinct / div16 / mod3; "runs": runs of 5, 11, 3, 13, ... rows whose ends
    fall on both sides of every edge of both tile sizes (runs end at, one before and one after multiples of 8 and of 32);
    "outside": ids -1, G, G + 5 and INT32_MIN / INT32_MAX among ids 0..5, which rule 2 ignores; "dups": the five copies of the
    duplicated row alone in group 1, the rows with a NaN / inf n2 alone in group 2, the rest in group 0."""
    t = GR.gid_tables()
    out = {"one": (t["one"], 1), "distinct": (t["distinct"], M), "div16": (t["div16"], 17), "mod3": (t["mod3"], 3)}
    ends = sorted({e + d for tile in TILES for e in range(tile, M, tile) for d in (-1, 0, 1) if (e // tile) % 3 != 1} | {M})
    runs = np.zeros(M, np.int32)
    a = 0
    for g, b in enumerate(ends):
        runs[a:b] = g % 17
        a = b
    out["runs"] = (runs, 17)
    rng = np.random.default_rng(515)
    outside = rng.integers(0, 6, M).astype(np.int32)
    outside[rng.choice(M, 60, replace=False)] = rng.choice(np.array([-1, 6, 11, -2 ** 31, 2 ** 31 - 1], np.int64), 60).astype(np.int32)
    outside[[0, 7, 8, 31, 32, 256]] = [-1, 6, -1, 5, 6, -1]
    out["outside"] = (outside, 6)
    dups = np.zeros(M, np.int32)
    dups[list(G.DUPS)] = 1
    dups[[G.NAN_G, G.INF_G, G.MIXINF_G]] = 2
    out["dups"] = (dups, 4)                                         # (group 3 has no rows at all)
    for v, _g in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def weight_tables() -> dict:
    """name -> weights (257,) float32 or None.  "edge" holds, among random weights in (0, 1], the values rule 3 decides on: 0, -0,
    a negative, 1 + ulp, NaN, +inf (all skipped), and 1, the smallest subnormal and FLT_MIN (all contributing)."""
    rng = np.random.default_rng(516)
    rnd = (1.0 - rng.random(M)).astype(F32)                          # (0, 1]
    edge = (1.0 - rng.random(M)).astype(F32)
    edge[[1, 20, 40, 41, 64, 65, 100, 130, 131]] = [0.0, -0.0, -0.5, np.nextafter(F32(1), F32(2)), np.nan, np.inf, 1.0, 2.0 ** -149, FLT_MIN]
    out = {"none": None, "ones": np.ones(M, F32), "random": rnd, "edge": edge}
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


EDGE_SKIPPED = (1, 20, 40, 41, 64, 65)


@functools.lru_cache(maxsize=None)
def table_ref(ids: str, weights: str, mode: int, m: int = M) -> dict:
    """pool_ref of the first m table rows under an id pattern and a weight set, computed once (n2 from gallery_ref.table_n2)."""
    gid, G_ = gid_tables()[ids]
    w = weight_tables()[weights]
    r = pool_ref(G.tables()[0][:m], gid[:m], None if w is None else w[:m], G_, mode, n2=G.table_n2()[:m])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r
