"""Reference of the grouped search (csrc/trl_gallery_groups.h, k_gallery_search_groups) and the group-id tables
its tests share.

Every gallery row c carries a group id gid[c] (int32); a row with gid[c] < 0 is excluded.  For one query:

  1. take the rows that are not excluded in the match order (gallery_ref.order_ref: better score first, equal scores to the lower
     index, NaN after every other);
  2. keep a row iff no earlier row in that order has the same gid;
  3. the first k kept rows are the result, (score, index, group);
  4. slots past the last kept row, and every slot of a row with valid[r] == 0, hold (NaN, -1, -1).

With all gids distinct this is gallery_ref.topk_ref."""
from __future__ import annotations

import functools

import numpy as np

import gallery_ref as G


def group_topk_ref(scores: np.ndarray, gid: np.ndarray, metric: int, k: int, valid: np.ndarray | None = None):
    """scores (n, m), gid (m,) -> (score (n, k) float32, index (n, k) int32, group (n, k) int32)."""
    n, m = scores.shape
    gid = np.asarray(gid, np.int32)
    assert gid.shape == (m,)
    sc = np.full((n, k), np.nan, G.F32)
    idx = np.full((n, k), -1, np.int32)
    grp = np.full((n, k), -1, np.int32)
    for r in range(n):
        if valid is not None and not valid[r]:
            continue
        seen, e = set(), 0
        for c in G.order_ref(scores[r], metric):
            g = int(gid[c])
            if g < 0 or g in seen:
                continue
            seen.add(g)
            sc[r, e], idx[r, e], grp[r, e] = scores[r, c], c, g
            e += 1
            if e == k:
                break
    return sc, idx, grp


# ---- shared group-id tables over gallery_ref.tables()' 257 rows -------------------------------------------------------------------
SPECIAL_G = (G.ZERO_G, G.NAN_G, G.INF_G, G.MIXINF_G)     # rows whose scores are NaN / inf under one metric or both; groups 36..39
PARTNER_G = (100, 101, 102, 103)                         # the ordinary rows they share their groups with in "random_shared"


@functools.lru_cache(maxsize=None)
def gid_tables() -> dict:
    """name -> gid (257,) int32, read-only.  tests/test_gpu_groups.py says what each exercises.  The three random tables draw groups
    0..35 and put -1 at 25 scattered rows behind the first slab; groups 36..39 are the special rows', each alone in its group
    ("random_alone") or sharing it with an ordinary row ("random_shared"); "random_slab" excludes the whole first slab as well."""
    i = np.arange(G.M_TABLE, dtype=np.int32)
    rng = np.random.default_rng(1107)
    rnd = rng.integers(0, 36, G.M_TABLE).astype(np.int32)
    rnd[rng.choice(np.arange(32, G.M_TABLE), 25, replace=False)] = -1
    rnd[list(SPECIAL_G)] = np.arange(36, 40)
    shared = rnd.copy()
    shared[list(PARTNER_G)] = np.arange(36, 40)
    slab = shared.copy()
    slab[:32] = -1
    t = {"distinct": i, "one": np.zeros_like(i), "mod3": i % 3, "div16": i // 16, "div32": i // 32, "div128": i // 128,
         "random_alone": rnd, "random_shared": shared, "random_slab": slab}
    for v in t.values():
        v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def table_group_topk(metric: int, name: str, m: int, k: int):
    """group_topk_ref of the query table against the first m gallery rows under gid table `name`, computed once."""
    return group_topk_ref(G.table_scores(metric)[:, :m], gid_tables()[name][:m], metric, k)
