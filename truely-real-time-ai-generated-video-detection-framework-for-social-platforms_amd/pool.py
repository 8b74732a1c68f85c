"""Embedding templates on the GPU: several embeddings of one person pooled into one.

    t = pool_embeddings(emb, ids)                     # one row per id: an identity's photos, a track's frames, a cluster's members
    t["template"], t["count"], t["cohesion"]

    p = EmbeddingPool(num_groups)                     # the streaming form: rows arrive in any number of calls
    p.add(emb, ids, weights=probs)
    p.result()

A template is the segmented, optionally weighted mean of unit embeddings, keyed by a group id per row, and its sum is defined in
fixed point ("Templates"; csrc/trl_pool.h is the rule's code, tests/pool_ref.py its reference).  For a pool
over groups 0 .. G - 1, with n2 the gallery's chain of a row (``FaceGallery``'s squared norm):

    ignored      a row whose id lies outside 0 .. G - 1 is counted nowhere: -1 labels (``cluster``'s noise, a tracker's dropped rows)
    contributes  iff 0 < w <= 1 (1.0 without weights; NaN fails) and n2 is finite and >= FLT_MIN; else the row is skipped and counted
    term         c = w / sqrt(n2);  q_k = int64(rint((c * x[k]) * 2**32));  wq = int64(rint(w * 2**32))          float32, one rounding each
    sum          A[g][k] += q_k;  W[g] += wq;  N[g] += 1                                                           integers
    finish       t = float32(A[g]) * 2**-32;  Wf = float32(W[g]) * 2**-32;  template = t / sqrt(n2 t)  (unit)  or  t / Wf  (mean)
                 cohesion = sqrt(n2 t) / Wf: the mean resultant length, 1 for identical rows, near 0 for unrelated ones

Integer addition is associative, so a result is the same bits for any tiling, any split of the rows into calls, any order of the
rows and any stream -- and whether a clip's tracks are pooled window by window as they arrive or all at once afterwards.  A group
without rows gives a template of +0 with count, weight and cohesion 0; a group whose sum cancels to zero gives what the formulas
give (unit: NaN, the gallery's "a zero row gives NaN").  A group takes at most 2**30 contributing rows.

The representative of a group is its contributing row closest to the group's own template -- the largest gallery cosine, bit for
bit ``FaceGallery.scores(template)[g, i]``; ties as floats go to the lower row, a NaN cosine is never chosen, and a group without a
candidate has index -1 and score NaN: "the most representative frame of a person" from embeddings alone.

``FaceGallery.templates`` enrols one template per identity, ``FaceTracker(templates=True)`` keeps one per track, and the clusters
of ``FaceGallery.cluster`` / ``cluster_embeddings`` need nothing more than ``pool_embeddings(emb, labels)`` with their labels."""
from __future__ import annotations

import torch

from . import _lib
from ._tensors import DIM, cuda_device, grown, ptr, rows, stream, vector

MAX_ROWS = 1 << 30                       # contributing rows of one group (csrc/trl_pool.h): the host's count of rows added stays below
ROW_CHUNK = 1 << 20                      # rows of one trl_pool_add call made for a larger input


def _tile(tile_rows) -> int:
    if tile_rows not in (0, 8, 16, 32):
        raise ValueError("tile_rows must be 0 (the default), 8, 16 or 32")
    return int(tile_rows)


def _block(a: int, x, n2, gid, w) -> tuple:
    """Rows a .. a + b - 1 as trl_pool_add and trl_pool_rep_add take them: (rows, ld_rows, n2, gid, w, b).  `x` (b, 512) and `n2`
    (b,) or None are the block's own; `gid` and `w` (or None) cover every row and are cut here."""
    b = x.shape[0]
    return ptr(x), (x.stride(0) if b > 1 else DIM), ptr(n2), ptr(gid[a:a + b]), ptr(None if w is None else w[a:a + b]), b


class EmbeddingPool:
    """The pooled sums of groups 0 .. num_groups - 1 on the device.  ``add`` takes rows in any number of calls and in any order;
    ``result`` finishes what has been added so far and may be called again after more.  No call synchronises."""

    def __init__(self, num_groups: int, device=None, _g0: int = 0):
        self.lib = _lib.load()
        self.device = cuda_device(device, "embeddings are pooled on a GPU")
        self._g0 = int(_g0)
        self._rows_added = 0
        self.num_groups = int(num_groups)
        self._state = torch.zeros((self._words(self.num_groups),), dtype=torch.int64, device=self.device)

    def _words(self, groups: int) -> int:
        """The int64 words of a state of `groups` groups (csrc/trl_pool.h): skipped, W[G], N[G], A[G][512]."""
        nbytes = self.lib.trl_pool_state_bytes(groups)
        if groups < 0 or not nbytes:
            raise ValueError(f"num_groups must be in 0 .. 2**31 - 1, not {groups}")
        return nbytes // 8

    def reset(self) -> None:
        """Forget every row."""
        _lib.check(self.lib.trl_pool_reset(ptr(self._state), self.num_groups, stream(self.device)))
        self._rows_added = 0

    def grow(self, num_groups: int) -> None:
        """Make room for groups up to ``num_groups - 1``: a device copy of the sums; the new groups are empty."""
        g, n = self.num_groups, int(num_groups)
        if n < g:
            raise ValueError(f"a pool of {g} groups cannot shrink to {n}")
        if n == g:
            return
        self._words(n)
        st = self._state                                  # each section grows on its own
        self._state = torch.cat([st[:1], grown(st[1:1 + g], n), grown(st[1 + g:1 + 2 * g], n), grown(st[1 + 2 * g:], DIM * n)])
        self.num_groups = n

    def add(self, emb, groups, weights=None, n2=None, tile_rows: int = 0) -> None:
        """Pool m more rows: ``emb`` (m, 512), ``groups`` (m,) integer ids, ``weights`` (m,) in (0, 1] or None (all 1), ``n2`` (m,)
        the rows' squared norms as ``FaceGallery`` keeps them, or None (they are computed).  A row whose id is outside the pool
        is ignored; a row with a bad weight or norm is skipped and counted in ``result()["skipped"]``."""
        x = rows(emb, self.device, keep_pitch=True)
        m = x.shape[0]
        gid = vector(groups, m, torch.int32, self.device, "groups")
        w = vector(weights, m, torch.float32, self.device, "weights")
        n2 = vector(n2, m, torch.float32, self.device, "n2")
        if self._rows_added + m > MAX_ROWS:
            raise ValueError(f"an EmbeddingPool takes at most 2**30 rows: {self._rows_added} added, {m} more")
        self._rows_added += m
        tile, s = _tile(tile_rows), stream(self.device)
        for a in range(0, m, ROW_CHUNK):
            self._add_block(a, x[a:a + ROW_CHUNK], None if n2 is None else n2[a:a + ROW_CHUNK], gid, w, tile, s)

    def _add_block(self, a: int, x, n2, gid, w, tile: int, s) -> None:
        """The one trl_pool_add call: the block of rows `x` that starts at row `a` of `gid` and `w` (_block)."""
        _lib.check(self.lib.trl_pool_add(ptr(self._state), self.num_groups, self._g0, *_block(a, x, n2, gid, w), tile, s))

    def result(self, unit: bool = True) -> dict:
        """``template`` (G, 512) float32 -- unit rows, or with ``unit=False`` the weighted mean of the unit rows --, ``count`` (G,)
        int32, ``weight`` (G,) float32 (the sum of the contributing rows' weights), ``cohesion`` (G,) float32 and ``skipped``, a
        0-d int64: all on the device."""
        g, d = self.num_groups, self.device
        out = {"template": torch.empty((g, DIM), dtype=torch.float32, device=d), "count": torch.empty((g,), dtype=torch.int32, device=d),
               "weight": torch.empty((g,), dtype=torch.float32, device=d), "cohesion": torch.empty((g,), dtype=torch.float32, device=d)}
        skipped = torch.empty((1,), dtype=torch.int64, device=d)
        _lib.check(self.lib.trl_pool_finish(ptr(self._state), g, 0 if unit else 1, ptr(out["template"]), ptr(out["count"]),
                                            ptr(out["weight"]), ptr(out["cohesion"]), ptr(skipped), stream(d)))
        out["skipped"] = skipped[0]
        return out

    def _representatives(self, template, blocks, gid, w, tile_rows: int = 0):
        """(index (G,) int32, score (G,) float32) of the rows that `blocks` yields -- (first row, rows, n2 or None) -- against
        `template`, this pool's result."""
        g, d, s = self.num_groups, self.device, stream(self.device)
        key = torch.empty((max(g, 1),), dtype=torch.int64, device=d)
        index = torch.empty((g,), dtype=torch.int32, device=d)
        score = torch.empty((g,), dtype=torch.float32, device=d)
        _lib.check(self.lib.trl_pool_rep_reset(ptr(key), g, s))
        for a, x, n2 in blocks():
            *block, m = _block(a, x, n2, gid, w)
            _lib.check(self.lib.trl_pool_rep_add(ptr(key), g, self._g0, ptr(template), *block, a, m, _tile(tile_rows), s))
        _lib.check(self.lib.trl_pool_rep_finish(ptr(key), g, ptr(index), ptr(score), s))
        return index, score


def _pool_blocks(device, blocks, m: int, gid, w, G: int, unit: bool, representative: bool, max_state_bytes: int, tile_rows: int) -> dict:
    """The one-shot pool over rows that `blocks()` yields as (first row, rows (b, 512), n2 or None), in chunks of groups that fit
    `max_state_bytes`: a chunk's pool covers groups g0 .. g0 + c - 1 and ignores the rows of the others, so the bits are those of
    one pool over all."""
    per = max(1, (int(max_state_bytes) - 8) // (514 * 8))
    if m > MAX_ROWS:
        raise ValueError(f"at most 2**30 rows are pooled, not {m}")
    out = {"template": torch.empty((G, DIM), dtype=torch.float32, device=device), "count": torch.empty((G,), dtype=torch.int32, device=device),
           "weight": torch.empty((G,), dtype=torch.float32, device=device), "cohesion": torch.empty((G,), dtype=torch.float32, device=device),
           "skipped": torch.zeros((), dtype=torch.int64, device=device)}
    if representative:
        out["representative"] = torch.empty((G,), dtype=torch.int32, device=device)
        out["rep_score"] = torch.empty((G,), dtype=torch.float32, device=device)
    s = stream(device)
    for g0 in range(0, G, per):
        c = min(per, G - g0)
        p = EmbeddingPool(c, device, _g0=g0)
        for a, x, n2 in blocks():
            p._add_block(a, x, n2, gid, w, _tile(tile_rows), s)
        r = p.result(unit)
        for name in ("template", "count", "weight", "cohesion"):
            out[name][g0:g0 + c].copy_(r[name])
        out["skipped"] += r["skipped"]
        if representative:
            index, score = p._representatives(r["template"], blocks, gid, w, tile_rows)
            out["representative"][g0:g0 + c].copy_(index)
            out["rep_score"][g0:g0 + c].copy_(score)
    return out


def pool_embeddings(emb, groups, num_groups: int | None = None, weights=None, unit: bool = True, representative: bool = False,
                    max_state_bytes: int = 256 << 20, device=None, tile_rows: int = 0) -> dict:
    """``EmbeddingPool``'s result for one set of rows: ``emb`` (m, 512), ``groups`` (m,) ids, ``weights`` (m,) or None.  The ids
    may be ``FaceGallery.cluster`` / ``cluster_embeddings`` labels as they are: -1 (noise) is ignored, so this is "one row per
    discovered person".  ``num_groups=None`` reads ``groups.max() + 1`` back (one synchronisation).  More groups than fit
    ``max_state_bytes`` of sums are pooled in chunks of groups, to the same bits.  ``representative=True`` adds ``representative``
    (G,) int32, each group's row closest to its template (-1 without one), and ``rep_score`` (G,) float32, that row's cosine --
    ``FaceGallery.scores(template)``'s bits."""
    if device is None:
        device = emb.device if isinstance(emb, torch.Tensor) and emb.device.type == "cuda" else None
    device = cuda_device(device, "embeddings are pooled on a GPU")
    x = rows(emb, device, keep_pitch=True)
    m = x.shape[0]
    gid = vector(groups, m, torch.int32, device, "groups")
    w = vector(weights, m, torch.float32, device, "weights")
    if num_groups is None:
        num_groups = max(int(gid.max().item()) + 1, 0) if m else 0
    G = int(num_groups)
    if G < 0:
        raise ValueError("num_groups must not be negative")

    def blocks():
        for a in range(0, m, ROW_CHUNK):
            yield a, x[a:a + ROW_CHUNK], None

    return _pool_blocks(device, blocks, m, gid, w, G, unit, representative, max_state_bytes, tile_rows)
