"""The gallery range search without a GPU: tests/range_ref.py (the reference the GPU tests hold trl_gallery_range_count / _fill to)
against the clustering's link matrix and against the figures its table is known by, and the host-only parts of the C ABI -- the
declarations, the exports and the workspace sizes."""
import os
import re

import numpy as np
import pytest

import cluster_ref as CR
import gallery_ref as G
import range_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"trl_gallery_range_workspace", "trl_gallery_range_count", "trl_gallery_range_fill"}

# (metric, threshold): (hits of 65 x 257, empty rows or None, longest row) of the query table against the gallery table
TABLE_FIGURES = {
    (G.COSINE, 0.12): (214, 11, 109), (G.COSINE, 0.999): (161, 27, 109), (G.COSINE, -2.0): (15011, None, 253),
    (G.EUCLIDEAN, 1.3): (215, 46, 59), (G.EUCLIDEAN, 31.0): (7932, 3, 254), (G.EUCLIDEAN, 1e30): (15748, None, 254),
}


def test_abi_declares_the_range_search():
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    assert NAMES <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and NAMES <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.trl_abi_version() == 7
    assert "#define TRL_ABI_VERSION 7" in hdr


def test_workspace_sizes():
    from truely_amd import _lib
    ws = _lib.load().trl_gallery_range_workspace
    for args in ((-1, 33, 0), (33, -1, 0), (33, 1 << 31, 0), (33, 33, 100), (33, 33, -128), (33, 33, 64)):
        assert ws(*args) == 0, args                                            # refused arguments
    assert ws(0, 33, 0) == 0 and ws(33, 0, 0) == 0 and ws(0, 0, 0) == 0        # nothing to count: nothing needed
    # one uint32 per (strip, wave, row), 4 waves
    assert ws(1, 1, 0) == 1 * 4 * 1 * 4
    assert ws(33, 257, 128) == 3 * 4 * 33 * 4
    sizes = [ws(32768, 512, cols) for cols in (0, 256, 128)]                   # 1, 2 and 4 strips of 1,024 row tiles
    assert sizes == [s * 4 * 32768 * 4 for s in (1, 2, 4)]
    big = [ws(1024, 1 << 20, cols) for cols in (0, 1 << 16, 1 << 12, 128)]
    assert all(a <= b for a, b in zip(big, big[1:])) and big[0] < big[-1]      # monotone in the strip count
    assert big[0] == 16 * 4 * 1024 * 4                                         # 16 strips of 32 row tiles: 256 KB ...
    assert big[0] * 256 < 1024 * (1 << 20) // 8                                # ... where n x m bits would take 128 MB
    assert ws(1024, 1 << 30, 0) == big[0]                                      # and it does not grow with m


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_reference_lists_are_the_link_matrix(metric):
    """Self mode: the unpacked lists are cluster_ref's links, with and without invalid rows; the scores beside the indices are the
    matrix's own."""
    n = CR.N_TABLE
    s = CR.table_scores(metric)
    for thr in CR.TABLE_THR[metric]:
        for valid in (None, CR.mask(n)):
            off, idx, sc = R.range_ref(s, metric, thr, valid, valid, skip_self=True)
            link = CR.links_ref(s, metric, thr, valid)
            assert np.array_equal(R.unpack(off, idx, n, n), link) and link.any()
            assert np.array_equal(np.diff(off), CR.degree_ref(link, valid) - (1 if valid is None else (valid != 0)))
            rows = np.repeat(np.arange(n), np.diff(off))
            assert G.same_bits(sc, s[rows, idx]).all() and idx.dtype == np.int32 and off.dtype == np.int64 and sc.dtype == np.float32
    # without skip_self the diagonal is back wherever a row matches itself
    off, idx, _sc = R.range_ref(s, metric, CR.TABLE_THR[metric][0], skip_self=False)
    with np.errstate(invalid="ignore"):
        plain = (s >= np.float32(CR.TABLE_THR[metric][0])) if metric == G.COSINE else (s <= np.float32(CR.TABLE_THR[metric][0]))
    assert np.array_equal(R.unpack(off, idx, n, n), plain) and np.diagonal(plain).sum() > 200


@pytest.mark.parametrize("key", sorted(TABLE_FIGURES))
def test_reference_on_the_query_table(key):
    """The figures the GPU tests' shared table is known by: empty rows, rows across several slabs and strips, nearly full rows."""
    metric, thr = key
    hits, empty, longest = TABLE_FIGURES[key]
    s = G.table_scores(metric)
    off, idx, sc = R.range_ref(s, metric, thr)
    per_row = np.diff(off)
    assert off[-1] == len(idx) == len(sc) == hits and per_row.max() == longest
    if empty is not None:
        assert (per_row == 0).sum() == empty
    assert not np.isnan(sc).any()
    if thr in R.LOOSE_THR.values():
        assert hits == (~np.isnan(s)).sum() - (np.isinf(s) & (s < 0 if metric == G.COSINE else s > 0)).sum()


def test_match_rule_on_special_values():
    """Thresholds equal to a score and one ulp either side, +-0, +-inf and NaN of both signs: inclusive, plain float32."""
    f = np.float32
    nan = [f(np.nan), -f(np.nan)]
    for x in (f(0.25), f(-0.0), f(0.0), f(1.0), f(2.0 ** -140)):
        up, down = np.nextafter(x, f(np.inf)), np.nextafter(x, f(-np.inf))
        assert R.match_ref(G.COSINE, x, x) and R.match_ref(G.EUCLIDEAN, x, x)
        assert not R.match_ref(G.COSINE, x, up) and R.match_ref(G.COSINE, x, down)
        assert R.match_ref(G.EUCLIDEAN, x, up) and not R.match_ref(G.EUCLIDEAN, x, down)
    assert R.match_ref(G.COSINE, f(0.0), f(-0.0)) and R.match_ref(G.COSINE, f(-0.0), f(0.0))
    assert R.match_ref(G.COSINE, f(np.inf), f(3e38)) and not R.match_ref(G.COSINE, -f(np.inf), f(-3e38))
    assert not R.match_ref(G.EUCLIDEAN, f(np.inf), f(3e38)) and R.match_ref(G.EUCLIDEAN, -f(np.inf), f(-3e38))
    for x in nan:
        assert not R.match_ref(G.COSINE, x, f(-3e38)) and not R.match_ref(G.EUCLIDEAN, x, f(3e38))
