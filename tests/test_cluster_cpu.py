"""The embedding clustering without a GPU: tests/cluster_ref.py (the reference the GPU tests hold trl_cluster_links and
trl_cluster_labels to) against its own stated structure, against scikit-learn's DBSCAN and scipy's connected components where those
import, and the host-only part of the C ABI."""
import re
import os

import numpy as np
import pytest

import cluster_ref as CR
import gallery_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(metric, thr) for metric in (G.COSINE, G.EUCLIDEAN) for thr in CR.TABLE_THR[metric]]


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_scores_are_symmetric_bit_for_bit(metric):
    s = CR.table_scores(metric)
    assert s.shape == (257, 257) and np.array_equal(s.view(np.uint32), s.T.view(np.uint32))       # NaN payloads included
    assert np.isnan(s).any() and np.array_equal(np.isnan(s), np.isnan(s).T)
    # the leading block is what a call with the first n rows computes, and the queries' table agrees where it holds gallery rows
    g, q = G.tables()
    assert G.same_bits(G.scores_ref(g[:33], g[:33], metric), s[:33, :33]).all()
    assert G.same_bits(G.table_scores(metric)[0], s[G.DUP_OF]).all()


def _structure(labels, core, degree):
    noise = int(((labels < 0) & (degree > 0)).sum())
    border = int(((labels >= 0) & (core == 0)).sum())
    return noise, border


def test_table_cases_are_not_trivial():
    """Figures of the whole table, every row valid: a later edit of the reference or of the table shows here."""
    for metric, thr, ms, want in ((G.COSINE, 0.12, 1, (62, None, None)), (G.COSINE, 0.12, 3, (2, 62, 86)), (G.EUCLIDEAN, 1.3, 4, (2, 193, 55))):
        link, deg = CR.table_links(metric, thr)
        labels, core, count = CR.labels_ref(link, deg, ms)
        noise, border = _structure(labels, core, deg)
        print(metric, thr, ms, "clusters", count, "noise", noise, "border", border, "links", int(link.sum()) // 2)
        assert count == want[0]
        if want[1] is not None:
            assert (noise, border) == want[1:]
        assert set(labels[labels >= 0].tolist()) == set(range(count))
    # min_samples = 1: every valid row is core, nothing is noise or border
    link, deg = CR.table_links(G.COSINE, 0.12)
    labels, core, count = CR.labels_ref(link, deg, 1)
    assert core.all() and (labels >= 0).all()
    # the loose thresholds give a graph with links too, the tight ones keep the duplicates together
    for metric, thr in CASES:
        link, deg = CR.table_links(metric, thr)
        assert link.any() and not link.all(), (metric, thr)
        assert np.array_equal(link, link.T) and not np.diagonal(link).any()
        assert link[np.ix_(G.DUPS, G.DUPS)].sum() == 20, (metric, thr)
    # a NaN score never links, in either metric: the NaN row and (cosine) the zero row keep degree 1
    for metric, thr in CASES:
        _link, deg = CR.table_links(metric, thr)
        assert deg[G.NAN_G] == 1 and (metric == G.EUCLIDEAN or deg[G.ZERO_G] == 1)


def test_border_rows_that_touch_two_clusters():
    """Rows 40, 41 and 200 invalid, cosine 0.12, min_samples 6: four border rows have core neighbours in two clusters, so the
    rule's 'smallest number' decides (an order-dependent DBSCAN could give either)."""
    invalid = (40, 41, 200)
    link, deg = CR.table_links(G.COSINE, 0.12, CR.N_TABLE, invalid)
    assert (deg[list(invalid)] == 0).all() and not link[list(invalid)].any() and not link[:, list(invalid)].any()
    labels, core, count = CR.labels_ref(link, deg, 6)
    assert (labels[list(invalid)] == -1).all() and not core[list(invalid)].any()
    two = 0
    for i in np.nonzero((core == 0) & (labels >= 0))[0]:
        seen = set(labels[link[i] & (core != 0)].tolist())
        assert labels[i] == min(seen)
        two += len(seen) >= 2
    assert two == 4, two


def test_hand_made_graphs():
    link, deg = CR.empty_graph(5)
    assert CR.labels_ref(link, deg, 1)[0].tolist() == [0, 1, 2, 3, 4] and CR.labels_ref(link, deg, 2)[0].tolist() == [-1] * 5
    link, deg = CR.clique(33)
    assert (deg == 33).all() and (CR.labels_ref(link, deg, 33)[0] == 0).all() and (CR.labels_ref(link, deg, 34)[0] == -1).all()
    link, deg = CR.star(40, 17)
    labels, core, count = CR.labels_ref(link, deg, 40)
    assert count == 1 and core.sum() == 1 and core[17] and (labels == 0).all()
    link, deg = CR.two_cliques_and_bridge()
    labels, core, count = CR.labels_ref(link, deg, 4)
    assert count == 2 and not core[0] and labels.tolist() == [0] + [0] * 5 + [1] * 5
    link, deg = CR.pendant_of_border()
    labels, core, count = CR.labels_ref(link, deg, 4)
    assert labels.tolist() == [0, 0, 0, 0, 0, -1] and core.tolist() == [1, 1, 1, 1, 0, 0] and count == 1
    for order in (np.arange(64), np.arange(64)[::-1], CR.bit_reverse(6)):
        link, deg = CR.path(order)
        labels, core, count = CR.labels_ref(link, deg, 1)
        assert count == 1 and (labels == 0).all() and sorted(deg.tolist()) == [2, 2] + [3] * 62
    # invalid rows (degree 0) are never core, even at min_samples = 1
    link, deg = CR.empty_graph(3)
    deg = deg.copy(); deg[1] = 0
    assert CR.labels_ref(link, deg, 1)[0].tolist() == [0, -1, 1]


def test_bitmap_packer():
    rng = np.random.default_rng(5)
    for n in (1, 31, 32, 33, 65):
        link = rng.random((n, n)) < 0.3
        adj = CR.pack_bitmap(link, (n + 31) // 32 + 2)
        assert adj.dtype == np.uint32 and adj.shape == (n, (n + 31) // 32 + 2) and not adj[:, (n + 31) // 32:].any()
        for i, j in ((0, 0), (n - 1, n - 1), (0, n - 1), (n // 2, n // 3)):
            assert bool(adj[i, j // 32] >> np.uint32(j % 32) & 1) == link[i, j]
        assert np.array_equal(CR.unpack_bitmap(adj, n), link)
        assert int(sum(bin(int(w)).count("1") for w in adj.ravel())) == int(link.sum())             # no bit at a column >= n


def test_reference_equals_sklearn_and_scipy():
    """The order-free rule IS scikit-learn's DBSCAN on these graphs (borders that touch two clusters included), and at
    min_samples = 1 scipy's component count."""
    cluster = pytest.importorskip("sklearn.cluster")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    invalid = (40, 41, 200)
    ok = CR.mask(CR.N_TABLE, invalid) != 0
    for metric, thr in CASES + [(G.COSINE, 0.5), (G.COSINE, 0.05), (G.EUCLIDEAN, 20.0)]:
        link, deg = CR.table_links(metric, thr, CR.N_TABLE, invalid)
        sub = link[np.ix_(ok, ok)]                        # (scikit-learn has no invalid rows: they are left out and put back)
        D = np.where(sub, 0.0, 1.0)
        np.fill_diagonal(D, 0.0)
        for ms in CR.MIN_SAMPLES:
            labels, core, count = CR.labels_ref(link, deg, ms)
            m = cluster.DBSCAN(eps=0.5, min_samples=ms, metric="precomputed").fit(D)
            assert np.array_equal(labels[ok], m.labels_), (metric, thr, ms)
            assert np.array_equal(np.nonzero(core[ok])[0], m.core_sample_indices_)
            assert (labels[~ok] == -1).all()
        assert CR.labels_ref(link, deg, 1)[2] == csgraph.connected_components(sub, directed=False)[0]


def test_abi_declares_cluster():
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_cluster_links", "trl_cluster_workspace", "trl_cluster_labels"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.trl_abi_version() == 7
    # host-only: the label stage's workspace is a few words per row, nothing like the bitmap
    assert lib.trl_cluster_workspace(0) <= 1024 and lib.trl_cluster_workspace(-1) == 0 and lib.trl_cluster_workspace(CR.MAX_N + 1) == 0
    assert 12 * CR.MAX_N <= lib.trl_cluster_workspace(CR.MAX_N) <= 12 * CR.MAX_N + 4096
    assert lib.trl_cluster_workspace(257) >= 3 * 257 * 4
    import truely_amd
    assert "cluster_embeddings" in truely_amd.__all__
