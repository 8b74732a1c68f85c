"""The score histograms on the device (trl_gallery_hist, csrc/trl_gallery.hip) against tests/hist_ref.py, exactly: integer counts
compared with np.array_equal; the refusals; the clustering's degrees as a second witness; gallery.py on top.

k_gallery_hist has k_gallery_links' frame (row tiles of 32, 32 columns per wave, 128 per workgroup, strips of column groups), so
the gallery table's first n rows against themselves are taken at the n of tests/test_gpu_cluster.py -- a lone row, a tile short of
/ equal to / past 32, a diagonal that crosses tiles and groups, a lone column in the third group -- in both pair modes, and the
65-row query table against the first m gallery rows.  Every shape runs with both metrics, the TIES edges (scores that equal edges)
and one other edge set, with and without the INVALID mask on rows and on columns, with default and 128-column strips, d_q at a 16-
and a 4-byte aligned address.  The counts lie in a prefilled buffer with a guard slot on either side; the workspace is exactly
the size asked for, with a guard behind it; rows and ids lying behind n and m in memory are other rows' -- not zeros."""
import ctypes as C_
import inspect

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
import cluster_ref as CR
import gallery_ref as G
import hist_ref as H

pytestmark = pytest.mark.gpu

TABLE_N = (1, 2, 31, 32, 33, 64, 65, 129, 257)
QUERY_M = (1, 31, 32, 33, 128, 129, 257)
ALL, UPPER = 0, 1
FILL = -0x5A5A5A5A5A5A5A5B
WS_GUARD = 256
TRL_ERR_INVALID = -1


def _ptr(t):
    return C_.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _dev(rows: np.ndarray, misalign: bool = False) -> torch.Tensor:
    rows = np.ascontiguousarray(rows, np.float32)
    if not misalign:
        return torch.from_numpy(rows.copy()).cuda()
    big = torch.zeros(rows.size + 8, dtype=torch.float32, device="cuda")
    v = big[1:1 + rows.size]
    v.copy_(torch.from_numpy(rows.copy()).reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


@pytest.fixture(scope="module")
def table(lib):
    """The gallery table's 257 rows and the 65 query rows on the device (each at a 16- and a 4-byte aligned address), the gallery
    packed at ld = 288, and both tables' ids."""
    g, q = G.tables()
    mat = torch.zeros((G.K, 288), dtype=torch.float32, device="cuda")
    n2 = torch.zeros((288,), dtype=torch.float32, device="cuda")
    rows = _dev(g)
    assert lib.trl_gallery_pack(_ptr(rows), 257, _ptr(mat), 288, _ptr(n2), 0, _stream()) == 0, lib.trl_last_error()
    return dict(g=(rows, _dev(g, True)), q=(_dev(q), _dev(q, True)), mat=mat, n2=n2, ld=288,
                gid=torch.from_numpy(H.gallery_ids()).cuda(), qid=torch.from_numpy(H.query_ids()).cuda())


def _mask_t(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.uint8)).cuda()


def _raw_hist(lib, t, q_t, qid_t, n, m, metric, pairs, edges, qvalid=None, gvalid=None, strip_cols=0, ws_delta=0, ws_offset=0, null=(),
              ld=None, nedges=None):
    """trl_gallery_hist into a prefilled buffer: (status, counts with a guard slot on either side (2 (E + 2) + 2,) int64)."""
    E = len(edges)
    e_t = torch.from_numpy(np.array(edges, np.float32)).cuda()
    counts = torch.full((2 * (E + 2) + 2,), FILL, dtype=torch.int64, device="cuda")
    nedges = E if nedges is None else nedges
    need = lib.trl_gallery_hist_workspace(n, m, nedges, strip_cols)
    size = max(need + ws_delta, 0)
    buf = torch.full((size + ws_offset + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    a = dict(q=q_t, qid=qid_t, mat=t["mat"], n2=t["n2"], gid=t["gid"], edges=e_t, counts=counts[1:])
    a.update({k: None for k in null})
    st = lib.trl_gallery_hist(_ptr(a["q"]), _ptr(_mask_t(qvalid)), _ptr(a["qid"]), n, _ptr(a["mat"]), t["ld"] if ld is None else ld,
                              _ptr(a["n2"]), _ptr(_mask_t(gvalid)), _ptr(a["gid"]), m, metric, pairs, _ptr(a["edges"]), nedges,
                              _ptr(a["counts"]), C_.c_void_p(buf.data_ptr() + ws_offset if size else 0), size, strip_cols, _stream())
    torch.cuda.synchronize()
    assert (buf[ws_offset + size:] == 0xA5).all(), "written behind the workspace"
    return st, counts.cpu().numpy()


def _check(lib, t, q_key, qid_key, n, m, metric, pairs, name, scores, qids, qmask, gmask):
    """One shape, metric, edge set and mask: default strips, 128-column strips and a misaligned d_q against the reference; then the
    same call with a workspace one byte short is refused and writes nothing."""
    edges = H.edge_set(name, metric)
    E = len(edges)
    want = H.hist_ref(scores, metric, edges, qids, H.gallery_ids()[:m], qmask, gmask, upper=pairs == UPPER)
    for strip_cols, mis in ((0, False), (128, False), (0, True)):
        st, c = _raw_hist(lib, t, t[q_key][mis], t[qid_key], n, m, metric, pairs, edges, qmask, gmask, strip_cols)
        assert st == 0, lib.trl_last_error()
        assert c[0] == FILL and c[-1] == FILL, "guard slot written"
        got = c[1:-1].reshape(2, E + 2)
        assert np.array_equal(got, want), (n, m, metric, pairs, name, qmask is not None, gmask is not None, strip_cols, mis,
                                           np.argwhere(got != want)[:4].tolist())
    st, c = _raw_hist(lib, t, t[q_key][0], t[qid_key], n, m, metric, pairs, edges, qmask, gmask, ws_delta=-1)
    assert st == TRL_ERR_INVALID and b"workspace" in lib.trl_last_error() and (c == FILL).all()
    return want


def _masks(n, m, square):
    qm, gm = CR.mask(n), CR.mask(m)
    return ((None, None), (qm, gm)) + (() if square and n < 32 else ((qm, None), (None, gm)))


@pytest.mark.parametrize("pairs", (UPPER, ALL))
@pytest.mark.parametrize("n", TABLE_N)
def test_table_against_itself(lib, table, n, pairs):
    other = H.PLAIN_SETS[TABLE_N.index(n) % len(H.PLAIN_SETS)]
    for metric in (G.COSINE, G.EUCLIDEAN):
        scores = CR.table_scores(metric)[:n, :n]
        for name in ("TIES", other):
            for qmask, gmask in _masks(n, n, True):
                want = _check(lib, table, "g", "gid", n, n, metric, pairs, name, scores, H.gallery_ids()[:n], qmask, gmask)
                if qmask is None and gmask is None:
                    assert want.sum() == (n * (n - 1) // 2 if pairs == UPPER else n * n)


@pytest.mark.parametrize("m", QUERY_M)
def test_queries_against_the_table(lib, table, m):
    other = H.PLAIN_SETS[(QUERY_M.index(m) + 3) % len(H.PLAIN_SETS)]
    n = G.N_TABLE
    for metric in (G.COSINE, G.EUCLIDEAN):
        scores = G.table_scores(metric)[:, :m]
        for name in ("TIES", other):
            for qmask, gmask in _masks(n, m, False):
                want = _check(lib, table, "q", "qid", n, m, metric, ALL, name, scores, H.query_ids(), qmask, gmask)
                if qmask is None and gmask is None:
                    assert want.sum() == n * m and (m < 3 or want[1].sum() > 0)


def test_fewer_query_rows_than_the_table_holds(lib, table):
    """n < 65 queries: the rows and ids behind n are not counted."""
    for n in (1, 33, 64):
        for metric in (G.COSINE, G.EUCLIDEAN):
            _check(lib, table, "q", "qid", n, 257, metric, ALL, "TIES", G.table_scores(metric)[:n], H.query_ids()[:n], None, None)


def test_nan_and_inf_scores(lib, table):
    """The table's NaN, inf and zero rows: NaN scores are counted in slot E + 1 of their class and nowhere else; +inf scores sit in
    the bins the reference puts them in."""
    for metric in (G.COSINE, G.EUCLIDEAN):
        s = CR.table_scores(metric)
        ids = H.gallery_ids()
        for name in ("INF", "TIES", "ONE"):
            E = len(H.edge_set(name, metric))
            for pairs in (UPPER, ALL):
                want = _check(lib, table, "g", "gid", 257, 257, metric, pairs, name, s, ids, None, None)
                keep = np.triu(np.ones_like(s, bool), 1) if pairs == UPPER else np.ones_like(s, bool)
                assert want[:, E + 1].sum() == (np.isnan(s) & keep).sum() > 200 and want[1, E + 1] > 0
    e = H.edge_set("INF", G.EUCLIDEAN)                        # (a +inf distance is not < the +inf edge: bin E - 1, and bin E stays empty)
    want = H.hist_ref(CR.table_scores(G.EUCLIDEAN), G.EUCLIDEAN, e, H.gallery_ids(), H.gallery_ids())
    assert want[:, len(e) - 1].sum() >= np.isinf(CR.table_scores(G.EUCLIDEAN)).sum() > 0 and want[:, len(e)].sum() == 0


def test_empty_problems_write_zero_counts(lib, table):
    edges = H.edge_set("E63", G.COSINE)
    for n, m, pairs, null in ((0, 257, ALL, ()), (65, 0, ALL, ()), (0, 0, UPPER, ()), (0, 0, ALL, ("q", "qid", "gid")), (0, 257, ALL, ("q", "qid")),
                              (65, 0, ALL, ("gid",))):
        assert lib.trl_gallery_hist_workspace(n, m, len(edges), 0) == 0
        st, c = _raw_hist(lib, table, table["q"][0], table["qid"], n, m, G.COSINE, pairs, edges, null=null)
        assert st == 0, lib.trl_last_error()
        assert c[0] == FILL and c[-1] == FILL and (c[1:-1] == 0).all()


def test_refusals(lib, table):
    edges = H.edge_set("E63", G.COSINE)

    def refused(null=(), **kw):
        a = dict(n=33, m=33, metric=0, pairs=UPPER, strip_cols=0, ws_delta=0, ws_offset=0, ld=None, nedges=None)
        a.update(kw)
        st, c = _raw_hist(lib, table, table["g"][0], table["gid"], a["n"], a["m"], a["metric"], a["pairs"], edges, None, None, a["strip_cols"],
                          a["ws_delta"], a["ws_offset"], null, a["ld"], a["nedges"])
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_hist"), (kw, null, st, lib.trl_last_error())
        assert (c == FILL).all(), (kw, null)

    for kw in (dict(nedges=0), dict(nedges=-1), dict(nedges=1024), dict(metric=2), dict(metric=-1), dict(pairs=2), dict(pairs=-1),
               dict(n=32), dict(m=65), dict(n=0), dict(m=0, pairs=UPPER), dict(ld=100), dict(ld=0), dict(ld=32, pairs=ALL), dict(ld=-32),
               dict(n=-1, pairs=ALL), dict(m=-1, pairs=ALL), dict(m=1 << 31, ld=1 << 31, pairs=ALL), dict(strip_cols=100), dict(strip_cols=-128),
               dict(ws_delta=-1), dict(ws_delta=-100), dict(ws_offset=4)):
        refused(**kw)
    for null in ("q", "qid", "mat", "n2", "gid", "edges", "counts"):
        refused(null=(null,))
    st, c = _raw_hist(lib, table, table["g"][0], table["gid"], 33, 33, 0, UPPER, edges)           # and the same call, unchanged, passes
    want = H.hist_ref(CR.table_scores(0)[:33, :33], 0, edges, H.gallery_ids()[:33], H.gallery_ids()[:33], upper=True)
    assert st == 0 and np.array_equal(c[1:-1].reshape(2, -1), want)
    st, c = _raw_hist(lib, table, table["g"][0], table["gid"], 33, 33, 0, UPPER, edges, ws_delta=64)  # a larger workspace is fine
    assert st == 0 and np.array_equal(c[1:-1].reshape(2, -1), want)


def test_counts_agree_with_the_clustering(lib, table):
    """Links are accepted pairs: at an edge equal to a clustering threshold, sum(degree[valid] - 1) of trl_cluster_links is twice the
    accepted pairs, genuine and impostor, of the upper histogram."""
    rows = table["g"][0]
    for metric in (G.COSINE, G.EUCLIDEAN):
        edges = H.with_thresholds(metric)
        E = len(edges)
        for n in (65, 257):
            for invalid in ((), CR.INVALID):
                valid = CR.mask(n, invalid) if invalid else None
                st, c = _raw_hist(lib, table, rows, table["gid"], n, n, metric, UPPER, edges, valid, valid)
                assert st == 0, lib.trl_last_error()
                both = c[1:-1].reshape(2, E + 2).sum(axis=0)
                for thr in CR.TABLE_THR[metric]:
                    e = int(np.nonzero(edges == np.float32(thr))[0][0])
                    accepted = both[e + 1:E + 1].sum() if metric == G.COSINE else both[:e + 1].sum()
                    words = (n + 31) // 32
                    adj = torch.empty((n, words), dtype=torch.int32, device="cuda")
                    deg = torch.empty((n,), dtype=torch.int32, device="cuda")
                    st = lib.trl_cluster_links(_ptr(rows), _ptr(_mask_t(valid)), n, _ptr(table["mat"]), table["ld"], _ptr(table["n2"]), metric,
                                               float(np.float32(thr)), _ptr(adj), words, _ptr(deg), 0, _stream())
                    assert st == 0, lib.trl_last_error()
                    d = deg.cpu().numpy()
                    assert (d[d > 0] - 1).sum() == 2 * accepted > 0, (metric, n, invalid, thr)


# ---- FaceGallery.score_histogram / roc / calibrate -------------------------------------------------------------------------------
def _ref_dict(scores, metric, edges, qids, gids, qv=None, gv=None, upper=False):
    c = H.hist_ref(scores, metric, edges, qids, gids, qv, gv, upper)
    E = len(edges)
    return c[1, :E + 1], c[0, :E + 1], c[:, E + 1]


def _same(h, ref, edges):
    assert all(h[k].device.type == "cuda" for k in ("edges", "genuine", "impostor", "nan"))
    assert h["genuine"].dtype == h["impostor"].dtype == h["nan"].dtype == torch.int64 and h["edges"].dtype == torch.float32
    E = len(edges)
    assert h["edges"].shape == (E,) and h["genuine"].shape == h["impostor"].shape == (E + 1,) and h["nan"].shape == (2,)
    assert np.array_equal(h["edges"].cpu().numpy(), edges)
    for k, want in zip(("genuine", "impostor", "nan"), ref):
        assert np.array_equal(h[k].cpu().numpy(), want), k


def test_face_gallery_histogram_roc_calibrate(lib):
    from truely_amd.gallery import FaceGallery, roc_from_counts, threshold_at_far
    g, q = G.tables()
    gids, qids = H.gallery_ids(), H.query_ids()
    glabels, qlabels = [f"person-{i}" for i in gids], [f"person-{i}" for i in qids]
    qlabels[5] = "a stranger"                                   # a label the gallery does not hold: impostor to every row
    qids = qids.copy(); qids[5] = 1000
    for name, metric in G.METRICS.items():
        gal = FaceGallery(metric=name, capacity=32)
        empty = gal.score_histogram(edges=[0.5])
        assert int(empty["genuine"].sum()) == int(empty["impostor"].sum()) == int(empty["nan"].sum()) == 0
        gal.add(g[:20], glabels[:20])
        gal.add(g[20:], glabels[20:])
        s_self, s_q = CR.table_scores(metric), G.table_scores(metric)
        default = (np.linspace(-1, 1, 1001) if metric == G.COSINE else np.linspace(0, 2, 1001)).astype(np.float32)
        ties = H.edge_set("TIES", metric)
        valid, qvalid = CR.mask(257), CR.mask(65)
        _same(gal.score_histogram(), _ref_dict(s_self, metric, default, gids, gids, upper=True), default)
        _same(gal.score_histogram(edges=ties, max_strip_cols=128), _ref_dict(s_self, metric, ties, gids, gids, upper=True), ties)
        for kw in (dict(valid=valid), dict(gallery_valid=torch.from_numpy(valid))):
            _same(gal.score_histogram(edges=ties, **kw), _ref_dict(s_self, metric, ties, gids, gids, valid, valid, True), ties)
        _same(gal.score_histogram(q, qlabels, edges=ties), _ref_dict(s_q, metric, ties, qids, gids), ties)
        _same(gal.score_histogram(torch.from_numpy(q.copy()).cuda(), qlabels, torch.from_numpy(ties), valid=qvalid, gallery_valid=valid),
              _ref_dict(s_q, metric, ties, qids, gids, qvalid, valid), ties)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            h = gal.score_histogram(q, qlabels, edges=ties)
            side.synchronize()
        _same(h, _ref_dict(s_q, metric, ties, qids, gids), ties)
        # rates and the threshold: the reference's loops on the reference's counts
        edges = H.edge_set("E1023", metric)
        gen, imp, nan = _ref_dict(s_q, metric, edges, qids, gids)
        want_t, want_f = H.roc_ref(gen, imp, nan, metric)
        r = gal.roc(q, qlabels, edges=edges)
        assert np.array_equal(r["edges"], edges) and np.array_equal(r["tar"], np.array(want_t)) and np.array_equal(r["far"], np.array(want_f))
        assert r["tar"].dtype == np.float64 and not np.isnan(r["far"]).any()
        looser = -1 if metric == G.COSINE else 1
        hit = 0
        for target in (0.5, 0.05, 1e-3, 0.0):
            want = H.threshold_ref(edges, want_t, want_f, target, metric)
            if want is None:
                with pytest.raises(ValueError):
                    gal.calibrate(target, q, qlabels, edges=edges)
                continue
            cal = gal.calibrate(target, q, qlabels, edges=edges)
            assert (cal["threshold"], cal["tar"], cal["far"]) == want and cal["far"] <= target
            e = int(np.nonzero(edges == np.float32(cal["threshold"]))[0][0])          # the threshold IS an edge
            assert float(edges[e]) == cal["threshold"]
            if 0 <= e + looser < len(edges):
                assert want_f[e + looser] > target
                hit += 1
            # identify at that threshold accepts a query exactly when the counts of its row alone hold an accepted pair
            who, _score = gal.identify(q, threshold=cal["threshold"])
            for i in range(0, G.N_TABLE, 4):
                h = gal.score_histogram(q[i:i + 1], qlabels[i:i + 1], edges=edges)
                both = (h["genuine"] + h["impostor"]).cpu().numpy()
                accepted = both[e + 1:].sum() if metric == G.COSINE else both[:e + 1].sum()
                assert (who[i] is not None) == (accepted > 0), (name, target, i)
                with np.errstate(invalid="ignore"):
                    want_row = (s_q[i] >= edges[e]).sum() if metric == G.COSINE else (s_q[i] <= edges[e]).sum()
                assert accepted == want_row
            assert any(w is not None for w in who) and any(w is None for w in who)
        assert hit >= 2
        assert inspect.signature(gal.calibrate).parameters["far"].default == 1e-3
        # what gallery.py itself refuses
        for kw in (dict(edges=[0.5, 0.5]), dict(edges=[0.5, 0.25]), dict(edges=[0.1, float("nan")]), dict(edges=[]),
                   dict(edges=np.linspace(0, 1, 1024)), dict(labels=qlabels), dict(valid=valid, gallery_valid=valid),
                   dict(emb=q), dict(emb=q, labels=qlabels[:3]), dict(emb=q, labels=qlabels, valid=valid),
                   dict(emb=q, labels=qlabels, gallery_valid=qvalid), dict(valid=qvalid)):
            with pytest.raises(ValueError):
                gal.score_histogram(**kw)
        with pytest.raises(_lib.TrlError, match="trl_gallery_hist"):
            gal.score_histogram(max_strip_cols=100)
    assert truely_amd.roc_from_counts is roc_from_counts and truely_amd.threshold_at_far is threshold_at_far
