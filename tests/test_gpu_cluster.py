"""The embedding clustering on the device (trl_cluster_links in csrc/trl_gallery.hip, trl_cluster_labels in csrc/trl_cluster.hip) against
tests/cluster_ref.py, exactly: bitmap words, degrees, labels, core flags and the cluster count; the refusals; gallery.py on top.

k_gallery_links tiles rows by 32 and columns by 32 per wave / 128 per workgroup and walks strips of 128-column groups, so the
table's first n rows are taken at n in {1, 2, 31, 32, 33, 64, 65, 129, 257} (a lone row, a tile short of / equal to / past 32, two
tiles and one row more, a group and one column more, three groups with a lone column in the third), once with the default strips
and once with strips of 128 columns.  Every output lies in a prefilled buffer with a guard row on either side, the bitmap with
two guard words per row too."""
import ctypes as C_
import os

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
import cluster_ref as CR
import gallery_ref as G

pytestmark = pytest.mark.gpu

TABLE_N = (1, 2, 31, 32, 33, 64, 65, 129, 257)
FILL_WORD, FILL_DEG, FILL_LABEL, FILL_CORE, FILL_COUNT = 0xA5A5A5A5, -77, -7, 9, -5
TRL_ERR_INVALID = -1
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    """The gallery table's 257 rows on the device, row-major at a 16- and at a 4-byte aligned address, and packed (ld = 288).  A
    call with n < 257 sees other rows, not zeros, behind its own."""
    g, _q = G.tables()
    rows, rows_mis = _dev(g), _dev(g, misalign=True)
    mat = torch.zeros((G.K, 288), dtype=torch.float32, device="cuda")
    n2 = torch.zeros((288,), dtype=torch.float32, device="cuda")
    assert lib.trl_gallery_pack(_ptr(rows), 257, _ptr(mat), 288, _ptr(n2), 0, _stream()) == 0, lib.trl_last_error()
    return rows, rows_mis, mat, n2, 288


def _raw_links(lib, q_t, valid, n, mat, ld, n2, metric, thr, strip_cols=0, pitch=None, null=()):
    """trl_cluster_links into prefilled buffers: (status, bitmap (n + 2, pitch) uint32, degree (n + 2,) int32), guards included."""
    words = (max(n, 0) + 31) // 32
    pitch = words + 2 if pitch is None else pitch
    rows = min(max(n, 1), 300) + 2                       # (a call with n past the table is one that must be refused)
    adj = torch.full((rows, max(pitch, 1)), FILL_WORD - (1 << 32), dtype=torch.int32, device="cuda")
    deg = torch.full((rows,), FILL_DEG, dtype=torch.int32, device="cuda")
    v_t = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8)).cuda()
    st = lib.trl_cluster_links(_ptr(None if "q" in null else q_t), _ptr(v_t), n, _ptr(None if "mat" in null else mat), ld,
                               _ptr(None if "n2" in null else n2), metric, thr, _ptr(None if "adj" in null else adj[1]), pitch,
                               _ptr(None if "degree" in null else deg[1:]), strip_cols, _stream())
    torch.cuda.synchronize()
    return st, adj.cpu().numpy().view(np.uint32), deg.cpu().numpy()


def _raw_labels(lib, adj: np.ndarray, deg: np.ndarray, n, min_samples, pitch=None, ws_delta=0, ws_offset=0, null=(), rounds=True):
    """trl_cluster_labels on a host bitmap (n, pitch) and degrees: (status, labels (n + 2,), core (n + 2,), count (3,), rounds)."""
    pitch = adj.shape[1] if pitch is None else pitch
    adj_t = torch.from_numpy(np.ascontiguousarray(adj).view(np.int32).copy()).cuda()
    deg_t = torch.from_numpy(np.ascontiguousarray(deg, np.int32).copy()).cuda()
    labels = torch.full((max(n, 1) + 2,), FILL_LABEL, dtype=torch.int32, device="cuda")
    core = torch.full((max(n, 1) + 2,), FILL_CORE, dtype=torch.uint8, device="cuda")
    count = torch.full((3,), FILL_COUNT, dtype=torch.int32, device="cuda")
    need = lib.trl_cluster_workspace(n)
    size = max(need + ws_delta, 0)
    ws = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")[ws_offset:ws_offset + size] if size else None
    r = C_.c_int(-1)
    st = lib.trl_cluster_labels(_ptr(None if "adj" in null else adj_t), pitch, _ptr(None if "degree" in null else deg_t), n, min_samples,
                                _ptr(None if "labels" in null else labels[1:]), _ptr(None if "core" in null else core[1:]),
                                _ptr(None if "count" in null else count[1:]), _ptr(ws), size, C_.byref(r) if rounds else None, _stream())
    torch.cuda.synchronize()
    return st, labels.cpu().numpy(), core.cpu().numpy(), count.cpu().numpy(), r.value


def _check_labels(lib, link, deg, min_samples, pitch_extra=0):
    n = len(deg)
    want_l, want_c, want_n = CR.labels_ref(link, deg, min_samples)
    adj = CR.pack_bitmap(link, (n + 31) // 32 + pitch_extra)
    st, labels, core, count, rounds = _raw_labels(lib, adj, deg, n, min_samples)
    assert st == 0, lib.trl_last_error()
    assert labels[0] == FILL_LABEL and labels[-1] == FILL_LABEL and core[0] == FILL_CORE and core[-1] == FILL_CORE, "guard written"
    assert count[0] == FILL_COUNT and count[2] == FILL_COUNT
    assert np.array_equal(labels[1:-1], want_l), (n, min_samples, np.nonzero(labels[1:-1] != want_l)[0][:5].tolist())
    assert np.array_equal(core[1:-1], want_c) and count[1] == want_n, (n, min_samples, int(count[1]), want_n)
    assert 1 <= rounds <= n + 4
    return rounds, want_n


# ---- links -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TABLE_N)
def test_links_and_labels_on_the_table(lib, table, n):
    """Bitmap words and degrees of the table's first n rows against the reference, bit for bit: both metrics, two thresholds each,
    default and 128-column strips, with and without a valid mask that kills rows on both sides of the 32-row tile edge, d_q at a
    16- and a 4-byte aligned address.  Then the labels of each of those bitmaps, as the device wrote it, at five min_samples."""
    rows, rows_mis, mat, n2, ld = table
    words = (n + 31) // 32
    for metric in (G.COSINE, G.EUCLIDEAN):
        for thr in CR.TABLE_THR[metric]:
            for invalid in ((), CR.INVALID):
                valid = CR.mask(n, invalid) if invalid else None
                link, deg = CR.table_links(metric, thr, n, invalid)
                want = CR.pack_bitmap(link)
                got = None
                for strip_cols, q_t in ((0, rows), (128, rows), (0, rows_mis)):
                    st, adj, dg = _raw_links(lib, q_t, valid, n, mat, ld, n2, metric, thr, strip_cols)
                    assert st == 0, lib.trl_last_error()
                    assert (adj[[0, -1]] == FILL_WORD).all() and (adj[:, words:] == FILL_WORD).all(), "guard row or guard word written"
                    assert dg[0] == FILL_DEG and dg[-1] == FILL_DEG
                    bad = np.argwhere(adj[1:-1, :words] != want)
                    assert not len(bad), (n, metric, thr, invalid, strip_cols, bad[:3].tolist())
                    assert np.array_equal(dg[1:-1], deg), (n, metric, thr, invalid, strip_cols)
                    got = adj[1:-1]
                for ms in CR.MIN_SAMPLES:
                    want_l, want_c, want_n = CR.labels_ref(link, deg, ms)
                    st, labels, core, count, rounds = _raw_labels(lib, got, deg, n, ms)          # (pitch = words + 2, guards and all)
                    assert st == 0, lib.trl_last_error()
                    assert np.array_equal(labels[1:-1], want_l) and np.array_equal(core[1:-1], want_c) and count[1] == want_n, \
                        (n, metric, thr, invalid, ms)
                    assert labels[0] == FILL_LABEL and labels[-1] == FILL_LABEL and core[0] == FILL_CORE and core[-1] == FILL_CORE


# ---- labels on hand-made bitmaps -------------------------------------------------------------------------------------------------
def test_labels_on_hand_made_graphs(lib):
    for ms in (1, 2):
        _check_labels(lib, *CR.empty_graph(70), ms)
        _check_labels(lib, *CR.empty_graph(1), ms)
    link, deg = CR.clique(33)
    for ms in (1, 33, 34):
        _check_labels(lib, link, deg, ms, pitch_extra=1)
    link, deg = CR.star(40, 17)                            # the centre is the only core row; 39 border rows
    _r, count = _check_labels(lib, link, deg, 40)
    assert count == 1
    link, deg = CR.two_cliques_and_bridge()                # the border row must take the lower number
    _r, count = _check_labels(lib, link, deg, 4)
    assert count == 2
    link, deg = CR.pendant_of_border()                     # a row whose only neighbour is not core: noise
    _check_labels(lib, link, deg, 4)
    link, deg = CR.empty_graph(40)                         # invalid rows (degree 0) between valid ones
    deg = deg.copy(); deg[[0, 31, 32, 39]] = 0
    _check_labels(lib, link, deg, 1)
    # two components that interleave across word and tile edges, one row apart
    n = 131
    even, odd = list(range(0, n, 2)), list(range(1, n, 2))
    link, deg = CR.graph(n, list(zip(even[:-1], even[1:])) + list(zip(odd[:-1], odd[1:])))
    _r, count = _check_labels(lib, link, deg, 1)
    assert count == 2


@pytest.mark.parametrize("order", ("ascending", "descending", "bit_reversed"))
def test_labels_on_a_long_path(lib, order):
    """A path of 4,096 rows: the component's label has to travel the whole path.  Correctness is the test; the rounds are printed
    (DESIGN.md records them)."""
    idx = {"ascending": np.arange(4096), "descending": np.arange(4096)[::-1], "bit_reversed": CR.bit_reverse(12)}[order]
    link, deg = CR.path(idx)
    rounds, count = _check_labels(lib, link, deg, 1)
    print(f"path of 4096, {order}: rounds = {rounds}")
    assert count == 1
    _r, count = _check_labels(lib, link, deg, 3)           # the two ends (degree 2) are border rows
    assert count == 1


# ---- end to end on analytic inputs -----------------------------------------------------------------------------------------------
def test_cluster_embeddings_on_a_line():
    """Rows p_i * e_0, p a permutation of 0..299, euclidean, thr 1.5: every product and sum is an exact small integer, so the
    links are |p_i - p_j| = 1: one cluster; at min_samples = 3 the two ends are border rows."""
    from truely_amd.gallery import cluster_embeddings
    assert truely_amd.cluster_embeddings is cluster_embeddings
    p = np.random.default_rng(300).permutation(300)
    emb = np.zeros((300, G.K), np.float32)
    emb[:, 0] = p
    info = cluster_embeddings(torch.from_numpy(emb).cuda(), 1.5, metric="euclidean", return_info=True)
    assert info["labels"].dtype == torch.int32 and info["labels"].device.type == "cuda" and info["labels"].shape == (300,)
    assert info["n_clusters"] == 1 and (info["labels"].cpu().numpy() == 0).all() and info["core"].cpu().numpy().all()
    assert np.array_equal(info["degree"].cpu().numpy(), np.where((p == 0) | (p == 299), 2, 3))
    print("line of 300: rounds =", info["rounds"])
    info = cluster_embeddings(emb, 1.5, metric="euclidean", min_samples=3, return_info=True, device="cuda")      # a host array
    ends = (p == 0) | (p == 299)
    assert info["n_clusters"] == 1 and (info["labels"].cpu().numpy() == 0).all()
    assert np.array_equal(info["core"].cpu().numpy(), (~ends).astype(np.uint8))
    labels = cluster_embeddings(torch.from_numpy(emb).cuda(), 0.5, metric="euclidean")      # nothing links: 300 clusters in row order
    assert np.array_equal(labels.cpu().numpy(), np.arange(300))


def test_cluster_embeddings_one_hot():
    """n = 2,080 one-hot rows e_(i mod 512), cosine thr 0.5, min_samples 5: residues below 32 have five members (cosine 1), all
    others four.  32 clusters numbered by residue, all else -1.  The rows span 65 row tiles and 17 column groups."""
    from truely_amd.gallery import cluster_embeddings
    n = 2080
    emb = np.zeros((n, G.K), np.float32)
    emb[np.arange(n), np.arange(n) % 512] = 1
    want = np.where(np.arange(n) % 512 < 32, np.arange(n) % 512, -1).astype(np.int32)
    info = cluster_embeddings(torch.from_numpy(emb).cuda(), 0.5, metric="cosine", min_samples=5, return_info=True)
    assert np.array_equal(info["labels"].cpu().numpy(), want) and info["n_clusters"] == 32
    assert np.array_equal(info["degree"].cpu().numpy(), np.where(np.arange(n) % 512 < 32, 5, 4))
    assert np.array_equal(info["core"].cpu().numpy(), (want >= 0).astype(np.uint8))
    valid = np.ones(n, np.uint8); valid[512 + 3] = 0                     # residue 3 loses a member: its four rows become noise
    labels = cluster_embeddings(torch.from_numpy(emb).cuda(), 0.5, min_samples=5, valid=valid).cpu().numpy()
    want_v = np.where(np.arange(n) % 512 == 3, -1, np.where(want > 3, want - 1, want))
    assert np.array_equal(labels, want_v)


# ---- FaceGallery.cluster ---------------------------------------------------------------------------------------------------------
def test_face_gallery_cluster(lib):
    from truely_amd.gallery import FaceGallery
    g, _q = G.tables()
    for name, metric in G.METRICS.items():
        thr = CR.TABLE_THR[metric][0]
        gal = FaceGallery(metric=name, capacity=32)
        empty = gal.cluster(thr, return_info=True)
        assert empty["labels"].shape == (0,) and empty["n_clusters"] == 0
        gal.add(g[:20], range(20))
        gal.add(g[20:257], range(20, 257))                 # growth past the capacity
        assert gal.ld >= 257
        for ms, invalid in ((1, ()), (3, ()), (6, (40, 41, 200))):
            link, deg = CR.table_links(metric, thr, 257, invalid)
            want_l, want_c, want_n = CR.labels_ref(link, deg, ms)
            valid = CR.mask(257, invalid) if invalid else None
            info = gal.cluster(thr, min_samples=ms, valid=valid, return_info=True)
            assert np.array_equal(info["labels"].cpu().numpy(), want_l) and np.array_equal(info["core"].cpu().numpy(), want_c)
            assert np.array_equal(info["degree"].cpu().numpy(), deg) and info["n_clusters"] == want_n and info["rounds"] >= 1
            labels = gal.cluster(thr, min_samples=ms, valid=valid)                         # a repeat call: equal bits
            assert labels.dtype == torch.int32 and labels.device.type == "cuda" and torch.equal(labels, info["labels"])
            assert torch.equal(gal.cluster(thr, min_samples=ms, valid=valid, max_strip_cols=128), labels)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            labels = gal.cluster(thr, min_samples=3)
            side.synchronize()
        assert np.array_equal(labels.cpu().numpy(), CR.labels_ref(*CR.table_links(metric, thr), 3)[0])
        for kw in (dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=-float("inf")), dict(min_samples=0),
                   dict(min_samples=-3), dict(max_strip_cols=100), dict(max_strip_cols=-128)):
            a = dict(threshold=thr)
            a.update(kw)
            with pytest.raises(_lib.TrlError, match="trl_cluster_"):
                gal.cluster(**a)
        with pytest.raises(ValueError):
            gal.cluster(thr, valid=np.ones(5, np.uint8))
    with pytest.raises(ValueError):
        truely_amd.cluster_embeddings(g[:4], 0.5, metric="manhattan", device="cuda")


def test_refusals(lib, table):
    rows, _mis, mat, n2, ld = table

    def refused_links(null=(), **kw):
        a = dict(n=33, ld=ld, metric=0, thr=0.12, strip_cols=0, pitch=None)
        a.update(kw)
        st, adj, deg = _raw_links(lib, rows, None, a["n"], mat, a["ld"], n2, a["metric"], a["thr"], a["strip_cols"], a["pitch"], null)
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_cluster_links"), (kw, null, st, lib.trl_last_error())
        assert (adj == FILL_WORD).all() and (deg == FILL_DEG).all(), (kw, null)

    for kw in (dict(n=-1), dict(n=65537, ld=65568, pitch=2049), dict(pitch=1), dict(n=65, pitch=2), dict(thr=float("nan")), dict(thr=float("inf")),
               dict(thr=-float("inf")), dict(metric=2), dict(metric=-1), dict(strip_cols=100), dict(strip_cols=-128), dict(ld=100),
               dict(ld=0), dict(ld=32)):
        refused_links(**kw)
    for null in ("q", "mat", "n2", "adj", "degree"):
        refused_links(null=(null,))
    st, adj, deg = _raw_links(lib, rows, None, 33, mat, ld, n2, 0, 0.12, pitch=2)          # and the same call at the least pitch passes
    assert st == 0 and np.array_equal(adj[1:-1], CR.pack_bitmap(CR.table_links(0, 0.12, 33)[0]))
    st, adj, deg = _raw_links(lib, rows, None, 0, mat, ld, n2, 0, 0.12)                     # n = 0: nothing is done
    assert st == 0 and (adj == FILL_WORD).all() and (deg == FILL_DEG).all()

    link, dg = CR.table_links(0, 0.12, 33)
    bitmap = CR.pack_bitmap(link)
    need = lib.trl_cluster_workspace(33)
    assert need >= 3 * 33 * 4

    def refused_labels(null=(), **kw):
        a = dict(n=33, min_samples=2, pitch=None, ws_delta=0, ws_offset=0)
        a.update(kw)
        st, labels, core, count, _r = _raw_labels(lib, bitmap, dg, a["n"], a["min_samples"], a["pitch"], a["ws_delta"], a["ws_offset"], null)
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_cluster_labels"), (kw, null, st, lib.trl_last_error())
        assert (labels == FILL_LABEL).all() and (core == FILL_CORE).all() and (count == FILL_COUNT).all(), (kw, null)

    for kw in (dict(ws_delta=-1), dict(ws_offset=4), dict(n=-1), dict(n=65537, pitch=2049), dict(pitch=1), dict(min_samples=0),
               dict(min_samples=-1)):
        refused_labels(**kw)
    for null in ("adj", "degree", "labels", "core", "count"):
        refused_labels(null=(null,))
    st, labels, core, count, r = _raw_labels(lib, bitmap, dg, 33, 2, rounds=False)         # a null rounds_out is fine
    assert st == 0 and np.array_equal(labels[1:-1], CR.labels_ref(link, dg, 2)[0])
    st, labels, core, count, r = _raw_labels(lib, bitmap, dg, 0, 2)                        # n = 0: the count is 0, nothing else
    assert st == 0 and (labels == FILL_LABEL).all() and (core == FILL_CORE).all() and count.tolist() == [FILL_COUNT, 0, FILL_COUNT] and r == 0


# ---- detect -> extract (keep_all) -> embed -> cluster ----------------------------------------------------------------------------
def test_cluster_end_to_end(engine):
    """Every face of the multi-face 270p clip, its frames given twice: a face and its copy in the second half share a label at
    cosine 0.999, and the labels are the reference's on the embeddings the device computed."""
    from truely_amd.gallery import cluster_embeddings
    from truely_amd.inception_resnet_v1 import InceptionResnetV1
    z = np.load(os.path.join(GOLD, "clip_multiface_270p.npz"))
    fr = truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))
    fr = np.concatenate([fr, fr])
    boxes, _p, counts = (t.cpu().numpy() for t in engine.mtcnn_detect(fr))
    half = len(fr) // 2
    assert counts[:half].sum() >= 4 and np.array_equal(counts[:half], counts[half:]), counts.tolist()
    rows = np.repeat(np.arange(len(fr)), counts).astype(np.int32)
    bx = np.concatenate([boxes[f, :counts[f]] for f in range(len(fr))]).astype(np.float32)
    faces, status = engine.extract_boxes(fr, torch.from_numpy(rows), torch.from_numpy(bx), 160, 0, "torch", True)
    assert (status.cpu().numpy() == 1).all()
    emb = InceptionResnetV1(engine=engine)(faces.to(engine.device))
    m = len(rows) // 2
    info = cluster_embeddings(emb, 0.999, metric="cosine", return_info=True)
    labels = info["labels"].cpu().numpy()
    print("faces", 2 * m, "clusters", info["n_clusters"], "rounds", info["rounds"], "labels", labels.tolist())
    assert (labels >= 0).all() and np.array_equal(labels[:m], labels[m:])
    e = emb.cpu().numpy()
    link = CR.links_ref(G.scores_ref(e, e, G.COSINE), G.COSINE, 0.999)
    want_l, want_c, want_n = CR.labels_ref(link, CR.degree_ref(link), 1)
    assert np.array_equal(labels, want_l) and info["n_clusters"] == want_n and np.array_equal(info["core"].cpu().numpy(), want_c)
    # and DBSCAN proper on the same embeddings: a face seen twice is a core row at min_samples = 2
    info2 = cluster_embeddings(emb, 0.999, metric="cosine", min_samples=2, return_info=True)
    want_l, want_c, want_n = CR.labels_ref(link, CR.degree_ref(link), 2)
    assert np.array_equal(info2["labels"].cpu().numpy(), want_l) and info2["core"].cpu().numpy().all()
