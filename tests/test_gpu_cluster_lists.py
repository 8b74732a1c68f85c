"""The label stage over neighbour lists on the device (trl_cluster_labels_lists, csrc/trl_cluster.hip) against tests/cluster_ref.py,
exactly: degrees, labels, core flags and the cluster count, with each lanes_per_row; the refusals; FaceGallery.cluster(method=...)
on top, where the range search writes the lists, and past the bitmap's 65,536 rows.

A row's list is walked by L = 4 / 16 / 64 lanes, so a list can be shorter than L, exactly L or take several passes.  The table's
lists (cosine 0.12: 0 .. 137 entries, mean 2; euclidean 31: up to 253, mean 130) are shorter, longer and no multiple of L for every
L; cliques of L + 1 rows give the lists of exactly L entries.  Every output lies in a prefilled buffer with a guard element on
either side."""
import ctypes as C_

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
import cluster_lists_ref as LR
import cluster_ref as CR
import gallery_ref as G

pytestmark = pytest.mark.gpu

TABLE_N = (1, 2, 31, 32, 33, 64, 65, 129, 257)
LANES = (0, 4, 16, 64)
FILL_DEG, FILL_LABEL, FILL_CORE, FILL_COUNT = -77, -7, 9, -5
TRL_ERR_INVALID = -1
MAX_LIST_N = 1 << 24
WS_LEAD = 4096                            # bytes of the test's own zeros in front of (and behind) a workspace placed "inside"


def _ptr(t):
    return C_.c_void_p(t.data_ptr() if t is not None else 0)


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _raw(lib, offsets, index, valid, n, min_samples, lanes, ws_delta=0, ws_offset=0, ws_inside=False, null=(), rounds=True):
    """trl_cluster_labels_lists on host lists: (status, degree (n + 2,), labels (n + 2,), core (n + 2,), count (3,), rounds), guards
    included.  ws_inside: the workspace lies WS_LEAD bytes inside a zeroed tensor of the test's."""
    off_t = torch.from_numpy(np.ascontiguousarray(offsets, np.int64).copy()).cuda()
    idx = np.ascontiguousarray(index, np.int32)
    idx_t = torch.from_numpy(idx.copy() if len(idx) else np.zeros(1, np.int32)).cuda()      # (an empty tensor has no address)
    v_t = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid, np.uint8).copy()).cuda()
    rows = min(max(n, 1), 1 << 20) + 2                   # (a call with n past that is one that must be refused)
    degree = torch.full((rows,), FILL_DEG, dtype=torch.int32, device="cuda")
    labels = torch.full((rows,), FILL_LABEL, dtype=torch.int32, device="cuda")
    core = torch.full((rows,), FILL_CORE, dtype=torch.uint8, device="cuda")
    count = torch.full((3,), FILL_COUNT, dtype=torch.int32, device="cuda")
    need = lib.trl_cluster_lists_workspace(n)
    size = max(need + ws_delta, 0)
    if ws_inside:
        big = torch.zeros((size + 2 * WS_LEAD,), dtype=torch.uint8, device="cuda")
        ws = big[WS_LEAD:WS_LEAD + size]
    else:
        ws = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")[ws_offset:ws_offset + size] if size else None
    r = C_.c_int(-1)
    st = lib.trl_cluster_labels_lists(_ptr(None if "offsets" in null else off_t), _ptr(None if "index" in null else idx_t), _ptr(v_t), n,
                                      min_samples, lanes, _ptr(None if "degree" in null else degree[1:]),
                                      _ptr(None if "labels" in null else labels[1:]), _ptr(None if "core" in null else core[1:]),
                                      _ptr(None if "count" in null else count[1:]), _ptr(ws), size, C_.byref(r) if rounds else None, _stream())
    torch.cuda.synchronize()
    return st, degree.cpu().numpy(), labels.cpu().numpy(), core.cpu().numpy(), count.cpu().numpy(), r.value


def _check(lib, link, deg, min_samples, lanes, want=None, lists=None, want_deg=None, **kw):
    """The call on the lists of `link` (or on `lists`), with the validity mask that `deg` implies, against labels_ref (or `want`)."""
    n = len(deg)
    want_l, want_c, want_n = CR.labels_ref(link, deg, min_samples) if want is None else want
    offsets, index = LR.csr_from_link(link) if lists is None else lists
    valid = None if (deg > 0).all() else (deg > 0).astype(np.uint8)
    st, degree, labels, core, count, rounds = _raw(lib, offsets, index, valid, n, min_samples, lanes, **kw)
    assert st == 0, lib.trl_last_error()
    assert degree[0] == FILL_DEG and degree[-1] == FILL_DEG and labels[0] == FILL_LABEL and labels[-1] == FILL_LABEL, "guard written"
    assert core[0] == FILL_CORE and core[-1] == FILL_CORE and count[0] == FILL_COUNT and count[2] == FILL_COUNT, "guard written"
    assert np.array_equal(degree[1:-1], deg if want_deg is None else want_deg), (n, min_samples, lanes)
    assert np.array_equal(labels[1:-1], want_l), (n, min_samples, lanes, np.nonzero(labels[1:-1] != want_l)[0][:5].tolist())
    assert np.array_equal(core[1:-1], want_c) and count[1] == want_n, (n, min_samples, lanes, int(count[1]), want_n)
    assert 1 <= rounds <= n + 4
    return rounds, want_n


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------
def test_table_lists_straddle_every_group_size():
    lengths = np.diff(LR.csr_from_link(CR.table_links(G.COSINE, 0.12)[0])[0])
    for L in (4, 16, 64):
        assert (lengths < L).any() and (lengths > L).any() and ((lengths > 0) & (lengths % L != 0)).any(), L
        assert (np.diff(LR.csr_from_link(CR.clique(L + 1)[0])[0]) == L).all()


@pytest.mark.parametrize("n", TABLE_N)
def test_labels_on_the_table(lib, n):
    """The lists of the table's first n rows: both metrics, two thresholds each, with and without invalid rows, five min_samples,
    every lanes_per_row.  Degrees, labels, core flags and the count equal the reference exactly."""
    for metric in (G.COSINE, G.EUCLIDEAN):
        for thr in CR.TABLE_THR[metric]:
            for invalid in ((), CR.INVALID):
                link, deg = CR.table_links(metric, thr, n, invalid)
                lists = LR.csr_from_link(link)
                for ms in CR.MIN_SAMPLES:
                    want = CR.labels_ref(link, deg, ms)
                    for lanes in LANES:
                        _check(lib, link, deg, ms, lanes, want=want, lists=lists)


# ---- 2. hand-made graphs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_labels_on_hand_made_graphs(lib, lanes):
    for ms in (1, 2):
        _check(lib, *CR.empty_graph(70), ms, lanes)
        _check(lib, *CR.empty_graph(1), ms, lanes)
    link, deg = CR.clique(33)
    for ms in (1, 33, 34):
        _check(lib, link, deg, ms, lanes)
    for size in (5, 17, 65):                               # lists of exactly 4, 16 and 64 entries
        link, deg = CR.clique(size)
        for ms in (size, size + 1):
            _check(lib, link, deg, ms, lanes)
    link, deg = CR.star(40, 17)                            # the centre is the only core row; 39 border rows
    _r, count = _check(lib, link, deg, 40, lanes)
    assert count == 1
    link, deg = CR.two_cliques_and_bridge()                # the border row must take the lower number
    _r, count = _check(lib, link, deg, 4, lanes)
    assert count == 2
    link, deg = CR.pendant_of_border()                     # a row whose only neighbour is not core: noise
    _check(lib, link, deg, 4, lanes)
    link, deg = CR.empty_graph(40)                         # invalid rows (d_valid = 0) between valid ones
    deg = deg.copy(); deg[[0, 31, 32, 39]] = 0
    _check(lib, link, deg, 1, lanes)
    n = 131                                                # two components that interleave, one row apart
    even, odd = list(range(0, n, 2)), list(range(1, n, 2))
    link, deg = CR.graph(n, list(zip(even[:-1], even[1:])) + list(zip(odd[:-1], odd[1:])))
    _r, count = _check(lib, link, deg, 1, lanes)
    assert count == 2


# ---- 3. a long path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("ascending", "descending", "bit_reversed"))
def test_labels_on_a_long_path(lib, order):
    """A path of 4,096 rows: the component's label has to travel the whole path.  Correctness is the test; the rounds are printed
    (DESIGN.md records them)."""
    idx = {"ascending": np.arange(4096), "descending": np.arange(4096)[::-1], "bit_reversed": CR.bit_reverse(12)}[order]
    link, deg = CR.path(idx)
    lists = LR.csr_from_link(link)
    for ms in (1, 3):                                      # at 3 the two ends (degree 2) are border rows
        want = CR.labels_ref(link, deg, ms)
        for lanes in LANES:
            rounds, count = _check(lib, link, deg, ms, lanes, want=want, lists=lists)
            print(f"path of 4096, {order}, min_samples {ms}, lanes_per_row {lanes}: rounds = {rounds}")
            assert count == 1


# ---- 4. the range search feeds it -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.METRICS))
def test_lists_equal_bitmap_on_the_table(lib, name):
    from truely_amd.gallery import FaceGallery
    g, _q = G.tables()
    metric = G.METRICS[name]
    gal = FaceGallery(metric=name, capacity=32)
    empty = gal.cluster(0.5, return_info=True, method="lists")
    assert empty["labels"].shape == (0,) and empty["n_clusters"] == 0 and empty["method"] == "lists" and empty["links"] == 0
    gal.add(g, range(257))
    for thr in CR.TABLE_THR[metric]:
        for invalid in ((), CR.INVALID):
            valid = CR.mask(257, invalid) if invalid else None
            link, deg = CR.table_links(metric, thr, 257, invalid)
            for ms in (1, 3):
                want = gal.cluster(thr, min_samples=ms, valid=valid, return_info=True, method="bitmap")
                auto = gal.cluster(thr, min_samples=ms, valid=valid, return_info=True)
                assert want["method"] == "bitmap" and auto["method"] == "bitmap" and "links" not in want
                popcount = int((want["degree"][want["degree"] > 0] - 1).sum().item())
                assert popcount == int(link.sum())
                for strip in (0, 128):
                    got = gal.cluster(thr, min_samples=ms, valid=valid, return_info=True, max_strip_cols=strip, method="lists")
                    assert got["method"] == "lists" and got["links"] == popcount and got["rounds"] >= 1
                    for k in ("labels", "core", "degree"):
                        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (name, thr, invalid, ms, strip, k)
                    assert got["n_clusters"] == want["n_clusters"] == CR.labels_ref(link, deg, ms)[2]
                labels = gal.cluster(thr, min_samples=ms, valid=valid, method="lists")
                assert labels.dtype == torch.int32 and torch.equal(labels, want["labels"])
        total = int(CR.table_links(metric, thr)[0].sum())
        assert gal.cluster(thr, method="lists", max_links=total, return_info=True)["links"] == total
        with pytest.raises(ValueError, match=str(total)):
            gal.cluster(thr, method="lists", max_links=total - 1)
    with pytest.raises(ValueError, match="method"):
        gal.cluster(0.5, method="matrix")
    with pytest.raises(_lib.TrlError, match="trl_cluster_labels_lists"):
        gal.cluster(CR.TABLE_THR[metric][0], min_samples=0, method="lists")


# ---- 5. stray indices -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_stray_indices_are_skipped(lib, lanes):
    """Entries -1, n and n + 1 put into the table's lists -- in front, in the middle and behind, and into empty lists -- are never
    followed: labels, core flags and count are those of the clean lists (a row's degree is its list's length + 1, so it counts
    them, and the reference is given those degrees).  The workspace lies inside zeros of the test's own, so a walk that followed a
    stray entry would read a label 0 there and show as a wrong label, not as a fault."""
    n = 257
    link, deg = CR.table_links(G.COSINE, 0.12, n)
    offsets, index = LR.csr_from_link(link)
    rows, extra = [], np.zeros(n, np.int32)
    for i in range(n):
        row = index[offsets[i]:offsets[i + 1]].tolist()
        if i % 3 == 0:
            row = [-1] + row[:len(row) // 2] + [n] + row[len(row) // 2:] + [n + 1]
            extra[i] = 3
        elif i % 3 == 1:
            row = row + [n + 1, -1]
            extra[i] = 2
        rows.append(row)
    dirty = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32))
    assert (extra[np.diff(offsets) == 0] > 0).any()
    _check(lib, link, deg, 1, lanes, lists=dirty, want_deg=deg + extra, ws_inside=True)        # min_samples = 1: core whatever the degree
    for ms in (3, 6):
        _check(lib, link, deg, ms, lanes, want=CR.labels_ref(link, deg + extra, ms), lists=dirty, want_deg=deg + extra, ws_inside=True)
    _check(lib, link, deg, 3, lanes, ws_inside=True)                                              # and the clean lists in the same place


# ---- 6. past the bitmap's limit ---------------------------------------------------------------------------------------------------
def test_cluster_past_the_bitmap_limit(lib):
    """66,000 rows of the chain input (tests/cluster_lists_ref.py; checked densely in test_cluster_lists_cpu.py): method="auto" takes
    the lists, and labels, core flags, degrees and count equal the union-find's at min_samples = 1 (a cluster per chain) and at the
    min_samples that makes the chain ends border rows."""
    from truely_amd.gallery import FaceGallery, MAX_CLUSTER_ROWS
    n = 66000
    assert n > MAX_CLUSTER_ROWS == CR.MAX_N
    emb, types, pairs = LR.chain_rows(n)
    gal = FaceGallery(metric="cosine", capacity=n)
    gal.add(torch.from_numpy(emb).cuda(), range(n))
    border_ms = LR.chain_border_ms(types, pairs)
    for ms in (1, border_ms):
        want_l, want_c, want_d, want_n = LR.chain_expect(types, pairs, ms)
        info = gal.cluster(LR.CHAIN_THR, min_samples=ms, return_info=True)
        print(f"chains of {n}, min_samples {ms}: links {info['links']} clusters {info['n_clusters']} rounds {info['rounds']}")
        assert info["method"] == "lists" and info["links"] == int(want_d.sum()) - n
        assert np.array_equal(info["degree"].cpu().numpy(), want_d) and np.array_equal(info["core"].cpu().numpy(), want_c)
        assert np.array_equal(info["labels"].cpu().numpy(), want_l) and info["n_clusters"] == want_n
    assert want_n == len(LR.CHAINS) - 2 and (want_l[want_c == 0] >= 0).any() and (want_l == -1).any()
    with pytest.raises(ValueError, match="65536"):
        gal.cluster(LR.CHAIN_THR, method="bitmap")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    link, deg = CR.table_links(G.COSINE, 0.12, 33)
    offsets, index = LR.csr_from_link(link)

    def refused(null=(), **kw):
        a = dict(n=33, min_samples=2, lanes=0, ws_delta=0, ws_offset=0)
        a.update(kw)
        st, degree, labels, core, count, _r = _raw(lib, offsets, index, None, a["n"], a["min_samples"], a["lanes"], a["ws_delta"],
                                                   a["ws_offset"], null=null)
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_cluster_labels_lists"), (kw, null, st, lib.trl_last_error())
        assert (degree == FILL_DEG).all() and (labels == FILL_LABEL).all() and (core == FILL_CORE).all() and (count == FILL_COUNT).all(), (kw, null)

    for kw in (dict(n=-1), dict(n=MAX_LIST_N + 1), dict(min_samples=0), dict(min_samples=-1), dict(lanes=1), dict(lanes=8), dict(lanes=32),
               dict(lanes=128), dict(lanes=-4), dict(ws_delta=-1), dict(ws_offset=4)):
        refused(**kw)
    for null in ("offsets", "index", "degree", "labels", "core", "count"):
        refused(null=(null,))
    want = CR.labels_ref(link, deg, 2)
    st, degree, labels, core, count, r = _raw(lib, offsets, index, None, 33, 2, 0, rounds=False)       # null d_valid and rounds_out are fine
    assert st == 0 and np.array_equal(labels[1:-1], want[0]) and np.array_equal(degree[1:-1], deg) and count[1] == want[2]
    for null in ((), ("offsets", "index", "degree", "labels", "core")):                                  # n = 0: the count is 0, nothing else
        st, degree, labels, core, count, r = _raw(lib, [0], [], None, 0, 2, 0, null=null)
        assert st == 0 and (degree == FILL_DEG).all() and (labels == FILL_LABEL).all() and (core == FILL_CORE).all()
        assert count.tolist() == [FILL_COUNT, 0, FILL_COUNT] and r == 0
    assert lib.trl_cluster_workspace(65537) == 0


def test_method_refusals(lib):
    from truely_amd.gallery import FaceGallery
    gal = FaceGallery(metric="cosine", capacity=65537)
    gal.add(torch.zeros((65537, G.K), dtype=torch.float32, device="cuda"), range(65537))
    with pytest.raises(ValueError, match="65536"):
        gal.cluster(0.5, method="bitmap")
    for method in ("list", "", None, "BITMAP"):
        with pytest.raises(ValueError, match="method"):
            gal.cluster(0.5, method=method)
    with pytest.raises(ValueError, match="method"):
        truely_amd.cluster_embeddings(np.zeros((4, G.K), np.float32), 0.5, device="cuda", method="dense")


# ---- 8. rows on a line ------------------------------------------------------------------------------------------------------------
def test_cluster_embeddings_on_a_line_by_lists():
    """test_gpu_cluster.py's line of 300 rows (euclidean, thr 1.5: the links are |p_i - p_j| = 1) through method="lists"."""
    from truely_amd.gallery import cluster_embeddings
    p = np.random.default_rng(300).permutation(300)
    emb = np.zeros((300, G.K), np.float32)
    emb[:, 0] = p
    info = cluster_embeddings(torch.from_numpy(emb).cuda(), 1.5, metric="euclidean", return_info=True, method="lists")
    assert info["labels"].dtype == torch.int32 and info["labels"].device.type == "cuda" and info["labels"].shape == (300,)
    assert info["n_clusters"] == 1 and (info["labels"].cpu().numpy() == 0).all() and info["core"].cpu().numpy().all()
    assert np.array_equal(info["degree"].cpu().numpy(), np.where((p == 0) | (p == 299), 2, 3))
    assert info["method"] == "lists" and info["links"] == 2 * 299
    print("line of 300 by lists: rounds =", info["rounds"])
    info = cluster_embeddings(emb, 1.5, metric="euclidean", min_samples=3, return_info=True, device="cuda", method="lists")      # a host array
    ends = (p == 0) | (p == 299)
    assert info["n_clusters"] == 1 and (info["labels"].cpu().numpy() == 0).all()
    assert np.array_equal(info["core"].cpu().numpy(), (~ends).astype(np.uint8))
    labels = cluster_embeddings(torch.from_numpy(emb).cuda(), 0.5, metric="euclidean", method="lists")      # nothing links: 300 clusters in row order
    assert np.array_equal(labels.cpu().numpy(), np.arange(300))
    assert cluster_embeddings(torch.from_numpy(emb).cuda(), 0.5, metric="euclidean", method="lists", max_links=0).shape == (300,)
