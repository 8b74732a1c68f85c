"""The embedding match on the device (csrc/trl_gallery.hip) against tests/gallery_ref.py bit for bit: trl_gallery_pack,
trl_gallery_scores, trl_gallery_search, their refusals, and gallery.py on top of them.

The kernels tile queries by 32 and gallery columns by 32 per wave / 128 per workgroup, and the search walks strips of 128-column
groups whose lists a second kernel merges.  So the table sits on both sides of every edge: m in {1, 31, 32, 33, 127, 128, 129, 257}
(a lone column, a wave's slab short of / equal to / past 32, a group short of / equal to / past 128, three groups with a lone
column in the third), n in {1, 2, 16, 17, 31, 32, 33, 65} (partial, full, two and three tiles), k in {1, 2, 5, 16} (k > m
included), every search once with the default strips and once with strips of 128 columns (one strip per group: the merge).
Every output lies in a NaN / -1 prefilled buffer with a guard row on either side, the score matrix with guard columns too.  Scores
are compared as uint32 (NaN by class), indices exactly."""
import ctypes as C_
import functools
import os

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
import gallery_ref as G

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
TABLE_M = (1, 31, 32, 33, 127, 128, 129, 257)
TABLE_N = (1, 2, 16, 17, 31, 32, 33, 65)
TABLE_K = (1, 2, 5, 16)
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
    """rows on the device; misalign: at an address that is 4 but not 16 bytes aligned."""
    rows = np.ascontiguousarray(rows, np.float32)
    if not misalign:
        return torch.from_numpy(rows.copy()).cuda()
    big = torch.zeros(rows.size + 8, dtype=torch.float32, device="cuda")
    v = big[1:1 + rows.size]
    v.copy_(torch.from_numpy(rows.copy()).reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


def _pack(lib, rows: np.ndarray, ld: int, c0: int = 0, mat=None, n2=None):
    """(mat [512][ld], n2 [ld]) with `rows` packed at column c0 (into zeroed tensors unless given)."""
    if mat is None:
        mat = torch.zeros((G.K, ld), dtype=torch.float32, device="cuda")
        n2 = torch.zeros((ld,), dtype=torch.float32, device="cuda")
    st = lib.trl_gallery_pack(_ptr(_dev(rows)), len(rows), _ptr(mat), ld, _ptr(n2), c0, _stream())
    assert st == 0, lib.trl_last_error()
    return mat, n2


@pytest.fixture(scope="module")
def table_gallery(lib):
    """The whole gallery table packed once, ld = 288.  A call with m < 257 reads its first m columns; the columns behind them
    hold other rows, not zeros, so a kernel that looked past m would show."""
    g, _q = G.tables()
    mat, n2 = _pack(lib, g, 288)
    return mat, n2, 288


def _raw_scores(lib, q_t, n, mat, ld, n2, m, metric, ldo, null=()):
    buf = torch.full((max(n, 1) + 2, max(ldo, 1)), float("nan"), dtype=torch.float32, device="cuda")
    st = lib.trl_gallery_scores(_ptr(None if "q" in null else q_t), n, _ptr(None if "mat" in null else mat), ld, _ptr(n2), m, metric,
                                _ptr(None if "out" in null else buf[1]), ldo, _stream())
    torch.cuda.synchronize()
    return st, buf.cpu().numpy().view(np.uint32)


def _raw_search(lib, q_t, valid_t, n, mat, ld, n2, m, metric, k, strip_cols=0, ws_delta=0, ws_offset=0):
    """trl_gallery_search into prefilled buffers with guard rows: (status, score bits (n + 2, k), index (n + 2, k))."""
    rows, kk = max(n, 1) + 2, max(k, 1)
    score = torch.full((rows, kk), float("nan"), dtype=torch.float32, device="cuda")
    index = torch.full((rows, kk), -7, dtype=torch.int32, device="cuda")
    need = lib.trl_gallery_search_workspace(n, m, k, strip_cols)
    size = max(need + ws_delta, 0)
    ws = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")[ws_offset:ws_offset + size] if size else None
    st = lib.trl_gallery_search(_ptr(q_t), _ptr(valid_t), n, _ptr(mat), ld, _ptr(n2), m, metric, k, _ptr(score[1]), _ptr(index[1]),
                                _ptr(ws), size, strip_cols, _stream())
    torch.cuda.synchronize()
    return st, score.cpu().numpy().view(np.uint32), index.cpu().numpy()


def _untouched(sbits, ibits):
    return (sbits == NAN_BITS).all() and (ibits == -7).all()


@functools.lru_cache(maxsize=None)
def _table_topk(metric: int, m: int, k: int):
    return G.topk_ref(G.table_scores(metric)[:, :m], metric, k)


def _check_search(lib, q_t, n, gal, m, metric, k, want_idx, want_sc, valid_t=None, strip_cols=(0, 128)):
    mat, n2, ld = gal
    outs = []
    for sc_cols in strip_cols:
        st, sbits, idx = _raw_search(lib, q_t, valid_t, n, mat, ld, n2, m, metric, k, sc_cols)
        assert st == 0, lib.trl_last_error()
        assert _untouched(sbits[[0, -1]], idx[[0, -1]]), "guard row written"
        got_s, got_i = sbits[1:-1].view(np.float32), idx[1:-1]
        assert np.array_equal(got_i, want_idx), (m, n, k, metric, sc_cols, np.argwhere(got_i != want_idx)[:3].tolist())
        ok = G.same_bits(got_s, want_sc)
        assert ok.all(), (m, n, k, metric, sc_cols, np.argwhere(~ok)[:3].tolist())
        outs.append((sbits, idx))
    for sbits, idx in outs[1:]:                            # the runs equal each other as well (NaN payloads included)
        assert np.array_equal(idx, outs[0][1]) and np.array_equal(np.isnan(sbits.view(np.float32)), np.isnan(outs[0][0].view(np.float32)))
    return outs[0]


# ---- pack ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (1, 31, 32, 33, 128, 129))
def test_pack(lib, m):
    g, _q = G.tables()
    want_n2 = G.table_n2()
    for c0 in (0, 1, 37):
        ld = (c0 + m + 31) // 32 * 32 + 32
        mat, n2 = _pack(lib, g[:m], ld, c0)
        torch.cuda.synchronize()
        mat, n2 = mat.cpu().numpy(), n2.cpu().numpy()
        assert G.same_bits(mat[:, c0:c0 + m], g[:m].T).all(), (m, c0)
        assert G.same_bits(n2[c0:c0 + m], want_n2[:m]).all(), (m, c0)
        assert not mat[:, :c0].view(np.uint32).any() and not mat[:, c0 + m:].view(np.uint32).any(), "padding columns written"
        assert not n2[:c0].view(np.uint32).any() and not n2[c0 + m:].view(np.uint32).any()


def test_pack_two_appends(lib):
    g, _q = G.tables()
    mat, n2 = _pack(lib, g[:33], 96)
    _pack(lib, g[33:73], 96, 33, mat, n2)
    torch.cuda.synchronize()
    mat, n2 = mat.cpu().numpy(), n2.cpu().numpy()
    assert G.same_bits(mat[:, :73], g[:73].T).all() and G.same_bits(n2[:73], G.table_n2()[:73]).all()
    assert not mat[:, 73:].view(np.uint32).any() and not n2[73:].view(np.uint32).any()


# ---- scores ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", TABLE_M)
def test_scores(lib, table_gallery, m):
    mat, n2, ld = table_gallery
    _g, q = G.tables()
    q_t, q_mis = _dev(q), _dev(q[:33], misalign=True)
    for metric in (G.COSINE, G.EUCLIDEAN):
        ref = G.table_scores(metric)
        for n in TABLE_N:
            for ldo, qq in ((m, q_t), (m + 5, q_t)) + (((m + 5, q_mis),) if n == 33 else ()):
                st, bits = _raw_scores(lib, qq, n, mat, ld, n2, m, metric, ldo)
                assert st == 0, lib.trl_last_error()
                assert (bits[0] == NAN_BITS).all() and (bits[n + 1:] == NAN_BITS).all(), "guard row written"
                assert (bits[1:n + 1, m:] == NAN_BITS).all(), "guard columns written"
                ok = G.same_bits(bits[1:n + 1, :m].view(np.float32), ref[:n, :m])
                assert ok.all(), (metric, m, n, ldo, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


# ---- search ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", TABLE_M)
def test_search(lib, table_gallery, m):
    _g, q = G.tables()
    q_t = _dev(q)
    for metric in (G.COSINE, G.EUCLIDEAN):
        for k in TABLE_K:
            want_idx, want_sc = _table_topk(metric, m, k)
            for n in TABLE_N:
                _check_search(lib, q_t, n, table_gallery, m, metric, k, want_idx[:n], want_sc[:n])
    q_mis = _dev(q[:33], misalign=True)
    want_idx, want_sc = _table_topk(G.COSINE, m, 5)
    _check_search(lib, q_mis, 33, table_gallery, m, G.COSINE, 5, want_idx[:33], want_sc[:33])


def test_duplicates_across_strips(lib, table_gallery):
    """Queries 0 and 32 are the row that the gallery holds five times, in three column groups: with strips of 128 columns the five
    reach the merge from three strips, with equal scores, and come out in index order."""
    _g, q = G.tables()
    for metric in (G.COSINE, G.EUCLIDEAN):
        want_idx, want_sc = _table_topk(metric, 257, 5)
        assert want_idx[0].tolist() == list(G.DUPS) and want_idx[32].tolist() == list(G.DUPS)
        sbits, idx = _check_search(lib, _dev(q), 33, table_gallery, 257, metric, 5, want_idx[:33], want_sc[:33])
        assert len(set(sbits[1, :5].tolist())) == 1 and idx[1].tolist() == list(G.DUPS)


def test_zero_sign_tie(lib):
    """-0 == +0: four gallery rows whose cosine is +0, -0, +0, -0, apart in three column groups among rows of negative cosine."""
    gz, qz = G.zero_sign_rows()
    place = {0: 0, 2: 130, 3: 131, 4: 260, 5: 262}
    g = np.repeat(gz[1:2], 263, axis=0)
    for src, at in place.items():
        g[at] = gz[src]
    ref = G.scores_ref(qz, g, G.COSINE)
    assert np.signbit(ref[0, [130, 260]]).all() and (ref[0, [0, 130, 131, 260]] == 0).all()
    mat, n2 = _pack(lib, g, 288)
    want_idx, want_sc = G.topk_ref(ref, G.COSINE, 6)
    assert want_idx[0].tolist() == [262, 0, 130, 131, 260, 1]
    sbits, idx = _check_search(lib, _dev(qz), 1, (mat, n2, 288), 263, G.COSINE, 6, want_idx, want_sc)
    assert sbits[1, 1:5].tolist() == [0, 0x80000000, 0, 0x80000000]
    st, bits = _raw_scores(lib, _dev(qz), 1, mat, 288, n2, 263, G.COSINE, 263)
    assert st == 0 and G.same_bits(bits[1].view(np.float32), ref[0]).all()


def test_valid_mask_and_special_rows(lib, table_gallery):
    _g, q = G.tables()
    valid = np.ones(65, np.uint8)
    valid[[0, 5, 31, 32, 64]] = 0
    valid[7] = 255
    v_t = torch.from_numpy(valid).cuda()
    for metric in (G.COSINE, G.EUCLIDEAN):
        want_idx, want_sc = G.topk_ref(G.table_scores(metric), metric, 5, valid)
        assert (want_idx[[0, 5, 31, 32, 64]] == -1).all()
        _check_search(lib, _dev(q), 65, table_gallery, 257, metric, 5, want_idx, want_sc, valid_t=v_t)
    # the zero query (1) and the NaN query (3) score NaN everywhere under cosine: NaN ranks by index
    sbits, idx = _check_search(lib, _dev(q), 5, table_gallery, 257, G.COSINE, 5, *[a[:5] for a in _table_topk(G.COSINE, 257, 5)])
    assert idx[2].tolist() == [0, 1, 2, 3, 4] and idx[4].tolist() == [0, 1, 2, 3, 4] and np.isnan(sbits[[2, 4]].view(np.float32)).all()
    # gallery rows holding NaN / zero (cosine) rank behind every row with a score
    want_idx, _ = _table_topk(G.COSINE, 12, 12)
    assert want_idx[8, -4:].tolist() == [G.ZERO_G, G.NAN_G, G.INF_G, G.MIXINF_G]      # 0 / 0, NaN, inf / inf, inf - inf
    _check_search(lib, _dev(q), 16, table_gallery, 12, G.COSINE, 12, *[a[:16] for a in _table_topk(G.COSINE, 12, 12)])


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_row_alone_equals_batch(lib, table_gallery, metric):
    """Row r of the 65-row call has the bits of the same row searched and scored alone: no dependence on n, tile or position."""
    mat, n2, ld = table_gallery
    _g, q = G.tables()
    q_t = _dev(q)
    want_idx, want_sc = _table_topk(metric, 257, 5)
    sbits, idx = _check_search(lib, q_t, 65, table_gallery, 257, metric, 5, want_idx, want_sc, strip_cols=(0,))
    st, whole = _raw_scores(lib, q_t, 65, mat, ld, n2, 257, metric, 257)
    assert st == 0
    for r in range(65):
        st, s1, i1 = _raw_search(lib, q_t[r:r + 1], None, 1, mat, ld, n2, 257, metric, 5)
        assert st == 0 and np.array_equal(i1[1], idx[1 + r]) and G.same_bits(s1[1].view(np.float32), sbits[1 + r].view(np.float32)).all(), r
        st, b1 = _raw_scores(lib, q_t[r:r + 1], 1, mat, ld, n2, 257, metric, 257)
        assert st == 0 and G.same_bits(b1[1].view(np.float32), whole[1 + r].view(np.float32)).all(), r


def test_large_gallery(lib):
    """m = 65,600 (indices past 16 bits, 513 column groups: the default plan's 257 strips of 2 groups, four or five to a lane of the merge), n = 3,
    k = 16.  The query rows are gallery rows 5 and 65,599 and a fresh row; row 5 is enrolled again at 70 and at 65,598."""
    rng = np.random.default_rng(65600)
    m = 65600
    g = rng.standard_normal((m, G.K), dtype=np.float32)
    g[70] = g[5]; g[65598] = g[5]
    q = np.stack([g[5], g[65599], rng.standard_normal(G.K, dtype=np.float32)])
    ld = (m + 31) // 32 * 32
    mat, n2 = _pack(lib, g, ld)
    assert lib.trl_gallery_search_workspace(3, m, 16, 0) == 257 * 3 * 16 * 8
    qn2 = G.n2_ref(q)
    ref = {metric: np.empty((3, m), np.float32) for metric in (G.COSINE, G.EUCLIDEAN)}
    for c0 in range(0, m, 8200):                                          # in column blocks; the chains once for both metrics
        gb = g[c0:c0 + 8200]
        dot, gn2 = G.dot_ref(q, gb), G.n2_ref(gb)
        for metric in ref:
            ref[metric][:, c0:c0 + 8200] = G.scores_from(dot, qn2, gn2, metric)
    for metric in (G.COSINE, G.EUCLIDEAN):
        want_idx, want_sc = G.topk_ref(ref[metric], metric, 16)
        assert want_idx[0, :3].tolist() == [5, 70, 65598] and want_idx[1, 0] == 65599
        _check_search(lib, _dev(q), 3, (mat, n2, ld), m, metric, 16, want_idx, want_sc, strip_cols=(0,))


# ---- stream, workspace, refusals -------------------------------------------------------------------------------------------------
def test_side_stream(lib, table_gallery):
    _g, q = G.tables()
    want_idx, want_sc = _table_topk(G.EUCLIDEAN, 257, 5)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        q_t = _dev(q)
        _check_search(lib, q_t, 65, table_gallery, 257, G.EUCLIDEAN, 5, want_idx, want_sc)
        mat, n2, ld = table_gallery
        st, bits = _raw_scores(lib, q_t, 65, mat, ld, n2, 257, G.EUCLIDEAN, 257)
        side.synchronize()
    assert st == 0 and G.same_bits(bits[1:66].view(np.float32), G.table_scores(G.EUCLIDEAN)).all()


def test_refusals(lib, table_gallery):
    mat, n2, ld = table_gallery
    _g, q = G.tables()
    q_t = _dev(q)
    need = lib.trl_gallery_search_workspace(33, 257, 5, 128)
    assert need == 3 * 33 * 5 * 8

    def refused_search(**kw):
        a = dict(n=33, ld=ld, m=257, metric=0, k=5, strip_cols=128, ws_delta=0, ws_offset=0)
        a.update(kw)
        st, sbits, idx = _raw_search(lib, q_t, None, a["n"], mat, a["ld"], n2, a["m"], a["metric"], a["k"], a["strip_cols"], a["ws_delta"], a["ws_offset"])
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_search"), (kw, st, lib.trl_last_error())
        assert _untouched(sbits, idx), kw

    refused_search(ws_delta=-1)                            # one byte too small
    refused_search(ws_offset=4)                            # not 8-byte aligned
    for kw in (dict(ld=100), dict(ld=0), dict(ld=256), dict(k=0), dict(k=17), dict(metric=2), dict(metric=-1), dict(strip_cols=100),
               dict(strip_cols=-128), dict(n=-1), dict(m=-1), dict(m=2 ** 31, ld=2 ** 31)):
        refused_search(**kw)
    st, sbits, idx = _raw_search(lib, q_t, None, 33, mat, ld, n2, 257, 0, 5, 128)       # and the same call with its workspace passes
    assert st == 0 and np.array_equal(idx[1:-1], _table_topk(0, 257, 5)[0][:33])
    for kw, null in ((dict(ld=100), ()), (dict(ld=256), ()), (dict(ldo=256), ()), (dict(metric=2), ()), (dict(n=-1), ()), (dict(m=-1), ()),
                     ({}, ("q",)), ({}, ("out",)), ({}, ("mat",))):
        a = dict(n=33, ld=ld, m=257, metric=0, ldo=257)
        a.update(kw)
        st, bits = _raw_scores(lib, q_t, a["n"], mat, a["ld"], n2, a["m"], a["metric"], a["ldo"], null)
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_scores"), (kw, null)
        assert (bits == NAN_BITS).all()
    g_t = _dev(_g[:40])
    z_mat, z_n2 = torch.zeros((G.K, 64), dtype=torch.float32, device="cuda"), torch.zeros((64,), dtype=torch.float32, device="cuda")
    for m_, ld_, c0 in ((40, 64, 25), (40, 48, 0), (40, 0, 0), (-1, 64, 0), (40, 64, -1)):
        assert lib.trl_gallery_pack(_ptr(g_t), m_, _ptr(z_mat), ld_, _ptr(z_n2), c0, _stream()) == TRL_ERR_INVALID, (m_, ld_, c0)
        assert lib.trl_last_error().startswith(b"trl_gallery_pack")
    assert lib.trl_gallery_pack(None, 40, _ptr(z_mat), 64, _ptr(z_n2), 0, _stream()) == TRL_ERR_INVALID
    torch.cuda.synchronize()
    assert not z_mat.cpu().numpy().view(np.uint32).any() and not z_n2.cpu().numpy().view(np.uint32).any()


def test_empty_calls(lib, table_gallery):
    mat, n2, ld = table_gallery
    q_t = _dev(G.tables()[1])
    st, sbits, idx = _raw_search(lib, q_t, None, 0, mat, ld, n2, 257, 0, 5)             # n = 0: nothing is done
    assert st == 0 and _untouched(sbits, idx)
    st, sbits, idx = _raw_search(lib, q_t, None, 3, mat, ld, n2, 0, 0, 5)               # m = 0: -1 / NaN
    assert st == 0 and _untouched(sbits[[0, -1]], idx[[0, -1]]) and (idx[1:-1] == -1).all() and np.isnan(sbits[1:-1].view(np.float32)).all()
    for n, m in ((0, 257), (3, 0)):
        st, bits = _raw_scores(lib, q_t, n, mat, ld, n2, m, 0, 257)
        assert st == 0 and (bits == NAN_BITS).all()
    assert lib.trl_gallery_pack(_ptr(q_t), 0, _ptr(mat), ld, _ptr(n2), 257, _stream()) == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_face_gallery(lib, table_gallery):
    from truely_amd.gallery import FaceGallery, pairwise
    assert truely_amd.FaceGallery is FaceGallery and truely_amd.pairwise is pairwise
    g, q = G.tables()
    labels = [f"id{r}" for r in range(257)]
    for name, metric in G.METRICS.items():
        gal = FaceGallery(metric=name, capacity=32)
        assert len(gal) == 0 and gal.labels == [] and gal.scores(q[:2]).shape == (2, 0)
        idx, sc = gal.search(q[:2], k=3)
        assert (idx.cpu().numpy() == -1).all() and np.isnan(sc.cpu().numpy()).all()
        assert gal.identify(q[:2])[0] == [None, None]
        gal.add(g[:20], labels[:20])                                  # a host array
        before_rows, before_n2 = gal.rows().cpu().numpy(), gal._n2[:20].cpu().numpy()
        gal.add(torch.from_numpy(g[20:50].copy()).cuda(), labels[20:50])   # a device tensor, past the capacity of 32: grows to 64
        assert gal.ld == 64 and len(gal) == 50
        gal.add(g[50:257], labels[50:257])
        assert len(gal) == 257 and gal.labels == labels and gal.ld >= 257 and gal.ld % 32 == 0
        rows = gal.rows()
        assert rows.device.type == "cuda" and G.same_bits(rows.cpu().numpy(), g).all()          # the round trip keeps the bits
        assert G.same_bits(rows.cpu().numpy()[:20], before_rows).all() and G.same_bits(gal._n2[:20].cpu().numpy(), before_n2).all()
        assert G.same_bits(gal._n2[:257].cpu().numpy(), G.table_n2()).all() and not gal._n2[257:].cpu().numpy().any()
        assert not gal._mat[:, 257:].cpu().numpy().any()
        ref = G.table_scores(metric)
        s = gal.scores(torch.from_numpy(q.copy()).cuda())
        assert s.shape == (65, 257) and s.device.type == "cuda" and G.same_bits(s.cpu().numpy(), ref).all()
        idx, sc = gal.search(q, k=5)
        want_idx, want_sc = _table_topk(metric, 257, 5)
        assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and idx.device.type == "cuda"
        assert np.array_equal(idx.cpu().numpy(), want_idx) and G.same_bits(sc.cpu().numpy(), want_sc).all()
        valid = np.ones(65, np.uint8); valid[2] = 0
        idx_v, _ = gal.search(q, k=5, valid=valid)
        assert (idx_v[2].cpu().numpy() == -1).all() and np.array_equal(idx_v[3:].cpu().numpy(), want_idx[3:])
        # identify: the label of the best match; None for NaN scores, invalid rows and matches that fail the threshold
        best_i, best_s = want_idx[:, 0], want_sc[:, 0]
        names, score = gal.identify(q)
        assert G.same_bits(score.cpu().numpy(), best_s).all()
        assert names == [None if np.isnan(best_s[r]) else labels[best_i[r]] for r in range(65)]
        assert names[0] == "id2" and names[32] == "id2" and names[3] is None
        if metric == G.EUCLIDEAN:                                     # (under cosine the subnormal row 12, whose n2 is 0, scores +-inf)
            assert names[7] in ("id14", "id15") and names[30] in ("id60", "id61")
        thr = 0.5 if metric == G.COSINE else 10.0                     # between a row's own copies (1 / 0) and unrelated rows (~0.1 / ~32)
        with np.errstate(invalid="ignore"):
            keep = (best_s >= thr) if metric == G.COSINE else (best_s <= thr)
        assert keep[0] and keep[32] and not keep[3] and not keep.all()
        names_t, _ = gal.identify(q, threshold=thr)
        assert names_t == [labels[best_i[r]] if keep[r] else None for r in range(65)] and names_t[0] == "id2" and names_t[3] is None
        assert gal.identify(q, valid=valid)[0][2] is None
        with pytest.raises(ValueError):
            gal.add(g[:3], labels[:2])
        with pytest.raises(ValueError):
            gal.search(q, k=17)
        with pytest.raises(ValueError):
            gal.search(q[:, :100])
        p = pairwise(torch.from_numpy(q[:9].copy()).cuda(), torch.from_numpy(g[:40].copy()).cuda(), metric=name)
        assert p.device.type == "cuda" and G.same_bits(p.cpu().numpy(), ref[:9, :40]).all()
    with pytest.raises(ValueError):
        FaceGallery(metric="manhattan")
    # the README's table: pairwise(e) is (e_i - e_j).norm() to within the bound of tests/test_gallery_cpu.py; the diagonal is 0
    e = q[8:16]
    p = pairwise(e).cpu().numpy()
    want = np.sqrt(((e[:, None, :].astype(np.float64) - e[None, :, :]) ** 2).sum(axis=2))
    assert p.shape == (8, 8) and G.same_bits(p, G.scores_ref(e, e, G.EUCLIDEAN)).all()
    # unit rows: s = 2 (1 + O(u)), S <= 1, so E <= (2 a + 2 g)(1 + u) + u d2 < 4.2 gamma(512) in test_gallery_cpu.py's bound
    off = ~np.eye(8, dtype=bool)
    E = 4.2 * G.gamma(512)
    assert (np.abs(p - want)[off] <= E / want[off] * (1 + G.U) + G.U * want[off]).all() and np.abs(np.diagonal(p)).max() <= np.sqrt(E)


def test_identify_end_to_end(engine):
    """Detect, extract and embed every face of the multi-face 270p clip on synthetic weights; enrol frame 0's faces; each face of
    the later frame that frame 0 shows too (a box centre within a quarter of the enrolled box's width: the faces drift by a pixel
    or two per frame, and the later frame also shows a face that frame 0 does not) is identified as the enrolled face it is."""
    from truely_amd.gallery import FaceGallery
    from truely_amd.inception_resnet_v1 import InceptionResnetV1
    z = np.load(os.path.join(GOLD, "clip_multiface_270p.npz"))
    fr = truely_amd.synthetic.synthetic_frames(int(z["n"]), int(z["H"]), int(z["W"]), seed=int(z["seed"]), faces=int(z["faces_per_frame"]))
    boxes, _p, counts = (t.cpu().numpy() for t in engine.mtcnn_detect(fr))
    later = len(fr) - 1
    assert later >= 1 and counts[0] >= 2 and 2 <= counts[later] <= counts[0], counts.tolist()
    rows = np.array([0] * int(counts[0]) + [later] * int(counts[later]), np.int32)
    bx = np.concatenate([boxes[0, :counts[0]], boxes[later, :counts[later]]]).astype(np.float32)
    faces, status = engine.extract_boxes(fr, torch.from_numpy(rows), torch.from_numpy(bx), 160, 0, "torch", True)
    assert (status.cpu().numpy() == 1).all()
    emb = InceptionResnetV1(engine=engine)(faces.to(engine.device))
    c, c1 = int(counts[0]), int(counts[later])
    centre = np.stack([(bx[:, 0] + bx[:, 2]) / 2, (bx[:, 1] + bx[:, 3]) / 2], 1)
    dist = np.sqrt(((centre[None, :c] - centre[c:, None]) ** 2).sum(axis=2))          # (later face, enrolled face)
    own = dist.argmin(axis=1)
    known = np.nonzero(dist.min(axis=1) < (bx[own, 2] - bx[own, 0]) / 4)[0]
    assert len(known) >= 2 and len(set(own[known].tolist())) == len(known), (own.tolist(), dist.tolist())
    for metric in ("cosine", "euclidean"):
        gal = FaceGallery(metric=metric, device=engine.device)
        gal.add(emb[:c], list(range(c)))
        names, score = gal.identify(emb[c:])
        print(metric, "own", own.tolist(), "known", known.tolist(), "identified", names, "score", score.cpu().numpy().tolist())
        assert [names[j] for j in known] == own[known].tolist()
        assert gal.identify(emb[:c])[0] == list(range(c))
