"""The grouped search on the device (k_gallery_search_groups / k_gallery_merge_groups in csrc/trl_gallery.hip) against
tests/group_ref.py: trl_gallery_search_groups, its refusals, and FaceGallery.identities / search_identities / identify_topk.

The kernel has the shared search body, so the sweep is test_gpu_gallery.py's: m in {1, 31, 32, 33, 127, 128, 129, 257} (a lone
column; a wave's slab short of / equal to / past 32; a group short of / equal to / past 128; three groups with a lone column in the
third), n in {1, 33, 65} (one row, two tiles, three tiles with a lone row), k in {1, 2, 5, 16}, both metrics, every case once with
the default strips and once with strips of 128 columns (one strip per column group: the merge kernel), and the two runs must be
equal.  The gid tables (group_ref.gid_tables) over the 257 gallery rows:

  distinct       i         must equal trl_gallery_search's output on the same inputs, as well as the reference
  one            0         one entry per query
  mod3           i % 3     fewer groups than k; every group in every lane, wave and strip
  div16          i // 16   replacement inside one lane's list (a lane walks 16 columns of a slab)
  div32          i // 32   replacement across the two lists of a wave
  div128         i // 128  replacement across waves, and across strips at strips of 128
  random_alone   0..39 at random, -1 at 25 scattered rows; the NaN / inf / zero rows each alone in a group
  random_shared  the same, those rows each sharing a group with an ordinary row
  random_slab    the same, and the whole first slab (rows 0..31) excluded

Every output lies in a NaN / -7 prefilled buffer with a guard row on either side, the workspace is exactly the bytes asked for,
scores are compared as uint32 (NaN by class), indices and groups exactly."""
import ctypes as C_

import numpy as np
import pytest
import torch

from truely_amd import _lib
import gallery_ref as G
import group_ref as GR

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
TABLE_M = (1, 31, 32, 33, 127, 128, 129, 257)
TABLE_N = (1, 33, 65)
TABLE_K = (1, 2, 5, 16)
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
    """rows on the device; misalign: at an address that is 4 but not 16 bytes aligned."""
    rows = np.ascontiguousarray(rows, np.float32)
    if not misalign:
        return torch.from_numpy(rows.copy()).cuda()
    big = torch.zeros(rows.size + 8, dtype=torch.float32, device="cuda")
    v = big[1:1 + rows.size]
    v.copy_(torch.from_numpy(rows.copy()).reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v


@pytest.fixture(scope="module")
def table_gallery(lib):
    """The whole gallery table packed once, ld = 288.  A call with m < 257 reads its first m columns; the columns behind them hold
    other rows, not zeros, so a kernel that looked past m would show."""
    g, _q = G.tables()
    mat = torch.zeros((G.K, 288), dtype=torch.float32, device="cuda")
    n2 = torch.zeros((288,), dtype=torch.float32, device="cuda")
    assert lib.trl_gallery_pack(_ptr(_dev(g)), len(g), _ptr(mat), 288, _ptr(n2), 0, _stream()) == 0, lib.trl_last_error()
    return mat, n2, 288


@pytest.fixture(scope="module")
def table_queries(lib):
    return _dev(G.tables()[1])


def _gid_dev(gid: np.ndarray, m: int):
    """Exactly m ids on the device (the kernel may read no more), None for m = 0."""
    return torch.from_numpy(np.ascontiguousarray(gid[:m], np.int32).copy()).cuda() if m > 0 else None


def _raw(lib, q_t, valid_t, n, gal, gid_t, m, metric, k, strip_cols=0, ws_delta=0, ws_offset=0, ld=None):
    """trl_gallery_search_groups into prefilled buffers with guard rows: (status, score bits, index, group), each (n + 2, k)."""
    mat, n2, ld0 = gal
    rows, kk = max(n, 1) + 2, max(k, 1)
    score = torch.full((rows, kk), float("nan"), dtype=torch.float32, device="cuda")
    index = torch.full((rows, kk), -7, dtype=torch.int32, device="cuda")
    group = torch.full((rows, kk), -7, dtype=torch.int32, device="cuda")
    need = lib.trl_gallery_search_groups_workspace(n, m, k, strip_cols)
    size = max(need + ws_delta, 0)
    ws = torch.empty((size + 16,), dtype=torch.uint8, device="cuda")[ws_offset:ws_offset + size] if size else None
    st = lib.trl_gallery_search_groups(_ptr(q_t), _ptr(valid_t), n, _ptr(mat), ld0 if ld is None else ld, _ptr(n2), _ptr(gid_t), m, metric, k,
                                       _ptr(score[1]), _ptr(index[1]), _ptr(group[1]), _ptr(ws), size, strip_cols, _stream())
    torch.cuda.synchronize()
    return st, score.cpu().numpy().view(np.uint32), index.cpu().numpy(), group.cpu().numpy()


def _untouched(sbits, idx, grp):
    return (sbits == NAN_BITS).all() and (idx == -7).all() and (grp == -7).all()


def _check(lib, q_t, n, gal, gid_t, m, metric, k, want, valid_t=None, strip_cols=(0, 128), what=""):
    """Both strip plans against `want` = (score, index, group) and against each other; returns the first run's (n, k) arrays."""
    want_sc, want_idx, want_grp = want
    outs = []
    for cols in strip_cols:
        st, sbits, idx, grp = _raw(lib, q_t, valid_t, n, gal, gid_t, m, metric, k, cols)
        tag = (what, m, n, k, metric, cols)
        assert st == 0, (tag, lib.trl_last_error())
        assert _untouched(sbits[[0, -1]], idx[[0, -1]], grp[[0, -1]]), ("guard row written", tag)
        got_s, got_i, got_g = sbits[1:-1].view(np.float32), idx[1:-1], grp[1:-1]
        assert np.array_equal(got_i, want_idx), (tag, np.argwhere(got_i != want_idx)[:3].tolist())
        assert np.array_equal(got_g, want_grp), (tag, np.argwhere(got_g != want_grp)[:3].tolist())
        ok = G.same_bits(got_s, want_sc)
        assert ok.all(), (tag, np.argwhere(~ok)[:3].tolist())
        outs.append((sbits, idx, grp))
    for sbits, idx, grp in outs[1:]:
        assert np.array_equal(idx, outs[0][1]) and np.array_equal(grp, outs[0][2])
        assert np.array_equal(np.isnan(sbits.view(np.float32)), np.isnan(outs[0][0].view(np.float32)))
    return outs[0][0][1:-1], outs[0][1][1:-1], outs[0][2][1:-1]


def _want(metric, name, m, k, n):
    return tuple(a[:n] for a in GR.table_group_topk(metric, name, m, k))


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(GR.gid_tables()))
def test_sweep(lib, table_gallery, table_queries, name):
    gid = GR.gid_tables()[name]
    mat, n2, ld = table_gallery
    for m in TABLE_M:
        gid_t = _gid_dev(gid, m)
        for metric in (G.COSINE, G.EUCLIDEAN):
            for k in TABLE_K:
                for n in TABLE_N:
                    sbits, idx, grp = _check(lib, table_queries, n, table_gallery, gid_t, m, metric, k, _want(metric, name, m, k, n), what=name)
                    if name == "distinct":                 # the plain search's output on the same inputs, bit for bit
                        score = torch.empty((n, k), dtype=torch.float32, device="cuda")
                        index = torch.empty((n, k), dtype=torch.int32, device="cuda")
                        need = lib.trl_gallery_search_workspace(n, m, k, 0)
                        ws = torch.empty((need,), dtype=torch.uint8, device="cuda") if need else None
                        assert lib.trl_gallery_search(_ptr(table_queries), None, n, _ptr(mat), ld, _ptr(n2), m, metric, k, _ptr(score), _ptr(index),
                                                      _ptr(ws), need, 0, _stream()) == 0
                        torch.cuda.synchronize()
                        assert np.array_equal(index.cpu().numpy(), idx) and np.array_equal(grp, idx)
                        plain = score.cpu().numpy()
                        assert G.same_bits(plain, sbits.view(np.float32)).all()


def test_replacement_happens(lib, table_gallery, table_queries):
    """The device result under the block tables holds rows that are not their group's first row, and the tied duplicates come out
    as each group's lowest-index copy: what test_groups_cpu.py asserts of the reference, seen in the kernel's own output."""
    t = GR.gid_tables()
    for metric in (G.COSINE, G.EUCLIDEAN):
        for name, per in (("div16", 16), ("div32", 32), ("div128", 128)):
            sbits, idx, grp = _check(lib, table_queries, 65, table_gallery, _gid_dev(t[name], 257), 257, metric, 16, _want(metric, name, 257, 16, 65))
            live = idx >= 0
            assert (idx[live] // per == grp[live]).all() and (idx[live] % per != 0).sum() > 65
        sbits, idx, grp = _check(lib, table_queries, 33, table_gallery, _gid_dev(t["div128"], 257), 257, metric, 3, _want(metric, "div128", 257, 3, 33))
        assert idx[0].tolist() == [2, 129, 256] and idx[32].tolist() == [2, 129, 256] and len(set(sbits[0].tolist())) == 1


def test_more_strips_than_merge_lanes(lib):
    """m = 8,960 at strips of 128 columns: 70 strips, so lanes 0..5 of k_gallery_merge_groups take two strips each before the fold.
    1,120 identities of 8 noisy rows each, scattered over the strips; the three queries are noisy copies of three identities, so
    each has eight strong rows of one group in up to eight strips, and 40 of the rows are excluded."""
    rng = np.random.default_rng(8960)
    m, per = 8960, 8
    centres = rng.standard_normal((m // per, G.K)).astype(np.float32)
    gid = rng.permutation(m).astype(np.int32) % (m // per)
    g = (centres[gid] + 0.3 * rng.standard_normal((m, G.K))).astype(np.float32)
    own = np.array([5, 600, 1119])
    q = (centres[own] + 0.3 * rng.standard_normal((3, G.K))).astype(np.float32)
    gid[rng.choice(m, 40, replace=False)] = -1
    gid[np.nonzero(gid == 600)[0][:3]] = -1                 # three of the eight strong rows of query 1 among them
    mat = torch.zeros((G.K, m), dtype=torch.float32, device="cuda")
    n2 = torch.zeros((m,), dtype=torch.float32, device="cuda")
    assert lib.trl_gallery_pack(_ptr(_dev(g)), m, _ptr(mat), m, _ptr(n2), 0, _stream()) == 0, lib.trl_last_error()
    assert lib.trl_gallery_search_groups_workspace(3, m, 16, 128) == (70 * 3 * 16 * 8 + 255) // 256 * 256 + 70 * 3 * 16 * 4
    for metric in (G.COSINE, G.EUCLIDEAN):
        ref = G.scores_ref(q, g, metric)
        want = GR.group_topk_ref(ref, gid, metric, 16)
        assert want[2][:, 0].tolist() == own.tolist() and (want[1] >= 0).all()
        strips_of_own = [len(set((np.nonzero(gid == o)[0] // 128).tolist())) for o in own]
        assert min(strips_of_own) >= 4                      # each strong group reaches the merge from several strips
        _check(lib, _dev(q), 3, (mat, n2, m), _gid_dev(gid, m), m, metric, 16, want)
        _check(lib, _dev(q), 3, (mat, n2, m), _gid_dev(gid, m), m, metric, 5, tuple(a[:, :5] for a in want))


# ---- further cases ---------------------------------------------------------------------------------------------------------------
def test_valid_mask(lib, table_gallery, table_queries):
    valid = np.ones(65, np.uint8)
    valid[[5, 31, 64]] = 0                                 # inside a tile, at the end of a tile, the lone row of the last tile
    valid[7] = 255
    v_t = torch.from_numpy(valid).cuda()
    gid = GR.gid_tables()["random_shared"]
    for metric in (G.COSINE, G.EUCLIDEAN):
        want = GR.group_topk_ref(G.table_scores(metric), gid, metric, 5, valid)
        assert (want[1][[5, 31, 64]] == -1).all() and (want[1][[4, 6, 30, 32, 63], 0] >= 0).all()
        _check(lib, table_queries, 65, table_gallery, _gid_dev(gid, 257), 257, metric, 5, want, valid_t=v_t)


def test_misaligned_queries(lib, table_gallery):
    q_mis = _dev(G.tables()[1][:33], misalign=True)
    gid = GR.gid_tables()["div16"]
    for m in (33, 257):
        _check(lib, q_mis, 33, table_gallery, _gid_dev(gid, m), m, G.COSINE, 5, _want(G.COSINE, "div16", m, 5, 33))


def test_side_stream(lib, table_gallery):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        q_t = _dev(G.tables()[1])
        _check(lib, q_t, 65, table_gallery, _gid_dev(GR.gid_tables()["mod3"], 257), 257, G.EUCLIDEAN, 5, _want(G.EUCLIDEAN, "mod3", 257, 5, 65))
        side.synchronize()


def test_empty_calls(lib, table_gallery, table_queries):
    gid_t = _gid_dev(GR.gid_tables()["div16"], 257)
    st, sbits, idx, grp = _raw(lib, table_queries, None, 0, table_gallery, gid_t, 257, 0, 5)        # n = 0: nothing is done
    assert st == 0 and _untouched(sbits, idx, grp)
    for gid0 in (None, gid_t):                                                                      # m = 0: NaN / -1 / -1; no ids needed
        st, sbits, idx, grp = _raw(lib, table_queries, None, 3, table_gallery, gid0, 0, 0, 5)
        assert st == 0 and _untouched(sbits[[0, -1]], idx[[0, -1]], grp[[0, -1]])
        assert (idx[1:-1] == -1).all() and (grp[1:-1] == -1).all() and np.isnan(sbits[1:-1].view(np.float32)).all()


def test_refusals(lib, table_gallery, table_queries):
    gid = GR.gid_tables()["div16"]
    gid_t = _gid_dev(gid, 257)
    need = lib.trl_gallery_search_groups_workspace(33, 257, 5, 128)
    assert need == (3 * 33 * 5 * 8 + 255) // 256 * 256 + 3 * 33 * 5 * 4

    def refused(ids=gid_t, **kw):
        a = dict(n=33, ld=288, m=257, metric=0, k=5, strip_cols=128, ws_delta=0, ws_offset=0)
        a.update(kw)
        st, sbits, idx, grp = _raw(lib, table_queries, None, a["n"], table_gallery, ids, a["m"], a["metric"], a["k"], a["strip_cols"],
                                   a["ws_delta"], a["ws_offset"], a["ld"])
        assert st == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_search_groups"), (kw, st, lib.trl_last_error())
        assert _untouched(sbits, idx, grp), kw

    refused(ws_delta=-1)                                   # one byte too small
    refused(ws_offset=4)                                   # not 8-byte aligned
    refused(ids=None)                                      # no group ids
    for kw in (dict(metric=2), dict(metric=-1), dict(k=0), dict(k=17), dict(ld=100), dict(ld=256), dict(strip_cols=100), dict(n=-1), dict(m=-1)):
        refused(**kw)
    st, sbits, idx, grp = _raw(lib, table_queries, None, 33, table_gallery, gid_t, 257, 0, 5, 128)    # the same call with its workspace passes
    assert st == 0 and np.array_equal(idx[1:-1], _want(0, "div16", 257, 5, 33)[1])


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_face_gallery_identities(lib):
    from truely_amd.gallery import FaceGallery
    g, q = G.tables()
    labels = [f"p{(7 * r) % 40}" if r % 5 else ("pair", (3 * r) % 11) for r in range(257)]         # strings and tuples, first seen out of order
    ids: dict = {}
    gid = np.array([ids.setdefault(l, len(ids)) for l in labels], np.int32)
    names = list(ids)
    assert 40 <= len(names) < 60 and np.bincount(gid).min() >= 2 and names != sorted(names, key=str)
    q_t = torch.from_numpy(q.copy()).cuda()
    for name, metric in G.METRICS.items():
        gal = FaceGallery(metric=name, capacity=32)
        assert gal.identities == []
        grp, idx, sc = gal.search_identities(q[:2], k=3)                                             # an empty gallery
        assert (grp.cpu().numpy() == -1).all() and (idx.cpu().numpy() == -1).all() and np.isnan(sc.cpu().numpy()).all()
        assert gal.identify_topk(q[:2]) == [[], []]
        gal.add(g[:20], labels[:20])
        assert gal.identities == list(dict.fromkeys(labels[:20]))
        gal.add(torch.from_numpy(g[20:50].copy()).cuda(), labels[20:50])                             # past the capacity of 32: grows, ids copied
        assert gal.ld == 64 and np.array_equal(gal._gid[:50].cpu().numpy(), gid[:50]) and (gal._gid[50:].cpu().numpy() == -1).all()
        gal.add(g[50:257], labels[50:257])
        assert gal.identities == names and gal.labels == labels
        assert gal._gid.dtype == torch.int32 and gal._gid.device.type == "cuda" and gal._gid.shape == (gal.ld,)
        assert np.array_equal(gal._gid[:257].cpu().numpy(), gid) and (gal._gid[257:].cpu().numpy() == -1).all()
        ref = G.table_scores(metric)
        want_sc, want_idx, want_grp = GR.group_topk_ref(ref, gid, metric, 5)
        for cols in (0, 128):
            grp, idx, sc = gal.search_identities(q_t, k=5, max_strip_cols=cols)
            assert grp.dtype == torch.int32 and idx.dtype == torch.int32 and sc.dtype == torch.float32 and grp.device.type == "cuda"
            assert np.array_equal(grp.cpu().numpy(), want_grp) and np.array_equal(idx.cpu().numpy(), want_idx)
            assert G.same_bits(sc.cpu().numpy(), want_sc).all()
        # a gallery mask is folded into the ids as -1; a query mask empties its rows
        gv = np.ones(257, np.uint8); gv[want_idx[:, 0][want_idx[:, 0] >= 0]] = 0                     # every query's best row
        valid = np.ones(65, np.uint8); valid[2] = 0
        m_sc, m_idx, m_grp = GR.group_topk_ref(ref, np.where(gv != 0, gid, -1), metric, 5, valid)
        assert not np.array_equal(m_idx[3:], want_idx[3:])
        grp, idx, sc = gal.search_identities(q_t, k=5, valid=valid, gallery_valid=torch.from_numpy(gv).cuda())
        assert np.array_equal(grp.cpu().numpy(), m_grp) and np.array_equal(idx.cpu().numpy(), m_idx) and G.same_bits(sc.cpu().numpy(), m_sc).all()
        assert (grp[2].cpu().numpy() == -1).all()
        # identify_topk: (label, score) pairs, best first; empty and NaN entries dropped, then those that fail the threshold
        def pairs(sc_, grp_, thr=None):
            out = []
            for r in range(len(sc_)):
                with np.errstate(invalid="ignore"):
                    keep = (grp_[r] >= 0) & ~np.isnan(sc_[r])
                    if thr is not None:
                        keep &= (sc_[r] >= np.float32(thr)) if metric == G.COSINE else (sc_[r] <= np.float32(thr))
                out.append([(names[grp_[r, e]], float(sc_[r, e])) for e in range(sc_.shape[1]) if keep[e]])
            return out
        top = gal.identify_topk(q_t, k=5)
        assert top == pairs(want_sc, want_grp)
        assert top[3] == [] and len(top[8]) == 5 and len({l for l, _s in top[8]}) == 5                # a NaN query; an ordinary one
        thr = 0.5 if metric == G.COSINE else 10.0                                                    # test_gpu_gallery.py's: copies pass, unrelated rows fail
        top_t = gal.identify_topk(q_t, k=5, threshold=thr)
        assert top_t == pairs(want_sc, want_grp, thr) and len(top_t[0]) >= 1 and top_t[0][0][0] == labels[2] and any(len(t) == 0 for t in top_t)
        assert gal.identify_topk(q_t, k=5, valid=valid)[2] == []
        # identify is the first entry of identify_topk(k = 1) wherever that is not empty, and None elsewhere
        who, best = gal.identify(q_t)
        one = gal.identify_topk(q_t, k=1)
        best = best.cpu().numpy()
        for r in range(65):
            if one[r]:
                assert one[r][0][0] == who[r] and np.float32(one[r][0][1]).view(np.uint32) == best[r].view(np.uint32), r
            else:
                assert who[r] is None
        with pytest.raises(ValueError):
            gal.search_identities(q_t, k=17)
        with pytest.raises(ValueError):
            gal.search_identities(q_t, gallery_valid=np.ones(5, np.uint8))
    # add takes any object as a label: unhashable ones are identities by == alone
    gal = FaceGallery(capacity=32)
    gal.add(g[:6], [["a"], ["b"], ["a"], "c", ["b"], "c"])
    assert gal.identities == [["a"], ["b"], "c"] and gal._gid[:6].tolist() == [0, 1, 0, 2, 1, 2]
    assert [l for l, _s in gal.identify_topk(g[4:5], k=3)[0]][0] == ["b"]
