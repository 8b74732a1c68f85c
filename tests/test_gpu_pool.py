"""Embedding templates on the device (csrc/trl_pool.hip, pool.py) against tests/pool_ref.py, bit for bit: every id pattern and weight
set of the reference's tables in both modes and at both tile sizes (the smallest the kernels support, 8, and the default, 32, so
that at 257 rows there are tile edges, a partial tile and groups that cross tiles); the same bits across splits into calls,
permutations, a side stream, n2 given or computed, a row pitch of 520, a 4-byte-aligned row pointer and chunks of groups; outputs
in prefilled buffers with a guard slot on either side; the representative against the reference and against FaceGallery.scores;
FaceGallery.templates and FaceTracker(templates=True) on top."""
import ctypes as C

import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import _lib
import gallery_ref as G
import pool_ref as P
import track_ref as T

pytestmark = pytest.mark.gpu
F32 = np.float32
TILES = (8, 0)                           # the smallest supported tile and the default
MODES = ((True, P.UNIT), (False, P.MEAN))
FILL_F, FILL_I = -7.25, -0x5A5A5A5B


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _lib.load()


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(x):
    return None if x is None else torch.from_numpy(np.array(x, order="C")).cuda()


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, F32).view(np.uint32)


def assert_same(got: dict, ref: dict, what=""):
    assert np.array_equal(got["count"].cpu().numpy(), ref["count"]), what
    assert int(got["skipped"]) == ref["skipped"], what
    for name in ("weight", "cohesion", "template"):
        assert G.same_bits(got[name].cpu().numpy(), ref[name]).all(), (what, name)
        assert got[name].dtype == torch.float32


def _table(ids, weights, m=P.M):
    gid, G_ = P.gid_tables()[ids]
    w = P.weight_tables()[weights]
    return G.tables()[0][:m], gid[:m], None if w is None else w[:m], G_


@pytest.mark.parametrize("weights", tuple(P.weight_tables()))
@pytest.mark.parametrize("ids", tuple(P.gid_tables()))
def test_tables_equal_reference(lib, ids, weights):
    x, gid, w, G_ = _table(ids, weights)
    dx, dg, dw = _t(x), _t(gid), _t(w)
    for unit, mode in MODES:
        ref = P.table_ref(ids, weights, mode)
        for tile in TILES:
            assert_same(truely_amd.pool_embeddings(dx, dg, G_, dw, unit=unit, tile_rows=tile), ref, (ids, weights, mode, tile))
            p = truely_amd.EmbeddingPool(G_)
            p.add(dx, dg, dw, tile_rows=tile)
            assert_same(p.result(unit), ref, (ids, weights, mode, tile, "pool"))
    if ids == "distinct":                                                            # num_groups read back from the ids
        assert_same(truely_amd.pool_embeddings(dx, dg, None, dw), P.table_ref(ids, weights, P.UNIT))


def _guarded(shape, dtype, fill):
    """A prefilled buffer with one guard slot (a row for the template) on either side of `shape`."""
    full = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return full, full[1:1 + shape[0]]


def _guards_intact(full, fill):
    return bool((full[0] == fill).all() and (full[-1] == fill).all())


@pytest.mark.parametrize("G_", (1, 3, 17, 257))
@pytest.mark.parametrize("m", (0, 1, 31, 33, 257))
def test_shapes_through_the_abi_with_guards(lib, m, G_):
    """trl_pool_* called directly at every (m, G): ids i * 7 % (G + 1) - so one id in G + 1 lies outside -, random weights, outputs
    in prefilled buffers: nothing beyond [G] / [G][512] is written, and what is written equals the reference."""
    x = G.tables()[0][:m]
    gid = (np.arange(m, dtype=np.int32) * 7 % (G_ + 1)).astype(np.int32)
    w = P.weight_tables()["random"][:m]
    dx, dg, dw = _t(x), _t(gid), _t(w)
    s = _stream()
    refs = {mode: P.pool_ref(x, gid, w, G_, mode, n2=G.table_n2()[:m]) for _unit, mode in MODES}
    tmpl = _t(refs[P.UNIT]["template"])
    want_i, want_s = P.representative_ref(x, gid, w, refs[P.UNIT]["template"], G.table_n2()[:m])
    for tile in TILES:
        state = torch.full((lib.trl_pool_state_bytes(G_) // 8 + 2,), FILL_I, dtype=torch.int64, device="cuda")
        assert lib.trl_pool_reset(_ptr(state[1:]), G_, s) == 0
        if m:
            assert lib.trl_pool_add(_ptr(state[1:]), G_, 0, _ptr(dx), 512, None, _ptr(dg), _ptr(dw), m, tile, s) == 0
        assert state[0].item() == FILL_I and state[-1].item() == FILL_I
        for unit, mode in MODES:
            ref = refs[mode]
            bufs = {"template": _guarded((G_, 512), torch.float32, FILL_F), "count": _guarded((G_,), torch.int32, FILL_I),
                    "weight": _guarded((G_,), torch.float32, FILL_F), "cohesion": _guarded((G_,), torch.float32, FILL_F),
                    "skipped": _guarded((1,), torch.int64, FILL_I)}
            assert lib.trl_pool_finish(_ptr(state[1:]), G_, mode, *[_ptr(bufs[k][1]) for k in ("template", "count", "weight", "cohesion",
                                                                                             "skipped")], s) == 0
            assert all(_guards_intact(bufs[k][0], FILL_I if bufs[k][0].dtype != torch.float32 else FILL_F) for k in bufs), (m, G_, tile)
            got = {k: v[1] for k, v in bufs.items()}
            got["skipped"] = got["skipped"][0]
            assert_same(got, ref, (m, G_, tile, mode))
        # the representative's buffers
        key = torch.full((G_ + 2,), FILL_I, dtype=torch.int64, device="cuda")
        index, score = _guarded((G_,), torch.int32, FILL_I), _guarded((G_,), torch.float32, FILL_F)
        assert lib.trl_pool_rep_reset(_ptr(key[1:]), G_, s) == 0
        if m:
            assert lib.trl_pool_rep_add(_ptr(key[1:]), G_, 0, _ptr(tmpl), _ptr(dx), 512, None, _ptr(dg), _ptr(dw), 0, m, tile, s) == 0
        assert lib.trl_pool_rep_finish(_ptr(key[1:]), G_, _ptr(index[1]), _ptr(score[1]), s) == 0
        assert key[0].item() == FILL_I and key[-1].item() == FILL_I
        assert _guards_intact(index[0], FILL_I) and _guards_intact(score[0], FILL_F)
        assert np.array_equal(index[1].cpu().numpy(), want_i) and G.same_bits(score[1].cpu().numpy(), want_s).all(), (m, G_, tile)


@pytest.mark.parametrize("ids,weights", (("runs", "edge"), ("outside", "random"), ("one", "none"), ("div16", "edge")))
def test_same_bits_however_the_rows_arrive(lib, ids, weights):
    x, gid, w, G_ = _table(ids, weights)
    ref = P.table_ref(ids, weights, P.UNIT)
    dx, dg, dw = _t(x), _t(gid), _t(w)
    pool = lambda: truely_amd.EmbeddingPool(G_)
    sl = lambda v, a, b: None if v is None else v[a:b]
    for tile in TILES:
        for step in (1, 32, 100):                                                     # adds of 1, 32 and 100 rows
            if step == 1 and tile == 0:
                continue
            p = pool()
            for a in range(0, P.M, step):
                p.add(dx[a:a + step], dg[a:a + step], sl(dw, a, a + step), tile_rows=tile)
            assert_same(p.result(), ref, (ids, tile, step))
        perm = torch.from_numpy(np.random.default_rng(3).permutation(P.M)).cuda()     # rows permuted
        p = pool()
        p.add(dx[perm], dg[perm], None if dw is None else dw[perm], tile_rows=tile)
        assert_same(p.result(), ref, (ids, tile, "perm"))
        side = torch.cuda.Stream()                                                    # a non-default stream
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            p = pool()
            p.add(dx, dg, dw, tile_rows=tile)
            r = p.result()
        side.synchronize()
        assert_same(r, ref, (ids, tile, "stream"))
        g = truely_amd.FaceGallery(capacity=P.M)                                      # n2 given: the gallery's own
        g.add(dx, range(P.M))
        p = pool()
        p.add(dx, dg, dw, n2=g._n2[:P.M], tile_rows=tile)
        assert_same(p.result(), ref, (ids, tile, "n2"))
        wide = torch.full((P.M, 520), 3.0, dtype=torch.float32, device="cuda")       # ld_rows 520
        wide[:, :512].copy_(dx)
        p = pool()
        p.add(wide[:, :512], dg, dw, tile_rows=tile)
        assert wide[:, :512].stride(0) == 520
        assert_same(p.result(), ref, (ids, tile, "ld"))
        big = torch.zeros(P.M * 512 + 8, dtype=torch.float32, device="cuda")          # a 4-byte-aligned row pointer
        off = big[1:1 + P.M * 512].view(P.M, 512)
        off.copy_(dx)
        assert off.data_ptr() % 8 == 4
        p = pool()
        p.add(off, dg, dw, tile_rows=tile)
        assert_same(p.result(), ref, (ids, tile, "align"))
        for nbytes in (1, 8 + 2 * 514 * 8, 8 + 5 * 514 * 8 + 100):                    # chunks of 1, 2 and 5 groups
            assert_same(truely_amd.pool_embeddings(dx, dg, G_, dw, max_state_bytes=nbytes, tile_rows=tile), ref, (ids, tile, nbytes))
    small = truely_amd.EmbeddingPool(1)                                               # grow keeps the sums; reset forgets them
    small.add(dx[:100], dg[:100], sl(dw, 0, 100))
    small.grow(G_)
    small.add(dx[100:], dg[100:], sl(dw, 100, P.M))
    if G_ > 1:                                                                        # (rows of groups >= 1 were ignored by the pool of 1)
        sub = P.finish(P.accumulate(P.accumulate(P.empty_state(G_), x[:100], np.where(gid[:100] == 0, 0, -1), sl(w, 0, 100)),
                                    x[100:], gid[100:], sl(w, 100, P.M)))
        assert_same(small.result(), sub, (ids, "grow"))
    else:
        assert_same(small.result(), ref, (ids, "grow"))
    small.reset()
    small.add(dx, dg, dw)
    assert_same(small.result(), ref, (ids, "reset"))


@pytest.mark.parametrize("ids,weights", (("dups", "none"), ("div16", "edge"), ("outside", "random"), ("one", "none"), ("runs", "random")))
def test_representative(lib, ids, weights):
    x, gid, w, G_ = _table(ids, weights)
    dx, dg, dw = _t(x), _t(gid), _t(w)
    gal = truely_amd.FaceGallery(capacity=P.M)
    gal.add(dx, range(P.M))
    for unit, mode in MODES:
        tmpl = P.table_ref(ids, weights, mode)["template"]
        want_i, want_s = P.representative_ref(x, gid, w, tmpl, G.table_n2())
        for tile in TILES:
            for nbytes in (256 << 20, 8 + 3 * 514 * 8):
                r = truely_amd.pool_embeddings(dx, dg, G_, dw, unit=unit, representative=True, tile_rows=tile, max_state_bytes=nbytes)
                assert r["representative"].dtype == torch.int32 and r["rep_score"].dtype == torch.float32
                assert np.array_equal(r["representative"].cpu().numpy(), want_i), (ids, mode, tile, nbytes)
                assert G.same_bits(r["rep_score"].cpu().numpy(), want_s).all(), (ids, mode, tile, nbytes)
        s = gal.scores(r["template"]).cpu().numpy()                                   # rep_score IS FaceGallery.scores(template)[g, rep[g]]
        rep, sc = r["representative"].cpu().numpy(), r["rep_score"].cpu().numpy()
        for g in range(G_):
            assert np.isnan(sc[g]) if rep[g] < 0 else G.same_bits(sc[g:g + 1], s[g, rep[g]:rep[g] + 1]).all(), (ids, mode, g)
    if ids == "dups":
        assert rep.tolist()[1:] == [G.DUPS[0], -1, -1]                                # five tied copies: the lowest; no rows; only NaN rows
    # the rows in several calls with their row0, out of order
    p = truely_amd.EmbeddingPool(G_)
    p.add(dx, dg, dw)
    t = p.result()["template"]
    blocks = lambda: iter([(133, dx[133:], None), (0, dx[:33], None), (33, dx[33:133], gal._n2[33:133])])
    index, score = p._representatives(t, blocks, dg, dw)
    want_i, want_s = P.representative_ref(x, gid, w, P.table_ref(ids, weights, P.UNIT)["template"], G.table_n2())
    assert np.array_equal(index.cpu().numpy(), want_i) and G.same_bits(score.cpu().numpy(), want_s).all()


def test_representative_zero_signs_and_nan_template(lib):
    """Cosines -0, +0, -0 against a given template row: they tie as floats, the lowest row wins and its own bits (-0) come back;
    a NaN template row leaves its group without a representative."""
    gz, qz = G.zero_sign_rows()
    rows = np.concatenate([gz[[2, 0, 4]], gz[[5]]])
    gid = np.array([0, 0, 0, 1], np.int32)
    tmpl = np.concatenate([qz, np.full((1, 512), np.nan, F32)])
    s = _stream()
    for tile in TILES:
        key = torch.empty((2,), dtype=torch.int64, device="cuda")
        index = torch.empty((2,), dtype=torch.int32, device="cuda")
        score = torch.empty((2,), dtype=torch.float32, device="cuda")
        assert lib.trl_pool_rep_reset(_ptr(key), 2, s) == 0
        assert lib.trl_pool_rep_add(_ptr(key), 2, 0, _ptr(_t(tmpl)), _ptr(_t(rows)), 512, None, _ptr(_t(gid)), None, 10, 4, tile, s) == 0
        assert lib.trl_pool_rep_finish(_ptr(key), 2, _ptr(index), _ptr(score), s) == 0
        want_i, want_s = P.representative_ref(rows, gid, None, tmpl)
        assert want_i.tolist() == [0, -1] and np.signbit(want_s[0]) and want_s[0] == 0
        assert index.cpu().numpy().tolist() == [10, -1]                               # (row0 = 10)
        assert G.same_bits(score.cpu().numpy(), want_s).all()


def _sphere_bound():
    """|cohesion - 1| for a group of ONE row: t = p, the row's quantised unit vector.  With e = rel + u + sqrt(512) 2^-33 (pool_ref.
    sum_bound per element, in the 2-norm: |t - v| <= |v| rel + sqrt(512) 2^-33 + u |t|, |v| = 1), | |t| - 1 | <= e; the chain that
    takes n2(t) is within gamma_512, its square root within gamma_512 / 2 and one rounding; Wf = 1 exactly."""
    g = G.gamma(512)
    rel = (1 + P.U) ** 2 / (np.sqrt(1 - g) * (1 - P.U)) - 1
    e = rel + P.U + np.sqrt(512.0) * 2.0 ** -33
    return (1 + e) * np.sqrt(1 + g) * (1 + P.U) - 1


def test_gallery_templates(lib):
    x, gid, _w, G_ = _table("div16", "none")
    gal = truely_amd.FaceGallery(capacity=64)                                         # (grows twice)
    labels = [f"person{int(g)}" for g in gid]
    for a, b in ((0, 40), (40, 200), (200, P.M)):
        gal.add(_t(x[a:b]), labels[a:b])
    for unit, mode in MODES:
        tg, info = gal.templates(unit=unit, representative=True)
        ref = P.table_ref("div16", "none", mode)
        assert_same(info, ref, mode)
        assert tg.labels == gal.identities == [f"person{g}" for g in range(G_)] and tg.metric == gal.metric and len(tg) == G_
        assert G.same_bits(tg.rows().cpu().numpy(), ref["template"]).all()
        want_i, want_s = P.representative_ref(x, gid, None, ref["template"], G.table_n2())
        assert np.array_equal(info["representative"].cpu().numpy(), want_i) and G.same_bits(info["rep_score"].cpu().numpy(), want_s).all()
    assert np.array_equal(gal.representatives().cpu().numpy(), P.representative_ref(x, gid, None, P.table_ref("div16", "none", P.UNIT)["template"])[0])
    # weights, and gallery_valid masking rows (a whole identity among them: it is not enrolled)
    w = P.weight_tables()["edge"]
    valid = np.ones(P.M, np.uint8)
    valid[[0, 5, 17, 100, 256]] = 0
    valid[32:48] = 0
    tg, info = gal.templates(weights=_t(w), gallery_valid=_t(valid))
    ref = P.pool_ref(x, np.where(valid != 0, gid, -1), w, G_, n2=G.table_n2())
    assert_same(info, ref, "valid")
    assert ref["count"][2] == 0 and ref["count"][16] == 0 and tg.labels == [f"person{g}" for g in range(G_) if g not in (2, 16)]
    assert G.same_bits(tg.rows().cpu().numpy(), ref["template"][ref["count"] > 0]).all()
    # one L2-normalised row per label: every template is its row, cohesion 1 within the bound
    rows = x[16:31]
    one = truely_amd.FaceGallery()
    one.add(_t(rows), range(15))
    tg, info = one.templates()
    coh = info["cohesion"].cpu().numpy().astype(np.float64)
    assert (info["count"].cpu().numpy() == 1).all() and (np.abs(coh - 1) <= _sphere_bound()).all(), np.abs(coh - 1).max()
    assert np.abs(tg.rows().cpu().numpy().astype(np.float64) - rows).max() < 1e-6


def test_identify_on_the_template_gallery(lib):
    """Six people, five noisy rows each, enrolled row by row; the template gallery names each enrolled row's own identity -- on rows
    built so that the reference does (its margins are asserted first)."""
    rng = np.random.default_rng(99)
    bases = rng.standard_normal((6, 512))
    person = np.repeat(np.arange(6), 5)[rng.permutation(30)]
    rows = (bases[person] + 0.6 * rng.standard_normal((30, 512))).astype(F32) * F32(3.0)
    ref = P.pool_ref(rows, person, None, 6)
    s = G.scores_ref(rows, ref["template"], G.COSINE)
    assert (s.argmax(axis=1) == person).all() and (np.sort(s, axis=1)[:, -1] - np.sort(s, axis=1)[:, -2]).min() > 0.3
    gal = truely_amd.FaceGallery()
    names = ["ann", "bob", "cy", "dee", "eve", "flo"]
    gal.add(_t(rows), [names[k] for k in person])
    tg, info = gal.templates()
    order = [names.index(n) for n in gal.identities]
    assert_same(info, {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in ref.items()})
    who, score = tg.identify(_t(rows), threshold=0.5)
    assert who == [names[k] for k in person]
    assert G.same_bits(score.cpu().numpy(), s[np.arange(30), person]).all()


def _windows(trk, clip, cuts, weights=None):
    counts = np.asarray(clip["counts"], np.int32)
    n = len(counts)
    rows = np.concatenate([[0], np.cumsum(counts)])
    cuts = sorted({0, n, *cuts})
    db, dc, de, dw = _t(clip["boxes"]), _t(counts), _t(clip["emb"]), _t(weights)
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ra, rb = int(rows[a]), int(rows[b])
        args = (db[ra:rb], dc[a:b], de[ra:rb]) + (() if weights is None else (dw[ra:rb],))
        outs.append(trk.update(*args))
    return {k: torch.cat([o[k] for o in outs]) for k in ("track", "sim", "flag")}


@pytest.mark.parametrize("name,cuts", (("dense8", ()), ("dense8", (1, 8, 9, 20)), ("dense_crowd", (2,)), ("dense_crowd", (1, 2, 3, 4)),
                                       ("dense_drift", (13, 27))))
def test_tracker_templates(lib, name, cuts):
    clip = T.dense_clip(name)
    ref = T.dense_ref(name)
    rules = (clip["iou_min"], clip["sim_min"], clip["max_age"])
    plain = _windows(truely_amd.FaceTracker(*rules), clip, cuts)
    trk = truely_amd.FaceTracker(*rules, templates=True)
    w = (1.0 - np.random.default_rng(4).random(len(clip["emb"]))).astype(F32) if name == "dense_drift" else None
    got = _windows(trk, clip, cuts, w)
    for k in ("track", "sim", "flag"):                                               # the flag changes nothing the tracker gives today
        assert torch.equal(got[k], plain[k]) and np.array_equal(_bits(got[k]) if k == "sim" else got[k].cpu().numpy(),
                                                                _bits(ref[k]) if k == "sim" else ref[k]), (name, k)
    n = ref["tracker"].next_id
    t = trk.templates()
    assert t["template"].shape == (n, 512) and trk._pool.num_groups == trk._table.shape[0] > 256 * (name == "dense_crowd")
    whole = truely_amd.pool_embeddings(_t(clip["emb"]), got["track"], n, _t(w))
    for k in ("template", "weight", "cohesion"):
        assert np.array_equal(_bits(t[k]), _bits(whole[k])), (name, k)
    assert torch.equal(t["count"], whole["count"]) and int(t["skipped"]) == int(whole["skipped"])
    assert_same(t, P.pool_ref(clip["emb"], ref["track"], w, n), name)
    with pytest.raises(ValueError):
        trk.update(_t(clip["boxes"][:1]), _t(np.array([1], np.int32)))               # templates need the embeddings
    with pytest.raises(ValueError):
        truely_amd.FaceTracker(*rules).templates()
    trk.reset()
    assert_same(trk.templates(), P.pool_ref(np.zeros((0, 512), F32), np.zeros(0, np.int32), None, 0), "reset")


def test_identify_tracks_names_two_people(lib):
    rng = np.random.default_rng(5)
    bases = rng.standard_normal((3, 512))
    frames = []
    for t in range(9):
        people = [0, 1] if t % 2 else [1, 0]
        frames.append([(T.person_boxes(k), (bases[k] + 0.5 * rng.standard_normal(512)).astype(F32)) for k in people])
    clip = T.make_clip(frames, iou_min=0.1, sim_min=0.3, max_age=3)
    gal = truely_amd.FaceGallery()
    gal.add(_t(bases.astype(F32)), ["ann", "bob", "cy"])
    trk = truely_amd.FaceTracker(0.1, 0.3, 3, templates=True)
    got = _windows(trk, clip, (4,))
    assert got["track"].cpu().numpy().tolist() == [0, 1, 1, 0] * 4 + [0, 1]          # track 0 is person 1
    who, score = trk.identify_tracks(gal, threshold=0.5)
    assert who == ["bob", "ann"] and bool((score > 0.8).all())
    t = trk.templates()
    assert t["count"].cpu().numpy().tolist() == [9, 9] and bool(((t["cohesion"] > 0.7) & (t["cohesion"] < 0.95)).all())
    assert trk.identify_tracks(gal, threshold=0.999)[0] == [None, None]


@pytest.mark.parametrize("groups", (1, 255, 256, 257))
def test_key_read_back_is_one_kernel_for_both_entries(lib, groups):
    """trl_pool_rep_finish and trl_best_read decode the same array of keys (csrc/trl_bestkey.h; the reference is
    tests/quality_ref.py's best_key) to the reference's rows and the scores' own bits -- -0.0 stays -0.0, an empty slot is row -1
    and NaN -- and to the same bits as each other, at the edges of a 256-thread workgroup."""
    import quality_ref as Q
    scores = [-np.inf, -1.0, -0.0, 0.0, 1e-42, 1.0, np.inf]
    cases = [(F32(s), row) for s in scores for row in (0, 2 ** 31 - 2)] + [(F32(0.5), 7), (F32(0.5), 8), None]      # (None: an empty slot)
    cases = [cases[(i + 2 * 2 + 1) % len(cases)] for i in range(groups)]                # (one group: -0.0 at row 2^31 - 2)
    keys = np.array([0 if c is None else Q.best_key(*c) for c in cases], np.uint64)
    want_row = np.array([-1 if c is None else c[1] for c in cases], np.int32)
    want_score = np.array([np.nan if c is None else c[0] for c in cases], F32)
    assert groups > 1 or (np.signbit(want_score[0]) and want_score[0] == 0 and want_row[0] == 2 ** 31 - 2)
    d_keys = torch.from_numpy(keys.view(np.int64)).cuda()
    got = []
    for entry in (lib.trl_pool_rep_finish, lib.trl_best_read):
        row = torch.full((groups,), FILL_I, dtype=torch.int32, device="cuda")
        score = torch.full((groups,), FILL_F, dtype=torch.float32, device="cuda")
        _lib.check(entry(_ptr(d_keys), groups, _ptr(row), _ptr(score), _stream()))
        got.append((row.cpu().numpy(), score.cpu().numpy()))
        assert np.array_equal(got[-1][0], want_row)
        empty = want_row < 0
        assert np.isnan(got[-1][1][empty]).all() and np.array_equal(_bits(got[-1][1])[~empty], _bits(want_score)[~empty])
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert np.array_equal(d_keys.cpu().numpy().view(np.uint64), keys)                   # (the keys are read, not written)
