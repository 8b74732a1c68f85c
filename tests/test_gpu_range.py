"""The gallery range search on the device (trl_gallery_range_count / trl_gallery_range_fill, csrc/trl_gallery.hip) against
tests/range_ref.py, bit for bit: np.array_equal on offsets and indices, same_bits on scores; the refusals; the clustering's link
bitmap as a second witness; gallery.py on top.

The kernels have k_gallery_links' frame (row tiles of 32, slabs of 32 columns, 128 columns per group, strips of groups) and every
wave walks a contiguous quarter of its strip, so the table is sliced to n and m on both sides of 32, 128 and the strip edges, and
every shape runs with default strips (one group each here), 128- and 256-column strips (two slabs per wave).  Outputs lie in
sentinel-filled buffers with slack on both sides; the workspace is exactly the size asked for, with a guard behind it; rows
and columns lying behind n and m in memory are other rows' -- not zeros."""
import ctypes as C_
import functools

import numpy as np
import pytest
import torch

from truely_amd import _lib
import cluster_ref as CR
import gallery_ref as G
import range_ref as R

pytestmark = pytest.mark.gpu

SLACK = 8
FILL64 = -0x5A5A5A5A5A5A5A5B
FILL32 = -0x5A5A5A5B
WS_GUARD = 256
TRL_ERR_INVALID = -1
STRIPS = (0, 128, 256)
THRESHOLDS = {m: CR.TABLE_THR[m] + (R.LOOSE_THR[m],) for m in (G.COSINE, G.EUCLIDEAN)}
EDGE_SHAPES = ((1, 1), (1, 257), (31, 31), (31, 32), (32, 33), (33, 127), (33, 128), (64, 129), (64, 256), (65, 31), (32, 257), (65, 33))
GINVALID = (0, 31, 32, 100, 127, 128, 129, 255, 256)      # columns on both sides of the 32-, 128- and 256-column edges


def _ptr(t):
    return C_.c_void_p(t.data_ptr() if t is not None else 0)


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


def _pack(lib, rows_t, m, ld):
    mat = torch.zeros((G.K, ld), dtype=torch.float32, device="cuda")
    n2 = torch.zeros((ld,), dtype=torch.float32, device="cuda")
    st = lib.trl_gallery_pack(_ptr(rows_t), m, _ptr(mat), ld, _ptr(n2), 0, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.trl_last_error()
    return mat, n2


@pytest.fixture(scope="module")
def table(lib):
    """The gallery table's 257 rows and the 65 query rows on the device (the queries also at a 4-byte aligned address), the gallery
    packed at ld = 288."""
    g, q = G.tables()
    rows = _dev(g)
    mat, n2 = _pack(lib, rows, 257, 288)
    return dict(g=rows, q=_dev(q), q4=_dev(q, True), mat=mat, n2=n2, ld=288)


def _mask_t(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.uint8)).cuda()


class Call:
    """One range search through the C ABI.  count() and fill() take overrides of single arguments (the refusal tests); the buffers
    are sized by the arguments given here."""

    def __init__(self, lib, t, q_t, n, m, metric, thr, self_=0, qvalid=None, gvalid=None, strip_cols=0, room=0):
        self.lib = lib
        self.a = dict(q=q_t, qvalid=_mask_t(qvalid), n=n, mat=t["mat"], ld=t["ld"], n2=t["n2"], gvalid=_mask_t(gvalid), m=m, metric=metric,
                      thr=float(np.float32(thr)), self_=self_, strip_cols=strip_cols)
        self.n = n
        self.offsets = torch.full((max(n, 0) + 1 + 2 * SLACK,), FILL64, dtype=torch.int64, device="cuda")
        self.need = lib.trl_gallery_range_workspace(n, m, strip_cols)
        self.ws = torch.full((self.need + 8 + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.room = room
        self.index = self.score = None

    def _common(self, a):
        return (_ptr(a["q"]), _ptr(a["qvalid"]), a["n"], _ptr(a["mat"]), a["ld"], _ptr(a["n2"]), _ptr(a["gvalid"]), a["m"], a["metric"],
                a["thr"], a["self_"])

    def _ws(self, ws_delta, ws_offset):
        size = max(self.need + ws_delta, 0)
        return C_.c_void_p(self.ws.data_ptr() + ws_offset if size else 0), size

    def count(self, ws_delta=0, ws_offset=0, null=(), stream=None, **over):
        a = dict(self.a, offsets=self.offsets[SLACK:])
        a.update(over)
        a.update({k: None for k in null})
        ws, size = self._ws(ws_delta, ws_offset)
        s = C_.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        st = self.lib.trl_gallery_range_count(*self._common(a), _ptr(a["offsets"]), ws, size, a["strip_cols"], s)
        torch.cuda.synchronize()
        return st

    def total(self):
        return int(self.offsets[SLACK + self.n].item())

    def fill(self, capacity, ws_delta=0, ws_offset=0, null=(), stream=None, **over):
        if self.index is None:
            entries = max(self.total(), capacity, 0) + self.room + 2 * SLACK
            self.index = torch.full((entries,), FILL32, dtype=torch.int32, device="cuda")
            self.score = torch.full((entries,), FILL32, dtype=torch.int32, device="cuda")      # (float32 entries, kept as their bits)
        a = dict(self.a, offsets=self.offsets[SLACK:], index=self.index[SLACK:], score=self.score[SLACK:])
        a.update(over)
        a.update({k: None for k in null})
        ws, size = self._ws(ws_delta, ws_offset)
        s = C_.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
        st = self.lib.trl_gallery_range_fill(*self._common(a), _ptr(a["offsets"]), ws, size, capacity, _ptr(a["index"]), _ptr(a["score"]),
                                             a["strip_cols"], s)
        torch.cuda.synchronize()
        return st

    def untouched_around(self):
        """The slack in front of and behind every array, and the guard behind the workspace."""
        off = self.offsets.cpu().numpy()
        assert (off[:SLACK] == FILL64).all() and (off[SLACK + self.n + 1:] == FILL64).all(), "written beside the offsets"
        assert (self.ws[self.need:] == 0xA5).all().item(), "written behind the workspace"
        if self.index is not None:
            for x in (self.index, self.score):
                assert (x[:SLACK] == FILL32).all().item() and (x[-SLACK:] == FILL32).all().item(), "written beside the lists"

    def outputs_are_sentinels(self):
        assert (self.offsets == FILL64).all().item() and (self.ws == 0xA5).all().item()
        if self.index is not None:
            assert (self.index == FILL32).all().item() and (self.score == FILL32).all().item()

    def result(self, capacity):
        """(offsets, the first min(capacity, total) entries of index and score); everything at or past them must be the sentinel."""
        self.untouched_around()
        off = self.offsets[SLACK:SLACK + self.n + 1].cpu().numpy()
        kept = min(capacity, self.total())
        idx, sc = self.index[SLACK:].cpu().numpy(), self.score[SLACK:].cpu().numpy()
        assert (idx[kept:] == FILL32).all() and (sc[kept:] == FILL32).all(), "written at or past the capacity"
        return off, idx[:kept], sc[:kept].view(np.float32)


def _same(got, want, kept=None, what=()):
    off, idx, sc = got
    woff, widx, wsc = want
    kept = len(widx) if kept is None else kept
    assert off.dtype == np.int64 and np.array_equal(off, woff), (what, np.nonzero(off != woff)[0][:4])
    assert len(idx) == kept and np.array_equal(idx, widx[:kept]), what
    assert R.same_bits(sc, wsc[:kept]).all(), what


def _search(lib, t, q_t, n, m, metric, thr, want, what, capacity=None, **kw):
    c = Call(lib, t, q_t, n, m, metric, thr, room=5, **kw)
    assert c.count() == 0, lib.trl_last_error()
    assert c.total() == want[0][-1], (what, c.total(), int(want[0][-1]))
    cap = c.total() if capacity is None else capacity
    assert c.fill(cap) == 0, lib.trl_last_error()
    _same(c.result(cap), want, min(cap, c.total()), what)
    return c


@functools.lru_cache(maxsize=None)
def _want(metric, thr, n, m, qinvalid=None, ginvalid=None):
    qv = None if qinvalid is None else CR.mask(n, qinvalid)
    gv = None if ginvalid is None else CR.mask(m, ginvalid)
    return R.range_ref(G.table_scores(metric)[:n, :m], metric, thr, qv, gv), qv, gv


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_shared_table(lib, table, metric):
    """65 queries against 257 rows at the clustering's thresholds and one that nearly every pair passes: empty rows, rows across
    several slabs and all three 128-column groups, full slabs; the same bytes whatever the strips."""
    for thr in THRESHOLDS[metric]:
        want, _qv, _gv = _want(metric, thr, 65, 257)
        per_row = np.diff(want[0])
        assert want[0][-1] > 150 and per_row.max() > 32 and (thr in R.LOOSE_THR.values() or (per_row == 0).any())
        for strip_cols in STRIPS:
            _search(lib, table, table["q"], 65, 257, metric, thr, want, (metric, thr, strip_cols), strip_cols=strip_cols)


def _duplicated_scores(metric):
    """Finite scores of the 65 x 257 table that occur more than once, ascending."""
    s = G.table_scores(metric)
    v, c = np.unique(s[np.isfinite(s)], return_counts=True)
    return v[c > 1]


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_thresholds_equal_to_scores(lib, table, metric):
    """The match is inclusive: at a threshold equal to a duplicated score every pair with that score is in, one ulp tighter exactly
    those pairs are out."""
    s = G.table_scores(metric)
    dup = _duplicated_scores(metric)
    assert len(dup) >= 3
    tighter = np.float32(np.inf) if metric == G.COSINE else np.float32(-np.inf)
    for x in (dup[0], dup[len(dup) // 2], dup[-1]):
        at = R.range_ref(s, metric, x)
        off = R.range_ref(s, metric, np.nextafter(x, tighter))
        assert at[0][-1] - off[0][-1] == (s == x).sum() >= 2
        for thr, want in ((x, at), (np.nextafter(x, tighter), off)):
            for strip_cols in (0, 256):
                _search(lib, table, table["q"], 65, 257, metric, thr, want, (metric, float(thr), strip_cols), strip_cols=strip_cols)


def test_zero_signs_nan_and_inf(lib, table):
    """+0 and -0 are one threshold and one score; NaN and zero rows never match; the subnormal row's +-inf cosines follow the plain
    comparison."""
    g, q = G.zero_sign_rows()
    t = dict(ld=32)
    t["mat"], t["n2"] = _pack(lib, _dev(g), 6, 32)
    s = G.scores_ref(q, g, G.COSINE)
    assert np.signbit(s[0, 2]) and s[0, 2] == 0 and not np.signbit(s[0, 0]) and s[0, 0] == 0
    lists = []
    for thr in (0.0, -0.0):
        want = R.range_ref(s, G.COSINE, thr)
        assert want[1].tolist() == [0, 2, 3, 4, 5]
        c = _search(lib, t, _dev(q), 1, 6, G.COSINE, thr, want, ("zero", thr))
        lists.append(c.result(c.total()))
    assert np.array_equal(lists[0][1], lists[1][1]) and R.same_bits(lists[0][2], lists[1][2]).all()
    for metric in (G.COSINE, G.EUCLIDEAN):
        s = G.table_scores(metric)
        want, _qv, _gv = _want(metric, R.LOOSE_THR[metric], 65, 257)
        hit = R.unpack(want[0], want[1], 65, 257)
        assert np.isnan(s).any() and not (hit & np.isnan(s)).any()            # (the device equals `want`: test_shared_table)
        if metric == G.COSINE:
            assert not hit[1].any() and not hit[:, G.ZERO_G].any()            # a zero row's cosines are NaN
            assert np.isinf(s).any()
            for thr in (3e38, -3e38):                                         # +inf >= 3e38; -inf >= -3e38 is false
                w = R.range_ref(s, metric, thr)
                assert thr < 0 or (0 < w[0][-1] == (s == np.inf).sum())
                _search(lib, table, table["q"], 65, 257, metric, thr, w, ("inf", thr))


@pytest.mark.parametrize("n,m", EDGE_SHAPES)
def test_edges_of_the_tiling(lib, table, n, m):
    for metric in (G.COSINE, G.EUCLIDEAN):
        for thr in (CR.TABLE_THR[metric][0], R.LOOSE_THR[metric]):
            want, _qv, _gv = _want(metric, thr, n, m)
            for strip_cols in (0, 128):
                _search(lib, table, table["q"], n, m, metric, thr, want, (n, m, metric, thr, strip_cols), strip_cols=strip_cols)


def test_empty_problems(lib, table):
    for n, m, null in ((65, 0, ()), (65, 0, ("q",)), (0, 257, ()), (0, 0, ()), (0, 257, ("q", "offsets"))):
        assert lib.trl_gallery_range_workspace(n, m, 0) == 0
        c = Call(lib, table, table["q"], n, m, G.COSINE, 0.5)
        assert c.count(null=null) == 0, lib.trl_last_error()
        off = c.offsets.cpu().numpy()
        if n == 0:
            assert (off == FILL64).all()                                      # nothing is done
        else:
            assert (off[SLACK:SLACK + n + 1] == 0).all()
            c.untouched_around()
        assert c.fill(0, null=null) == 0 and c.fill(4, null=null) == 0, lib.trl_last_error()
        assert (c.index == FILL32).all().item() and (c.score == FILL32).all().item()


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_masks(lib, table, metric):
    """Invalid query rows on both sides of the 32-row tile edge, invalid gallery columns on both sides of the 32-, 128- and
    256-column edges, and both."""
    thr = R.LOOSE_THR[metric]
    for qi, gi in ((CR.INVALID, None), (None, GINVALID), (CR.INVALID, GINVALID)):
        for t in (thr, CR.TABLE_THR[metric][0]):
            want, qv, gv = _want(metric, t, 65, 257, qi, gi)
            if qv is not None:
                assert all(want[0][r + 1] == want[0][r] for r in CR.INVALID if r < 65)
            if gv is not None:
                assert not np.isin(want[1], GINVALID).any()
            for strip_cols in STRIPS:
                _search(lib, table, table["q"], 65, 257, metric, t, want, (metric, t, qi, gi, strip_cols), qvalid=qv, gvalid=gv,
                        strip_cols=strip_cols)
    plain, _qv, _gv = _want(metric, thr, 65, 257)
    assert plain[0][-1] > _want(metric, thr, 65, 257, CR.INVALID, GINVALID)[0][0][-1]


def _links_bitmap(lib, table, n, metric, thr, valid):
    words = (n + 31) // 32
    adj = torch.empty((n, words), dtype=torch.int32, device="cuda")
    deg = torch.empty((n,), dtype=torch.int32, device="cuda")
    st = lib.trl_cluster_links(_ptr(table["g"]), _ptr(_mask_t(valid)), n, _ptr(table["mat"]), table["ld"], _ptr(table["n2"]), metric,
                               float(np.float32(thr)), _ptr(adj), words, _ptr(deg), 0, C_.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, lib.trl_last_error()
    torch.cuda.synchronize()
    return CR.unpack_bitmap(adj.cpu().numpy().view(np.uint32), n), deg.cpu().numpy()


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_self_mode_is_the_link_bitmap(lib, table, metric):
    """self = 1 on the table's rows: the lists are cluster_ref's link matrix and the bitmap trl_cluster_links writes, with and
    without the invalid rows; the counts are degree - 1."""
    s = CR.table_scores(metric)
    for n in (257, 33):
        for thr in CR.TABLE_THR[metric]:
            for invalid in ((), CR.INVALID):
                valid = CR.mask(n, invalid) if invalid else None
                link, deg = CR.table_links(metric, thr, n, invalid)
                want = R.range_ref(s[:n, :n], metric, thr, valid, valid, skip_self=True)
                assert np.array_equal(R.unpack(want[0], want[1], n, n), link)
                for strip_cols in STRIPS:
                    c = _search(lib, table, table["g"], n, n, metric, thr, want, (metric, n, thr, invalid, strip_cols), self_=1,
                                qvalid=valid, gvalid=valid, strip_cols=strip_cols)
                off, idx, _sc = c.result(c.total())
                bitmap, degree = _links_bitmap(lib, table, n, metric, thr, valid)
                assert np.array_equal(R.unpack(off, idx, n, n), bitmap)
                ok = degree > 0
                assert np.array_equal(np.diff(off)[ok], degree[ok] - 1) and (np.diff(off)[~ok] == 0).all() and np.array_equal(degree, deg)


@pytest.mark.parametrize("metric", (G.COSINE, G.EUCLIDEAN))
def test_capacity(lib, table, metric):
    """Entries below the capacity are the reference's; every byte at or past it keeps the sentinel."""
    thr = CR.TABLE_THR[metric][0]
    want, _qv, _gv = _want(metric, thr, 65, 257)
    total = int(want[0][-1])
    long_row = int(np.argmax(np.diff(want[0])))
    inside = int(want[0][long_row]) + int(np.diff(want[0])[long_row]) // 2
    assert np.diff(want[0])[long_row] > 32 and 1 < inside < total - 1
    for cap in (0, 1, total - 1, total, total + 5, inside):
        for strip_cols in (0, 256):
            _search(lib, table, table["q"], 65, 257, metric, thr, want, (metric, cap, strip_cols), capacity=cap, strip_cols=strip_cols)


def test_misaligned_queries_side_stream_and_repeats(lib, table):
    for metric in (G.COSINE, G.EUCLIDEAN):
        thr = CR.TABLE_THR[metric][0]
        want, _qv, _gv = _want(metric, thr, 65, 257)
        _search(lib, table, table["q4"], 65, 257, metric, thr, want, ("4-byte aligned", metric))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        c = Call(lib, table, table["q"], 65, 257, metric, thr, strip_cols=128)
        assert c.count(stream=side) == 0 and c.fill(c.total(), stream=side) == 0, lib.trl_last_error()
        first = c.result(c.total())
        _same(first, want, what=("side stream", metric))
        ws_first = c.ws.clone()
        assert c.count() == 0 and c.fill(c.total()) == 0, lib.trl_last_error()           # the same call again: the same bytes
        second = c.result(c.total())
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1]) and R.same_bits(first[2], second[2]).all()
        assert torch.equal(ws_first, c.ws)


def _identities(n_id, copies, rng, noise=0.5):
    """copies noisy unit copies of each of n_id random unit rows, copy c of identity i at row c * n_id + i."""
    base = rng.standard_normal((n_id, G.K)).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    rows = np.tile(base, (copies, 1)) + (noise / np.sqrt(G.K)) * rng.standard_normal((n_id * copies, G.K))
    rows = rows.astype(np.float32)
    return rows / np.linalg.norm(rows, axis=1, keepdims=True).astype(np.float32)


def test_default_plan_with_many_strips():
    """n = 96 against m = 4,224: 33 column groups and, by the default plan, 33 strips; then strips of three and of eight groups, whose
    waves walk several slabs each and whose last strip is short.  The yardstick is FaceGallery.scores() of the same call put through
    the reference (that kernel is pinned to gallery_ref by tests/test_gpu_gallery.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.gallery import FaceGallery
    rng = np.random.default_rng(4224)
    rows = _identities(264, 16, rng)
    q = _identities(96, 1, rng)
    q[:] = rows[:96] * 0.8 + q * 0.2                                           # each query near one identity, none a stored row
    gal = FaceGallery(metric="cosine", capacity=4224)
    gal.add(rows, range(4224))
    want = R.range_ref(gal.scores(q).cpu().numpy(), G.COSINE, 0.5)
    per_row = np.diff(want[0])
    assert (per_row >= 1).all() and (per_row < 4224).all() and per_row.max() >= 8
    groups = [np.unique(want[1][want[0][r]:want[0][r + 1]] // 128) for r in range(96)]
    assert min(len(g) for g in groups) >= 4                                    # every row has hits in several strips
    for strip_cols in (0, 384, 1024):
        off, idx, sc = gal.range_search(q, threshold=0.5, max_strip_cols=strip_cols)
        assert off.dtype == torch.int64 and idx.dtype == torch.int32 and sc.dtype == torch.float32
        _same((off.cpu().numpy(), idx.cpu().numpy(), sc.cpu().numpy()), want, what=("many strips", strip_cols))
        assert np.array_equal(gal.range_count(q, threshold=0.5, max_strip_cols=strip_cols).cpu().numpy(), per_row)


@pytest.mark.parametrize("n", (1025, 2049))
def test_more_rows_than_the_scan_has_threads(n):
    """k_range_scan's 1,024 threads own ceil(n / 1024) rows each: n = 1,025 (two a thread, the last thread with rows has one, half the
    threads none) and n = 2,049 (three a thread); every other shape of this file has n <= 257, one row a thread.  The queries are noisy
    copies of 256 stored rows, eight loose copies of an identity, so a row has one to eight matches; the yardstick is scores() put
    through the reference, as above."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.gallery import FaceGallery
    rng = np.random.default_rng(n)
    rows = _identities(32, 8, rng, noise=1.0)
    q = rows[np.arange(n) % 256] * 0.8 + _identities(n, 1, rng) * 0.2
    gal = FaceGallery(metric="cosine", capacity=256)
    gal.add(rows, range(256))
    want = R.range_ref(gal.scores(q).cpu().numpy(), G.COSINE, 0.5)
    per_row = np.diff(want[0])
    assert len(per_row) == n and (per_row >= 1).all() and per_row.max() <= 16 and len(np.unique(per_row)) > 2
    off, idx, sc = gal.range_search(q, threshold=0.5)
    _same((off.cpu().numpy(), idx.cpu().numpy(), sc.cpu().numpy()), want, what=("scan", n))
    assert np.array_equal(gal.range_count(q, threshold=0.5).cpu().numpy(), per_row)


def test_refusals_of_the_abi(lib, table):
    """Every refusal of the header, against the good call n = m = 33, self = 1: the status, the message's first word, and outputs
    that keep the sentinel."""
    bad = (dict(n=-1, self_=0), dict(m=-1, self_=0), dict(m=1 << 31, ld=1 << 31, self_=0), dict(ld=100), dict(ld=0), dict(ld=-32), dict(ld=32),
           dict(metric=2), dict(metric=-1), dict(self_=2), dict(self_=-1), dict(n=32), dict(m=32), dict(thr=float("nan")),
           dict(thr=float("inf")), dict(thr=float("-inf")), dict(strip_cols=100), dict(strip_cols=-128), dict(strip_cols=64))
    ws_bad = (dict(ws_delta=-1), dict(ws_delta=-100), dict(ws_offset=4))
    # pass 1: nothing is written
    for kw in bad + ws_bad:
        c = Call(lib, table, table["g"], 33, 33, 0, 0.12, self_=1)
        assert c.count(**kw) == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_range_count"), (kw, lib.trl_last_error())
        c.outputs_are_sentinels()
    for null in ("q", "mat", "n2", "offsets"):
        c = Call(lib, table, table["g"], 33, 33, 0, 0.12, self_=1)
        assert c.count(null=(null,)) == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_range_count"), null
        c.outputs_are_sentinels()
    # pass 2 behind a good pass 1: the lists keep the sentinel
    want = R.range_ref(CR.table_scores(0)[:33, :33], 0, 0.12, skip_self=True)
    for kw in bad + ws_bad + (dict(capacity=-1),):
        c = Call(lib, table, table["g"], 33, 33, 0, 0.12, self_=1, room=5)
        assert c.count() == 0 and c.total() == want[0][-1] > 0
        kw = dict(kw)
        cap = kw.pop("capacity", c.total())
        assert c.fill(cap, **kw) == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_range_fill"), (kw, lib.trl_last_error())
        assert (c.index == FILL32).all().item() and (c.score == FILL32).all().item()
    for null in ("q", "mat", "n2", "offsets", "index", "score"):
        c = Call(lib, table, table["g"], 33, 33, 0, 0.12, self_=1, room=5)
        assert c.count() == 0
        assert c.fill(c.total(), null=(null,)) == TRL_ERR_INVALID and lib.trl_last_error().startswith(b"trl_gallery_range_fill"), null
        assert (c.index == FILL32).all().item() and (c.score == FILL32).all().item()
    c = Call(lib, table, table["g"], 33, 33, 0, 0.12, self_=1, room=5)         # a null workspace where one is needed
    assert c.count(ws_delta=-c.need) == TRL_ERR_INVALID and b"workspace" in lib.trl_last_error()
    c.outputs_are_sentinels()
    # and the same call, unchanged, passes; a larger workspace is fine
    _search(lib, table, table["g"], 33, 33, 0, 0.12, want, "good", self_=1)
    c = Call(lib, table, table["g"], 33, 33, 0, 0.12, self_=1)
    assert c.count(ws_delta=8) == 0 and c.fill(c.total(), ws_delta=8) == 0
    _same(c.result(c.total()), want)


def test_face_gallery_range_search(lib):
    from truely_amd.gallery import FaceGallery
    g, q = G.tables()
    for name, metric in G.METRICS.items():
        gal = FaceGallery(metric=name, capacity=32)
        off, idx, sc = gal.range_search(threshold=0.5)                                     # an empty gallery
        assert off.tolist() == [0] and idx.shape == sc.shape == (0,) and gal.range_count(q[:3], threshold=0.5).tolist() == [0, 0, 0]
        gal.add(g[:20], range(20))
        gal.add(g[20:], range(20, 257))
        thr = CR.TABLE_THR[metric][0]
        s_q, s_self = G.table_scores(metric), CR.table_scores(metric)
        valid, qvalid = CR.mask(257), CR.mask(65)

        def same(got, want):
            assert all(x.device.type == "cuda" for x in got)
            assert (got[0].dtype, got[1].dtype, got[2].dtype) == (torch.int64, torch.int32, torch.float32)
            _same(tuple(x.cpu().numpy() for x in got), want)

        same(gal.range_search(q, thr), R.range_ref(s_q, metric, thr))
        same(gal.range_search(torch.from_numpy(q.copy()).cuda(), threshold=thr, valid=qvalid, gallery_valid=torch.from_numpy(valid),
                              max_strip_cols=128), R.range_ref(s_q, metric, thr, qvalid, valid))
        want_self = R.range_ref(s_self, metric, thr, skip_self=True)
        same(gal.range_search(threshold=thr), want_self)
        link, degree = CR.table_links(metric, thr)
        got = gal.range_search(threshold=thr, max_strip_cols=256)
        assert np.array_equal(R.unpack(got[0].cpu().numpy(), got[1].cpu().numpy(), 257, 257), link)
        assert np.array_equal(gal.range_count(threshold=thr).cpu().numpy(), degree - 1)
        info = gal.cluster(thr, return_info=True)
        assert np.array_equal(gal.range_count(threshold=thr).cpu().numpy(), info["degree"].cpu().numpy() - 1)
        for kw in (dict(valid=valid), dict(gallery_valid=valid)):
            same(gal.range_search(threshold=thr, **kw), R.range_ref(s_self, metric, thr, valid, valid, skip_self=True))
        counts = gal.range_count(q, thr, valid=qvalid)
        assert counts.dtype == torch.int64 and counts.device.type == "cuda"
        assert np.array_equal(counts.cpu().numpy(), np.diff(R.range_ref(s_q, metric, thr, qvalid)[0]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = gal.range_search(q, thr)
            side.synchronize()
        same(got, R.range_ref(s_q, metric, thr))
        # max_results: at the total it passes, below it the total is named
        total = int(want_self[0][-1])
        same(gal.range_search(threshold=thr, max_results=total), want_self)
        with pytest.raises(ValueError, match=str(total)):
            gal.range_search(threshold=thr, max_results=total - 1)
        for kw in (dict(threshold=thr, valid=qvalid), dict(threshold=thr, valid=valid, gallery_valid=valid), dict(emb=q, threshold=thr, valid=valid),
                   dict(emb=q, threshold=thr, gallery_valid=qvalid), dict(emb=q[:, :100], threshold=thr), dict()):
            with pytest.raises(ValueError):
                gal.range_search(**kw)
            with pytest.raises(ValueError):
                gal.range_count(**kw)
        for kw in (dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=thr, max_strip_cols=100)):
            with pytest.raises(_lib.TrlError, match="trl_gallery_range_count"):
                gal.range_search(q, **kw)
    with pytest.raises(ValueError):
        FaceGallery(metric="manhattan")
