"""The host layer of the context-free entry points without a GPU: every call that trl_gallery.hip, trl_cluster.hip, trl_tracks.hip,
trl_pool.hip and trl_quality.hip answer BEFORE their first HIP call -- a refusal, or "nothing to do" -- with its status and its
message, against tests/golden/host_refusals.json, and trl_quality_workspace's byte counts against the same file.

The golden file was recorded from the library of the commit BEFORE the entry points moved onto csrc/trl_host.h; a status or a
message that differs is a change of behaviour.  `python tests/test_host_layer_cpu.py --record` writes it from whatever library
TRUELY_HIP_LIB selects: record it from the library the change is held against, never from the tree under test.

Per entry the table holds: a null for each required pointer, a state / key / workspace pointer off by 4 bytes, each count at -1 and
at one past its documented limit, bad enumerators (metric, mode, pairs, self, tile_rows, lanes_per_row), a workspace one byte too
small, and the calls that succeed with nothing to do (m == 0, n == 0, groups == 0, with the null outputs those allow).  No case
reaches the device lookup: every status is TRL_OK or TRL_ERR_INVALID."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_refusals.json")
NAN, INF = float("nan"), float("inf")
QUALITY_M = (0, 1, 2, 3, 255, 256, 65535, 65536, 2 ** 24, -1, 2 ** 24 + 1)

_BUF = (C.c_longlong * 512)()           # never read or written: every case is answered before the pointers are used
P = C.addressof(_BUF)


def _show(v):
    if v is None:
        return "null"
    if isinstance(v, int) and P <= v < P + C.sizeof(_BUF):
        return "p" if v == P else f"p+{v - P}"
    if isinstance(v, C.Structure):
        return "(" + ", ".join(repr(getattr(v, n)) for n, _ in v._fields_) + ")"
    return repr(v)


class _Entry:
    """One exported function with an argument list that it accepts; __call__ gives the case that changes some of them."""

    def __init__(self, lib, name, **base):
        self.fn, self.name, self.base = getattr(lib, name), name, base

    def __call__(self, **changed):
        assert set(changed) <= set(self.base), (self.name, changed)
        args = dict(self.base, **changed)
        label = f"{self.name}({', '.join(f'{k}={_show(v)}' for k, v in changed.items())})"
        return label, lambda: self.fn(*args.values())

    def each(self, **values):
        """One case per value: each(m=(-1, 5), k=(0,)) -> m=-1, m=5, k=0"""
        return [self(**{k: v}) for k, vs in values.items() for v in vs]


def _cases(lib):
    from truely_amd._lib import TrlQualityParams
    out = []
    ws_cases = lambda e, need: [e(ws_bytes=need - 1), e(ws=P + 4), e(ws=None)]
    gallery_bad = dict(mat=(None,), n2=(None,), ld=(0, 33, -32))

    e = _Entry(lib, "trl_gallery_pack", rows=P, m=1, mat=P, ld=32, n2=P, c0=0, stream=None)
    out += e.each(m=(-1, 2 ** 31), c0=(-1, 32), rows=(None,), **gallery_bad) + [e(m=0), e(m=0, rows=None), e(m=0, c0=32)]

    e = _Entry(lib, "trl_gallery_scores", q=P, n=1, mat=P, ld=32, n2=P, m=1, metric=0, out=P, ldo=1, stream=None)
    out += e.each(n=(-1,), m=(-1, 2 ** 31, 33), metric=(2, -1), ldo=(0,), q=(None,), out=(None,), **gallery_bad)
    out += [e(n=2 ** 31 - 32, m=2 ** 31 - 1, ld=2 ** 31, ldo=2 ** 31 - 1), e(n=0), e(n=0, q=None, out=None), e(m=0, ldo=0), e(m=0, q=None, out=None)]

    for grouped in (False, True):
        base = dict(q=P, valid=None, n=1, mat=P, ld=256, n2=P, gid=P, m=256, metric=0, k=1, score=P, index=P, group=P, ws=P, ws_bytes=0,
                    max_strip_cols=128, stream=None)
        if not grouped:
            del base["gid"], base["group"]
        size = lib.trl_gallery_search_groups_workspace if grouped else lib.trl_gallery_search_workspace
        need = size(1, 256, 1, 128)
        assert need > 0
        e = _Entry(lib, "trl_gallery_search_groups" if grouped else "trl_gallery_search", **dict(base, ws_bytes=need))
        out += e.each(n=(-1,), m=(-1, 2 ** 31, 257), k=(0, 17), max_strip_cols=(-128, 100), metric=(2, -1), q=(None,), score=(None,),
                      index=(None,), **gallery_bad)
        out += ws_cases(e, need) + [e(n=0), e(n=0, q=None, score=None, index=None, ws=None, ws_bytes=0)]
        if grouped:
            out += e.each(gid=(None,), group=(None,)) + [e(n=0, m=0, gid=None, group=None)]

    need = lib.trl_gallery_range_workspace(1, 1, 0)
    assert need > 0
    base = dict(q=P, qvalid=None, n=1, mat=P, ld=32, n2=P, gvalid=None, m=1, metric=0, threshold=0.5, self_pairs=0, offsets=P, ws=P, ws_bytes=need)
    range_bad = dict(n=(-1,), m=(-1, 2 ** 31, 33), max_strip_cols=(-128, 100), metric=(2, -1), self_pairs=(2, -1), threshold=(NAN, INF, -INF),
                     offsets=(None,), q=(None,), **gallery_bad)
    e = _Entry(lib, "trl_gallery_range_count", **base, max_strip_cols=0, stream=None)
    out += e.each(**range_bad) + ws_cases(e, need) + [e(self_pairs=1, m=2), e(n=0), e(n=0, q=None, offsets=None, ws=None, ws_bytes=0)]
    e = _Entry(lib, "trl_gallery_range_fill", **base, capacity=1, index=P, score=P, max_strip_cols=0, stream=None)
    out += e.each(**range_bad, capacity=(-1,), index=(None,), score=(None,)) + ws_cases(e, need)
    out += [e(self_pairs=1, m=2), e(n=0), e(n=0, q=None, offsets=None, ws=None, ws_bytes=0), e(capacity=0), e(capacity=0, index=None, score=None),
            e(m=0, ws=None, ws_bytes=0), e(m=0, q=None, index=None, score=None, ws=None, ws_bytes=0)]

    e = _Entry(lib, "trl_cluster_links", q=P, valid=None, n=1, mat=P, ld=32, n2=P, metric=0, threshold=0.5, adj=P, pitch_words=1, degree=P,
               max_strip_cols=0, stream=None)
    out += e.each(n=(-1, 65537, 33), max_strip_cols=(-128, 100), metric=(2, -1), threshold=(NAN, INF), pitch_words=(0,), q=(None,), adj=(None,),
                  degree=(None,), **gallery_bad)
    out += [e(n=0), e(n=0, pitch_words=0, q=None, adj=None, degree=None)]

    need = lib.trl_gallery_hist_workspace(1, 1, 1, 0)
    assert need > 0
    e = _Entry(lib, "trl_gallery_hist", q=P, qvalid=None, qid=P, n=1, mat=P, ld=32, n2=P, gvalid=None, gid=P, m=1, metric=0, pairs=0, edges=P,
               nedges=1, counts=P, ws=P, ws_bytes=need, max_strip_cols=0, stream=None)
    out += e.each(nedges=(0, 1024, -1), n=(-1,), m=(-1, 2 ** 31, 33), max_strip_cols=(-128, 100), metric=(2, -1), pairs=(2, -1), edges=(None,),
                  counts=(None,), q=(None,), qid=(None,), gid=(None,), **gallery_bad)
    out += ws_cases(e, need) + [e(pairs=1, m=2)]

    need = lib.trl_cluster_workspace(1)
    assert need > 0
    e = _Entry(lib, "trl_cluster_labels", adj=P, pitch_words=1, degree=P, n=1, min_samples=1, labels=P, core=P, count=P, ws=P, ws_bytes=need,
               rounds_out=None, stream=None)
    out += e.each(n=(-1, 65537), min_samples=(0, -1), pitch_words=(0,), count=(None,), adj=(None,), degree=(None,), labels=(None,), core=(None,))
    out += ws_cases(e, need)

    need = lib.trl_cluster_lists_workspace(1)
    assert need > 0
    e = _Entry(lib, "trl_cluster_labels_lists", offsets=P, index=P, valid=None, n=1, min_samples=1, lanes_per_row=0, degree=P, labels=P, core=P,
               count=P, ws=P, ws_bytes=need, rounds_out=None, stream=None)
    out += e.each(n=(-1, 2 ** 24 + 1), min_samples=(0,), lanes_per_row=(3, 128, -4, 1), count=(None,), offsets=(None,), index=(None,),
                  degree=(None,), labels=(None,), core=(None,))
    out += ws_cases(e, need)

    e = _Entry(lib, "trl_track_update", state=P, boxes=P, counts=P, n=1, m=1, emb=None, iou_min=0.1, sim_min=0.4, max_age=3, track=P, sim=P,
               flag=P, table=P, table_cap=1, stream=None)
    out += e.each(n=(-1,), m=(-1,), max_age=(-1,), table_cap=(-1,), iou_min=(NAN,), sim_min=(NAN,), state=(None, P + 4), counts=(None,),
                  boxes=(None,), track=(None,), sim=(None,), flag=(None,), table=(None,))
    e = _Entry(lib, "trl_track_scores", state=P, table=P, table_cap=1, frame_count=1, fps=1, score=P, summary=P, stream=None)
    out += e.each(table_cap=(-1,), state=(None,), summary=(None,), table=(None,), score=(None,))

    state_bad = (None, P + 4)
    groups_bad = (-1, 2 ** 31)
    e = _Entry(lib, "trl_pool_reset", state=P, groups=2, stream=None)
    out += e.each(state=state_bad, groups=groups_bad)
    rows_bad = dict(ld=(511, 0), m=(-1, 2 ** 30 + 1), tile=(1, 7, 64, -8), rows=(None,), gid=(None,))
    e = _Entry(lib, "trl_pool_add", state=P, groups=2, g0=0, rows=P, ld=512, n2=None, gid=P, w=None, m=1, tile=0, stream=None)
    out += e.each(state=state_bad, groups=groups_bad, **rows_bad) + [e(m=0), e(m=0, rows=None, gid=None), e(m=0, groups=0)]
    e = _Entry(lib, "trl_pool_finish", state=P, groups=2, mode=0, template=P, count=P, weight=P, cohesion=P, skipped=None, stream=None)
    out += e.each(state=state_bad, groups=groups_bad, mode=(2, -1), template=(None,), count=(None,), weight=(None,), cohesion=(None,))
    out += [e(groups=0), e(groups=0, template=None, count=None, weight=None, cohesion=None)]
    e = _Entry(lib, "trl_pool_rep_reset", key=P, groups=2, stream=None)
    out += e.each(key=state_bad, groups=groups_bad) + [e(groups=0)]
    e = _Entry(lib, "trl_pool_rep_add", key=P, groups=2, g0=0, template=P, rows=P, ld=512, n2=None, gid=P, w=None, row0=0, m=1, tile=0,
               stream=None)
    out += e.each(key=state_bad, groups=groups_bad, template=(None,), row0=(-1, 2 ** 31 - 1), **rows_bad)
    out += [e(row0=2 ** 31 - 2 ** 30, m=2 ** 30), e(m=0), e(m=0, row0=2 ** 31 - 1), e(m=0, template=None, rows=None, gid=None), e(groups=0),
            e(groups=0, template=None, rows=None, gid=None)]
    e = _Entry(lib, "trl_pool_rep_finish", key=P, groups=2, index=P, score=P, stream=None)
    out += e.each(key=state_bad, groups=groups_bad, index=(None,), score=(None,)) + [e(groups=0), e(groups=0, index=None, score=None)]

    need = lib.trl_quality_workspace(1)
    assert need > 0
    prm = lambda **kw: TrlQualityParams(**dict(dict(sharp_ref=100.0, clip_ref=0.5, contrast_ref=64.0, yaw_ref=1.0, pitch_ref=1.0, size_ref=80.0), **kw))
    e = _Entry(lib, "trl_face_quality", frames=P, n=1, H=8, W=8, frame_of=P, boxes=P, points=None, m=1, params=None, max_band_rows=0, ws=P,
               ws_bytes=need, raw=P, feat=P, hist=None, status=P, stream=None)
    out += e.each(m=(-1, 2 ** 24 + 1), n=(-1,), H=(0, 16385), W=(0, 16385), max_band_rows=(-1,), frames=(None,), frame_of=(None,), boxes=(None,),
                  raw=(None,), feat=(None,), status=(None,),
                  params=(prm(sharp_ref=0.0), prm(clip_ref=-1.0), prm(contrast_ref=NAN), prm(yaw_ref=INF), prm(pitch_ref=-0.0), prm(size_ref=-INF)))
    out += ws_cases(e, need) + [e(m=0), e(m=0, params=prm()),
                                e(m=0, n=0, frames=None, frame_of=None, boxes=None, ws=None, ws_bytes=0, raw=None, feat=None, status=None)]
    e = _Entry(lib, "trl_best_update", keys=P, groups=2, quality=P, gid=P, m=1, row_base=0, faces=None, face_floats=0, best_faces=None, stream=None)
    out += e.each(keys=state_bad, groups=groups_bad, m=(-1,), row_base=(-1, 2 ** 31 - 1), faces=(P,), best_faces=(P,), quality=(None,), gid=(None,))
    out += [e(faces=P, best_faces=P, face_floats=0), e(m=0), e(m=0, row_base=2 ** 31 - 1), e(m=0, quality=None, gid=None), e(groups=0),
            e(groups=0, quality=None, gid=None)]
    e = _Entry(lib, "trl_best_read", keys=P, groups=2, row=P, quality=P, stream=None)
    out += e.each(keys=state_bad, groups=groups_bad, row=(None,), quality=(None,)) + [e(groups=0), e(groups=0, row=None, quality=None)]
    return out


def _sizes(lib):
    """The size functions' answers where they refuse (0) and, for the quality workspace, at every m the layout is held at."""
    out = [[f"trl_quality_workspace({m})", lib.trl_quality_workspace(m)] for m in QUALITY_M]
    out += [[f"trl_pool_state_bytes({g})", lib.trl_pool_state_bytes(g)] for g in (-1, 2 ** 31)]
    out += [[f"trl_cluster_workspace({n})", lib.trl_cluster_workspace(n)] for n in (-1, 65537)]
    out += [[f"trl_cluster_lists_workspace({n})", lib.trl_cluster_lists_workspace(n)] for n in (-1, 2 ** 24 + 1)]
    for a in ((-1, 1, 1, 0), (1, -1, 1, 0), (1, 2 ** 31, 1, 0), (1, 1, 0, 0), (1, 1, 17, 0), (1, 1, 1, 100)):
        out.append([f"trl_gallery_search_workspace{a}", lib.trl_gallery_search_workspace(*a)])
        out.append([f"trl_gallery_search_groups_workspace{a}", lib.trl_gallery_search_groups_workspace(*a)])
    out += [[f"trl_gallery_range_workspace{a}", lib.trl_gallery_range_workspace(*a)] for a in ((-1, 1, 0), (1, -1, 0), (1, 1, 100))]
    out += [[f"trl_gallery_hist_workspace{a}", lib.trl_gallery_hist_workspace(*a)] for a in ((-1, 1, 1, 0), (1, 1, 0, 0), (1, 1, 1024, 0), (1, 1, 1, 100))]
    return out


def record():
    """{"calls": [[case, status, message]], "sizes": [[call, bytes]]}: the message of a refusal, "" for a success."""
    from truely_amd import _lib
    lib = _lib.load()
    calls = []
    for label, call in _cases(lib):
        status = call()
        calls.append([label, status, lib.trl_last_error().decode() if status else ""])
    return {"calls": calls, "sizes": _sizes(lib)}


def _text(data) -> str:
    return json.dumps(data, indent=0, allow_nan=False) + "\n"


def test_refusals_and_sizes_equal_the_recorded_ones():
    got, want = record(), json.load(open(GOLDEN))
    labels = [c[0] for c in got["calls"]]
    assert len(set(labels)) == len(labels)
    assert all(status in (0, -1) for _l, status, _m in got["calls"])               # TRL_OK or TRL_ERR_INVALID: no case reached HIP
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    for g, w in zip(got["sizes"], want["sizes"]):
        assert g == w
    assert _text(got) == open(GOLDEN).read()                                      # ... and nothing missing or added: byte for byte


def test_quality_workspace_layout():
    """hists at offset 0 (1024 bytes a face), the sums behind them, 16 bytes a face: 1040 max(m, 1) bytes, 0 where m is refused"""
    sizes = dict(json.load(open(GOLDEN))["sizes"])
    for m in QUALITY_M:
        assert sizes[f"trl_quality_workspace({m})"] == (1040 * max(m, 1) if 0 <= m <= 2 ** 24 else 0), m


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    sys.path.insert(0, ROOT)
    import truely_amd  # noqa: F401
    open(GOLDEN, "w").write(_text(record()))
