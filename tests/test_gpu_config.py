"""The cascade at every threshold and max_faces its configuration accepts.

trl_config carries thr0, thr1, thr2 and max_faces; trl_create checks none of them beyond max_faces >= 1, and the rest of the
suite runs at (x, 0.7, 0.7) or (0, 0, 0) and max_faces = 64.  Here:

  a. trl_softmax2_p1 at stages 2 and 3 over its whole logit range, against list_ref.probs (orc_expf), bit for bit;
  b. thr1 / thr2 on a row's own probability and the floats on either side of it: the comparison is `p > thr`, as detect_face's
     `ipass = score > threshold`;
  c. thresholds outside (0, 1): +-0, 1, 2, +-inf, NaN, and one engine whose three thresholds differ, so that a stage reading
     another stage's field shows;
  d. the whole cascade against the oracle at stage thresholds off 0.7, with the oracle's row counts pinned so that no case is
     vacuous, and thr1 / thr2 on a real R-Net / O-Net probability;
  e. max_faces 1, 2, 3, 63, 65, 200: the truncation of k_select, the row stride of every max_faces-wide tensor, the memsets
     behind the counts, select_faces, extract_faces(keep_all=True), clone();
  f. thr0 on the inclusive edges 0.01f / 0.99f of the PNet prefilter and of the deferred confirm pass, and just outside them.

Logits are finite throughout: no layer can make a NaN or an infinity from uint8 pixels and finite weights, so the stage kernels
never see one.  All lists are 640 x 480 frames through trl_debug_lists, as in test_gpu_lists.py."""
import contextlib

import numpy as np
import pytest

import truely_amd
import extract_ref as X
import list_ref as R
from test_gpu_lists import _check, _run
from test_gpu_parity import _check_cascade
from test_gpu_pnet_screen import _check_levels, _oracle_maps

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = F32(np.inf)


@contextlib.contextmanager
def _engine(blob, **kw):
    from truely_amd.engine import Engine
    eng = Engine(blob, **kw)
    try:
        yield eng
    finally:
        eng.close()


def _np(t):
    return t.cpu().numpy()


# ---- a - c: the stage kernels on a list whose probabilities span the softmax's range ------------------------------------------
_REF = {}


@pytest.fixture(scope="module")
def span(oracle):
    """({kind: case}, the reference probabilities of the rows: both kinds carry the same logit pairs)"""
    cases = {kind: R.range_case(kind) for kind in (2, 3)}
    assert np.array_equal(cases[2]["logits"][0][:, :2], cases[3]["logits"][0][:, :2])
    return cases, R.probs(oracle.expf, cases[2]["logits"][0])


def _ref(oracle, case, thr):
    key = (case["kind"], F32(thr).tobytes())
    if key not in _REF:
        _REF[key] = R.reference(case, oracle.expf, max_faces=64, thr=thr)
    return _REF[key]


def _stage(eng, oracle, case, thr, tag):
    """one kind of the hook on `eng` against list_ref at `thr`; returns (the output's score column, the reference's)"""
    ref = _ref(oracle, case, thr)
    got = _run(eng, case)
    _check(case, ref, got, tag)
    k = f"rows{case['kind']}"
    return got[k][0][:, 4], ref[0][k][:, 4]


def test_stage_probabilities_over_the_logit_range(blob, oracle, span):
    cases, p = span
    n = len(p)
    assert 280 <= n <= 360
    # the reference reaches both ends of its range, and enough of the middle
    assert (p == F32(1)).any() and (p == R.CLAMP_PROB).any() and p.min() == R.CLAMP_PROB
    assert len(np.unique(p[(p > F32(0.01)) & (p < F32(0.99))])) >= 50
    with _engine(blob, thresholds=(0.6, -1.0, -1.0)) as eng:
        for kind in (2, 3):
            got, ref = _stage(eng, oracle, cases[kind], -1.0, f"range kind {kind}")
            # every row passes, and NMS and the pad test remove nothing: the score column is the probabilities, sorted
            assert len(ref) == n and len(got) == n
            assert np.array_equal(ref, np.sort(p)[::-1])


def _pick(p, which):
    if which == "half":
        return p[np.argmin(np.abs(p.astype(np.float64) - 0.5))]
    return F32(1) if which == "one" else R.CLAMP_PROB


# (nextafter(1, 2) adds nothing over the thresholds 2.0 and +inf below)
ON_ROW = [(w, s) for w in ("half", "one", "clamp") for s in ("below", "on", "above") if (w, s) != ("one", "above")]


@pytest.mark.parametrize("which,side", ON_ROW, ids=[f"{w}-{s}" for w, s in ON_ROW])
def test_stage_threshold_on_a_rows_probability(blob, oracle, span, which, side):
    cases, p = span
    v = _pick(p, which)
    hits = int((p == v).sum())
    assert hits >= 1 and (which != "half" or abs(float(v) - 0.5) < 0.01)
    t = {"below": np.nextafter(v, F32(0)), "on": v, "above": np.nextafter(v, F32(2))}[side]
    with _engine(blob, thresholds=(0.6, float(t), float(t))) as eng:
        assert F32(eng.cfg.thr1) == t and F32(eng.cfg.thr2) == t
        for kind in (2, 3):
            got, ref = _stage(eng, oracle, cases[kind], t, f"thr {t!r} kind {kind}")
            if side == "below":      # every row with probability v is kept (nothing else can remove it in this list)
                assert int((ref == v).sum()) == hits and int((got == v).sum()) == hits
            else:                    # p > thr is strict: a row ON the threshold is dropped
                assert not (ref == v).any() and not (got == v).any()
                assert len(got) == int((p > t).sum())


OUTSIDE = [("0", F32(0)), ("-0", F32(-0.0)), ("1", F32(1)), ("1-", np.nextafter(F32(1), F32(0))), ("2", F32(2)), ("-inf", -INF),
           ("+inf", INF), ("nan", F32(np.nan))]


@pytest.mark.parametrize("name,t", OUTSIDE, ids=[n for n, _ in OUTSIDE])
def test_stage_threshold_outside_the_unit_interval(blob, oracle, span, name, t):
    cases, p = span
    want = int((p > t).sum())                                # numpy's float32 comparison: false for NaN
    # nothing passes 1, 2, +inf, NaN; everything passes -inf and -- the reference softmax never returns 0 -- +-0
    assert want == {"0": len(p), "-0": len(p), "-inf": len(p), "1-": int((p == F32(1)).sum())}.get(name, 0)
    with _engine(blob, thresholds=(0.6, float(t), float(t))) as eng:
        assert F32(eng.cfg.thr1).tobytes() == t.tobytes() or name == "nan"
        for kind in (2, 3):
            got, ref = _stage(eng, oracle, cases[kind], t, f"thr {name} kind {kind}")
            assert len(ref) == want and len(got) == want


def test_each_stage_reads_its_own_threshold(blob, oracle, span):
    """(0.6, 0.0, NaN): stage 2 keeps every row, stage 3 none -- three different fields, so thr0 or the other stage's in the
    wrong place changes a count"""
    cases, p = span
    with _engine(blob, thresholds=(0.6, 0.0, float("nan"))) as eng:
        got, ref = _stage(eng, oracle, cases[2], 0.0, "mixed kind 2")
        assert len(ref) == len(p) and len(got) == len(p)
        got, ref = _stage(eng, oracle, cases[3], float("nan"), "mixed kind 3")
        assert len(ref) == 0 and len(got) == 0


# ---- d: the whole cascade against the oracle at stage thresholds off 0.7 -------------------------------------------------------
# per-frame (stage-2, stage-3) row counts of the oracle on the clip below (at the defaults: (15, 3), (13, 4))
TRIPLES = [((0.6, 0.0, 0.0), [(30, 8), (23, 6)]),
           ((0.6, 0.3, 0.5), [(30, 4), (23, 4)]),
           ((0.6, 0.9, 0.95), [(1, 0), (3, 1)]),
           ((0.6, 0.99, 0.999), [(0, 0), (0, 0)]),
           ((0.6, 1.0, 0.7), [(0, 0), (0, 0)]),
           ((0.6, 0.7, 1.0), [(15, 0), (13, 0)]),
           ((0.5, 0.6, 0.6), [(188, 12), (213, 16)])]


@pytest.fixture(scope="module")
def clip():
    return truely_amd.synthetic.synthetic_frames(2, 180, 320, seed=11, faces=-1)


@pytest.fixture(scope="module")
def orc(blob):
    """an oracle of this module's own: its params are set per case, and the session's stays at the defaults"""
    from oracle.oracle import Oracle
    return Oracle(blob)


@contextlib.contextmanager
def _oracle_at(orc, triple):
    was = (orc.params.thr0, orc.params.thr1, orc.params.thr2)
    orc.params.thr0, orc.params.thr1, orc.params.thr2 = (float(t) for t in triple)
    try:
        yield orc
    finally:
        orc.params.thr0, orc.params.thr1, orc.params.thr2 = was


def _oracle_counts(orc, clip):
    tr = [orc.detect(f, trace=True, max_trace=1 << 14)[2] for f in clip]
    return [(len(t["boxes1"]), len(t["boxes2"]), len(t["boxes3"])) for t in tr]


@pytest.mark.parametrize("triple,counts", TRIPLES, ids=["-".join(str(t) for t in tr) for tr, _ in TRIPLES])
def test_cascade_at_stage_thresholds(blob, orc, clip, triple, counts):
    with _oracle_at(orc, triple), _engine(blob, thresholds=triple) as eng:
        n = _oracle_counts(orc, clip)
        assert [c[1:] for c in n] == counts
        _check_cascade(eng, orc, clip)
        assert [tuple(len(eng.stage_boxes(s, f)) for s in (2, 3)) for f in range(2)] == counts
        if triple[0] == 0.5:
            # 860 + 794 stage-1 rows: more than the R-Net batch a new context starts with, so the call was re-run
            assert [c[0] for c in n] == [860, 794] and eng.stage_totals()[0] == 860 + 794
            assert eng.list_stats()["attempts"] >= 2


@pytest.fixture(scope="module")
def medians(orc, clip):
    """(p2, p3): the (upper) median probability of frame 0's stage-2 and stage-3 rows with thr1 = thr2 = 0"""
    with _oracle_at(orc, (0.6, 0.0, 0.0)):
        tr = orc.detect(clip[0], trace=True)[2]
    p2, p3 = (np.sort(tr[k][:, 4])[len(tr[k]) // 2] for k in ("boxes2", "boxes3"))
    assert (p2, p3) == (F32(0.7162569), F32(0.6642022))
    return p2, p3


@pytest.mark.parametrize("stage", [2, 3])
def test_cascade_threshold_on_a_real_probability(blob, orc, clip, medians, stage):
    """thr1 (thr2) one float below an R-Net (O-Net) probability of frame 0, then on it: the stage loses exactly that row"""
    p = medians[stage - 2]
    n = []
    for t in (np.nextafter(p, F32(0)), p):
        triple = (0.6, float(t), 0.0) if stage == 2 else (0.6, 0.0, float(t))
        with _oracle_at(orc, triple), _engine(blob, thresholds=triple) as eng:
            n.append(_oracle_counts(orc, clip)[0][stage - 1])
            _check_cascade(eng, orc, clip)
            assert len(eng.stage_boxes(stage, 0)) == n[-1]
            assert (eng.stage_boxes(stage, 0)[:, 4] == p).any() == (len(n) == 1)
    assert n == ([15, 14] if stage == 2 else [4, 3])


# ---- e: max_faces --------------------------------------------------------------------------------------------------------------
HOOK_FACES = (1, 2, 63, 65, 200)


@pytest.fixture(scope="module")
def face_cases(oracle):
    """kind-3 hook inputs: the special list with the selection frames behind it, and a dup list with 225 stage-3 rows; their
    references at every max_faces"""
    cases = [R.build_case(3, "special", 150), R.build_case(3, "dup", 450)]
    refs = {k: [R.reference(c, oracle.expf, max_faces=k) for c in cases] for k in HOOK_FACES + (64,)}
    assert len(refs[64][1][0]["rows3"]) > 200 and len(refs[64][0][0]["rows3"]) > 65
    assert [r["sel"]["count"] for r in refs[2][0]] == [2, 2, 2, 2, 0]
    return cases, refs


@pytest.fixture(scope="module")
def faces_engine(blob):
    """engines by max_faces, shared by the hook test and the end-to-end test, closed behind the module"""
    from truely_amd.engine import Engine
    made = {}

    def get(k):
        if k not in made:
            made[k] = Engine(blob, max_faces=k)
        assert made[k].cfg.max_faces == k
        return made[k]
    yield get
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("k", HOOK_FACES)
def test_select_kernel_at_max_faces(faces_engine, face_cases, k):
    cases, refs = face_cases
    eng = faces_engine(k)
    for case, ref, ref64 in zip(cases, refs[k], refs[64]):
        got = _run(eng, case)
        assert got["boxes"].shape[1] == k and got["points"].shape[1] == k
        _check(case, ref, got, f"max_faces {k} {case['fam']}")            # counts, rows [:count], box0 / prob0 / rect / valid
        for f, (r, r64) in enumerate(zip(ref, ref64)):
            assert r["sel"]["count"] == min(len(r["rows3"]), k)
            # max_faces bounds the rows returned, not the face the pipeline embeds
            for key in ("box0", "prob0", "rect", "valid"):
                assert np.array_equal(got[key][f], r64["sel"][key]), (k, f, key)


@pytest.fixture(scope="module")
def wide(engine, orc, clip):
    """what the default engine (max_faces 64) returns on the clip: 3 and 4 faces"""
    import torch
    n3 = [c[2] for c in _oracle_counts(orc, clip)]
    assert n3 == [3, 4]
    det = {(lm, sl): [_np(t) for t in engine.mtcnn_detect(clip, landmarks=lm, select_largest=sl)] for lm in (False, True)
           for sl in (True, False)}
    emb = {key: _np(v) for key, v in engine.detect_embed(clip).items()}
    ext = {key: _np(v) for key, v in engine.extract_faces(clip, keep_all=True).items()}
    torch.cuda.synchronize()
    for d in det.values():
        assert d[2].tolist() == n3
    return n3, det, emb, ext


@pytest.mark.parametrize("k", [1, 2, 3])
def test_cascade_at_max_faces(faces_engine, clip, wide, k):
    import torch
    n3, det, emb, ext = wide
    want = [min(n, k) for n in n3]
    H, W = clip.shape[1:3]
    eng = faces_engine(k)
    for (lm, sl), ref in det.items():
        # the outputs are torch.empty blocks: leave NaNs in the allocator's small free blocks, so that a slot the call does not
        # write is seen (best effort: which block an allocation gets is the allocator's choice)
        dirty = [torch.full((128,), float("nan"), device=eng.device) for _ in range(16)]
        torch.cuda.synchronize()
        del dirty
        got = eng.mtcnn_detect(clip, landmarks=lm, select_largest=sl)
        assert len(got) == (4 if lm else 3)
        counts = _np(got[2])
        assert counts.tolist() == want, (k, lm, sl)
        for a, b in zip([got[0], got[1]] + ([got[3]] if lm else []), [ref[0], ref[1]] + ([ref[3]] if lm else [])):
            a = _np(a)
            assert a.shape[:2] == (2, k)
            for f, c in enumerate(want):
                assert a[f, :c].tobytes() == b[f, :c].tobytes(), (k, lm, sl, f)
                assert not a[f, c:].view(np.uint32).any(), f"max_faces {k}: slots past the count are not zero"
        if not lm:                                           # MTCNN.select_boxes on the k-wide tensors
            boxes, probs = _np(got[0]), _np(got[1])
            for method in X.METHODS:
                pick = _np(eng.select_faces(got[0], got[1], got[2], H, W, method))
                for f, c in enumerate(want):
                    r = X.select(boxes[f, :c], probs[f, :c], method, W, H)
                    assert pick[f] == (-1 if r is None else r), (k, sl, method, f)
    out = eng.detect_embed(clip)
    for key, v in emb.items():
        assert _np(out[key]).tobytes() == v.tobytes(), key
    out = {key: _np(v) for key, v in eng.extract_faces(clip, keep_all=True).items()}
    assert out["counts"].tolist() == want
    first = np.concatenate([np.arange(c) + o for c, o in zip(want, np.cumsum([0] + n3[:-1]))])   # default rows of the first faces
    assert out["faces"].shape[0] == sum(want)
    for key in ("faces", "frame", "box", "prob", "status"):
        assert out[key].tobytes() == np.ascontiguousarray(ext[key][first]).tobytes(), key


def test_clone_keeps_thresholds_and_max_faces(blob, clip):
    with _engine(blob, thresholds=(0.6, 0.3, 0.5), max_faces=2) as eng:
        twin = eng.clone()
        try:
            for f in ("thr0", "thr1", "thr2", "max_faces"):
                assert getattr(twin.cfg, f) == getattr(eng.cfg, f)
            a = [_np(t) for t in eng.mtcnn_detect(clip, landmarks=True)] + [_np(v) for v in eng.detect_embed(clip).values()]
            b = [_np(t) for t in twin.mtcnn_detect(clip, landmarks=True)] + [_np(v) for v in twin.detect_embed(clip).values()]
            assert a[2].tolist() == [2, 2]                   # four faces each at (0.6, 0.3, 0.5), two returned
            assert a[0].shape == (2, 2, 4)
            assert [x.tobytes() for x in a] == [x.tobytes() for x in b]
        finally:
            twin.close()


# ---- f: thr0 on the prefilter's own edges --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(oracle):
    fr = truely_amd.synthetic.synthetic_frames(2, 120, 160, seed=41)
    return fr, _oracle_maps(oracle, fr, 120, 160)


EDGES = [("0.01", F32(0.01), True), ("0.01-", np.nextafter(F32(0.01), F32(0)), False),
         ("0.99", F32(0.99), True), ("0.99+", np.nextafter(F32(0.99), F32(1)), False)]


@pytest.mark.parametrize("name,thr,inside", EDGES, ids=[e[0] for e in EDGES])
def test_thr0_on_the_prefilter_edges(blob, small, name, thr, inside):
    """0.01f and 0.99f are the inclusive ends of the range the prefilter (and with it the deferred confirm pass) serves: on them a
    queue is set up, one float outside every M-tile runs the exact chain inline; the records are the oracle's on both sides"""
    fr, maps = small
    with _engine(blob, thresholds=(float(thr), 0.7, 0.7), cap_level=3072, cap_frame=3072) as eng:
        assert F32(eng.cfg.thr0) == thr
        n = _check_levels(eng, maps, fr, float(thr))
        q = eng.pnet_defer()
        if inside:
            assert q["slots"] > 0 or q["hold"] > 0, q
        else:
            assert q["slots"] == 0 and q["hold"] == 0 and q["queued"] == 0, q
        assert n > 0 or thr > 0.9
