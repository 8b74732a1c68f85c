"""Face quality without a GPU: tests/quality_ref.py (the reference the GPU tests hold the kernels to) against independent
computations -- a float64 convolution of the mirror-padded crop, counted histograms, sorted-array percentiles, np.var within a derived
bound --, its invariance under any split of a rectangle's rows into bands, csrc/trl_quality.h built for the host (plain, and with the
sanitizers) and held to the reference bit for bit, the best shot's key against its definition, and the ABI's host side."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import quality_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc")
F32, F64 = np.float32, np.float64


def _crops():
    """(batch, row name, frame, crop luma) of every rectangle of the table that holds a face"""
    frame_of, boxes = Q.rect_table()
    for batch, frames in Q.frame_batches().items():
        for r, row in enumerate(Q.RECTS):
            status, (X0, Y0, X1, Y1) = Q.rect_of(int(frame_of[r]), 4, Q.H, Q.W, boxes[r])
            assert status == (row[0] not in Q.NO_FACE), row[0]
            if status:
                yield batch, row[0], int(frame_of[r]), Q.luma(frames[frame_of[r], Y0:Y1, X0:X1])


def test_rectangles_of_the_table():
    frame_of, boxes = Q.rect_table()
    rect = {row[0]: Q.rect_of(int(frame_of[r]), 4, Q.H, Q.W, boxes[r])[1] for r, row in enumerate(Q.RECTS)}
    size = {k: (v[2] - v[0], v[3] - v[1]) for k, v in rect.items()}
    assert size["1x1"] == (1, 1) and size["1x5"] == (1, 5) and size["5x1"] == (5, 1) and size["2x2"] == (2, 2) and size["3x3"] == (3, 3)
    assert [size[k][0] for k in ("w63", "w64", "w65")] == [63, 64, 65]
    assert rect["larger"] == rect["exact_frame"] == rect["huge_finite"] == (0, 0, Q.W, Q.H)
    assert rect["straddles"] == (0, 80, 21, Q.H)
    assert rect["frac_out"] == (10, 20, 41, 51) and rect["frac_in"] == (11, 21, 40, 50) and rect["frac_1x1"] == (10, 20, 11, 21)
    assert all(rect[k] == (0, 0, 0, 0) for k in Q.NO_FACE)


def test_luma_rule():
    assert Q.luma(np.array([255, 255, 255])) == 255 and Q.luma(np.array([0, 0, 0])) == 0
    assert 1868 + 9617 + 4899 == 1 << 14                                     # the weights sum to one: a grey stays itself
    g = np.arange(256)
    assert (Q.luma(np.stack([g, g, g], -1)) == g).all()
    assert Q.luma(np.array([255, 0, 0])) == 29 and Q.luma(np.array([0, 255, 0])) == 150 and Q.luma(np.array([0, 0, 255])) == 76


def test_reference_against_independent_computations():
    seen = 0
    for batch, name, frame, Y in _crops():
        h, w = Y.shape
        hist, sl, sl2 = Q.band_sums(Y, 0, h)
        # the Laplacian: a float64 3 x 3 convolution of the mirror-padded crop (a single row or column is its own neighbour)
        P = np.pad(Y.astype(F64), 1, mode="reflect") if min(h, w) > 1 else \
            np.pad(np.pad(Y.astype(F64), ((1, 1), (0, 0)), mode="reflect" if h > 1 else "edge"), ((0, 0), (1, 1)), mode="reflect" if w > 1 else "edge")
        L = P[:-2, 1:-1] + P[2:, 1:-1] + P[1:-1, :-2] + P[1:-1, 2:] - 4 * P[1:-1, 1:-1]
        assert L.sum() == sl and (L * L).sum() == sl2, (batch, name)
        assert np.abs(L).max() <= 1020
        if batch == "flat" and min(h, w) > 1:
            assert (np.abs(L) == (1020 if frame == 3 else 0)).all(), (batch, name)     # the checkerboard; a constant
        # the histogram, counted bin by bin; the percentiles of the sorted pixels
        assert hist.tolist() == [int((Y == v).sum()) for v in range(256)]
        raw, p05, p95 = Q.raw_of(hist, sl, sl2, w)
        N = h * w
        s = np.sort(Y.reshape(-1))
        assert p05 == s[-(-N // 20) - 1] and p95 == s[-(-19 * N // 20) - 1], (batch, name)
        assert raw.tolist() == [N, Y.sum(), (Y * Y).sum(), sl, sl2, (Y <= 15).sum(), (Y >= 240).sum(), w]
        # sharpness: float32 of a float64 chain a - b b with a = SL2 / N, b = SL / N.  Three float64 roundings on a and b b, one on
        # the difference, one to float32: |sharpness - var| <= 2^-24 |var| + 4 * 2^-53 (a + b^2), doubled for np.var's own rounding
        feat = Q.features(1, raw, p05, p95, h, None)
        var = np.var(L)
        bound = 2.0 ** -24 * var + 8 * 2.0 ** -53 * (sl2 / N + (sl / N) ** 2) + 1e-300
        assert abs(F64(feat[1]) - var) <= bound, (batch, name, float(feat[1]), var)
        assert 0 <= feat[0] <= 1 and feat[2] == F32(Y.mean()) and np.isnan(feat[6:10]).all()
        seen += 1
    assert seen == 2 * (len(Q.RECTS) - len(Q.NO_FACE))


def test_raw_sums_do_not_depend_on_the_bands():
    rng = np.random.default_rng(11)
    for batch, name, frame, Y in _crops():
        h = Y.shape[0]
        whole = Q.band_sums(Y, 0, h)
        for trial in range(4):
            cuts = [0, h] if trial == 0 else sorted({0, h, *rng.integers(0, h + 1, trial * 3).tolist()})
            if trial == 1:
                cuts = list(range(h + 1))                                   # every row its own band
            hist, sl, sl2 = np.zeros(256, np.int64), 0, 0
            for a, b in zip(cuts[:-1], cuts[1:]):
                part = Q.band_sums(Y, a, b)
                hist, sl, sl2 = hist + part[0], sl + part[1], sl2 + part[2]
            assert (hist == whole[0]).all() and (sl, sl2) == whole[1:], (batch, name, cuts)


def test_pose_and_composite_rules():
    pts = Q.points_table()
    pose = {name: Q.pose_of(pts[i]) for i, (name, _) in enumerate(Q.POINTS)}
    assert pose["frontal"].tolist() == [0.0, 0.0, 0.0, 40.0]
    assert pose["turned"][0] > 0 and pose["turned_mirror"][0] == -pose["turned"][0] and pose["turned_mirror"][1] == pose["turned"][1]
    assert pose["turned_mirror"][2] == -pose["turned"][2] and pose["turned_mirror"][3] == pose["turned"][3]
    assert pose["nose_on_left_eye"][0] == -1 and pose["nose_on_right_eye"][0] == 1 and pose["nose_past_eye"][0] == 2
    assert all(np.isnan(pose[k]).all() for k in Q.NAN_POSE)
    assert pose["chin_down"][1] > 0.8 and pose["rolled"][2] > 0.5
    Y = Q.luma(Q.frame_batches()["busy"][0, 0:90, 0:100])
    raw, p05, p95 = Q.raw_of(*Q.band_sums(Y, 0, 90), 100)
    q = {name: Q.features(1, raw, p05, p95, 90, pts[i])[0] for i, (name, _) in enumerate(Q.POINTS)}
    none = Q.features(1, raw, p05, p95, 90, None)[0]
    assert none == q["frontal"] and 0.9 < none < 1                            # noise: sharp, full contrast, a little clipping, 90 px
    assert all(q[k] == 0 for k in Q.NAN_POSE + ("nose_on_left_eye", "nose_on_right_eye", "nose_past_eye")) and 0 < q["turned"] < 1
    assert Q.features(1, raw, p05, p95, 90, pts[1], dict(yaw_ref=3.0))[0] > q["turned"]
    assert Q.features(1, raw, p05, p95, 90, None, dict(size_ref=180.0))[0] == none * F32(0.5)
    assert not Q.features(0, raw, p05, p95, 90, pts[0]).any()
    flat = Q.quality_ref(Q.frame_batches()["flat"], [0, 1, 2, 3], [[0, 0, 128, 96]] * 4)
    assert flat["quality"].tolist() == [0, 0, 0, 0] and flat["sharpness"].tolist() == [0, 0, 0, 1020.0 ** 2]
    assert flat["dark_frac"].tolist() == [0, 1, 0, 0.5] and flat["bright_frac"].tolist() == [0, 0, 1, 0.5] and flat["contrast"][3] == 255


# ---- csrc/trl_quality.h on the host -----------------------------------------------------------------------------------------------------
def _compile(tmp, sanitize: bool):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp / ("quality_san" if sanitize else "quality"))
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(ROOT, "tests", "quality_main.cpp"),
           "-o", out]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and sanitize:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def quality_program(request, tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("quality"), request.param == "sanitized")


def _hex(a):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32).tolist())


def _params_hex(params):
    return _hex([F32({**Q.DEFAULTS, **(params or {})}[k]) for k in ("sharp_ref", "clip_ref", "contrast_ref", "yaw_ref", "pitch_ref", "size_ref")])


def test_header_equals_reference(quality_program, tmp_path):
    """csrc/trl_quality.h on the host, banded three ways: every rectangle of the table on both frame batches, and the points table
    under every parameter set."""
    frame_of, boxes = Q.rect_table()
    pts = Q.points_table()
    pf = np.zeros(len(pts), np.int32)
    pb = np.tile(np.array([[3.5, 2.25, 99.5, 90.0]], F32), (len(pts), 1))
    for batch, frames in Q.frame_batches().items():
        path = tmp_path / f"{batch}.bin"
        path.write_bytes(frames.tobytes())
        cases = [(frame_of, boxes, None, None, band) for band in (1, 7, 1000)]
        cases += [(pf, pb, pts, prm, 13) for prm in Q.PARAM_SETS]
        script = []
        for fo, bx, pt, prm, band in cases:
            script.append(f"Q 4 {Q.H} {Q.W} {len(bx)} {int(pt is not None)} {band} {_params_hex(prm)}")
            script += [f"{int(fo[r])} {_hex(bx[r])}" + ("" if pt is None else " " + _hex(pt[r])) for r in range(len(bx))]
        r = subprocess.run([quality_program, str(path)], input="\n".join(script) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = iter(r.stdout.splitlines())
        for n, (fo, bx, pt, prm, band) in enumerate(cases):
            ref = Q.quality_ref(frames, fo, bx, pt, prm)
            for i in range(len(bx)):
                v = next(lines).split()
                assert int(v[0]) == ref["status"][i], (batch, n, i)
                assert [int(t) for t in v[1:9]] == ref["raw"][i].tolist(), (batch, n, i)
                got = np.array([int(t, 16) for t in v[9:21]], np.uint32).view(F32)
                assert Q.same_bits(got, ref["feat"][i]), (batch, n, i, got.tolist(), ref["feat"][i].tolist())
                assert [int(t) for t in v[21:]] == ref["hist"][i].tolist(), (batch, n, i)
        assert next(lines, None) is None


def test_best_shot_keys(quality_program, tmp_path):
    """The key orders rows as the definition does -- larger quality, ties (-0 == +0 among them) to the lower row, NaN never -- for
    every split of the rows into calls, ids outside the groups are ignored, and trl_best_key on the host gives the reference's keys."""
    q = Q.best_qualities()
    m = len(q)
    rng = np.random.default_rng(9)
    for G_ in (1, 3, 70):
        gid = rng.integers(-2, G_ + 2, m).astype(np.int32)
        faces = rng.standard_normal((m, 5)).astype(F32)
        want = Q.best_brute(q, gid, G_)
        assert (want >= 0).all() if G_ <= 3 else ((want >= 0).any() and (want < 0).any())
        results = []
        for cuts in Q.BEST_SPLITS:
            keys, best = [0] * G_, np.zeros((G_, 5), F32)
            for a, b in zip(cuts[:-1], cuts[1:]):
                Q.best_update(keys, q[a:b], gid[a:b], a, faces[a:b], best)
            row, quality = Q.best_read(keys, q)
            assert (row == want).all(), (G_, cuts)
            live = row >= 0
            assert Q.same_bits(quality[live], q[row[live]]) and np.isnan(quality[~live]).all()
            assert Q.same_bits(best[live], faces[row[live]]) and not best[~live].any()
            results.append((row, quality, best))
        assert all(Q.same_bits(a, b) for r in results[1:] for a, b in zip(r, results[0]))
    # a group of -0 and +0 alone: the first row wins with its own sign; a group of NaN alone has no best row
    keys = [0, 0]
    Q.best_update(keys, np.array([-0.0, 0.0, np.nan, np.nan], F32), [0, 0, 1, 1], 0)
    row, quality = Q.best_read(keys, np.array([-0.0, 0.0, np.nan, np.nan], F32))
    assert row.tolist() == [0, -1] and np.signbit(quality[0]) and quality[0] == 0 and np.isnan(quality[1])
    # the header's key
    pairs = [(v, i) for v in (0.0, -0.0, 1.0, 0.5, -1.0, np.nan, np.inf, -np.inf, 1e-45, 0.99999994) for i in (0, 1, 77, 2 ** 31 - 2)]
    (tmp_path / "none.bin").write_bytes(b"")
    script = f"K {len(pairs)}\n" + "".join(f"{_hex([v])} {i}\n" for v, i in pairs)
    r = subprocess.run([quality_program, str(tmp_path / "none.bin")], input=script, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    for (v, i), line in zip(pairs, r.stdout.splitlines(), strict=True):
        key, back, bits = line.split()
        assert int(key, 16) == Q.best_key(v, i), (v, i)
        assert (int(back), int(bits, 16)) == ((-1, 0x7FC00000) if np.isnan(v) else (i, int(np.array(v, F32).view(np.uint32)))), (v, i)


def test_abi_rejections_need_no_device():
    import truely_amd
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_quality_workspace", "trl_face_quality", "trl_best_update", "trl_best_read"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    section = hdr[hdr.index("Face quality"):]
    assert "UNPINNED" in section and "PLACEHOLDERS" in section
    assert all(hasattr(truely_amd, n) for n in ("face_quality", "QualityParams", "BestShots"))
    lib = _lib.load()
    assert lib.trl_abi_version() == 7
    ws = lib.trl_quality_workspace
    assert ws(1) == 1040 and ws(0) == ws(1) and ws(1000) == 1040 * 1000 and ws(-1) == 0 and ws(2 ** 24 + 1) == 0
    buf = (C.c_longlong * 4096)()
    p = C.addressof(buf)
    prm = lambda **kw: _lib.TrlQualityParams(*[kw.get(k, 1.0) for k, _ in _lib.TrlQualityParams._fields_])
    fq = lambda frames=p, n=1, H=4, W=4, fo=p, boxes=p, pts=None, m=1, params=None, band=0, ws=p, wsb=4096, raw=p, feat=p, hist=None, st=p: \
        lib.trl_face_quality(frames, n, H, W, fo, boxes, pts, m, None if params is None else C.byref(params), band, ws, wsb, raw, feat, hist, st, None)
    bad = [fq(frames=None), fq(fo=None), fq(boxes=None), fq(raw=None), fq(feat=None), fq(st=None), fq(ws=None), fq(ws=p + 4), fq(wsb=1039),
           fq(m=-1), fq(m=2 ** 24 + 1), fq(n=-1), fq(H=0), fq(W=0), fq(H=16385), fq(W=16385), fq(band=-1), fq(m=0, band=-1),
           fq(params=prm(sharp_ref=0.0)), fq(params=prm(clip_ref=-1.0)), fq(params=prm(contrast_ref=float("nan"))),
           fq(params=prm(yaw_ref=float("inf"))), fq(params=prm(pitch_ref=0.0)), fq(m=0, params=prm(size_ref=0.0))]
    bu = lambda keys=p, groups=2, q=p, gid=p, m=1, base=0, faces=None, floats=0, best=None: \
        lib.trl_best_update(keys, groups, q, gid, m, base, faces, floats, best, None)
    bad += [bu(keys=None), bu(keys=p + 4), bu(groups=-1), bu(groups=2 ** 31), bu(q=None), bu(gid=None), bu(m=-1), bu(base=-1),
            bu(base=2 ** 31 - 1), bu(faces=p), bu(best=p), bu(faces=p, best=p, floats=0)]
    bad += [lib.trl_best_read(None, 2, p, p, None), lib.trl_best_read(p + 4, 2, p, p, None), lib.trl_best_read(p, -1, p, p, None),
            lib.trl_best_read(p, 2, None, p, None), lib.trl_best_read(p, 2, p, None, None)]
    assert all(b != 0 for b in bad) and len(set(bad)) == 1, bad
    assert b"trl_best_read" in lib.trl_last_error()
    # nothing to do is no error, and needs no device either
    assert fq(m=0) == 0 and fq(m=0, frames=None, fo=None, boxes=None, raw=None, feat=None, st=None, ws=None, wsb=0) == 0
    assert bu(m=0) == 0 and bu(m=0, q=None, gid=None) == 0 and bu(groups=0) == 0 and lib.trl_best_read(p, 0, None, None, None) == 0
    with pytest.raises(ValueError):
        truely_amd.QualityParams(sharp_ref=0.0)
    with pytest.raises(ValueError):
        truely_amd.QualityParams(yaw_ref=float("nan"))
    assert truely_amd.QualityParams().size_ref == 80.0
