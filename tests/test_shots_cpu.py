"""Shot boundaries without a GPU: tests/shots_ref.py (the reference the GPU tests hold the kernels to) against independent
computations -- np.bincount, np.cumsum, worked examples --, csrc/trl_shots.h and the cut rule of csrc/trl_tracks.h built for the
host (plain, and with the sanitizers; a stand-alone program, run as a program) and held to the reference bit for bit, and the ABI's
host side."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import shots_ref as S
import track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc")
F32 = np.float32


# ---- the reference against independent computations -------------------------------------------------------------------------------------
def test_counts_are_bincounts():
    for H, W in S.SIZES[:4]:
        fr = S.content_frames("noise", 1, H, W)[0]
        sig = S.signature(fr)
        assert np.array_equal(sig, S.signature_fast(fr))
        eh, ew = S.edges(H), S.edges(W)
        for i in range(4):
            for j in range(4):
                for c in range(3):
                    want = np.bincount(fr[eh[i]:eh[i + 1], ew[j]:ew[j + 1], c].reshape(-1) // 8, minlength=32)
                    assert np.array_equal(sig[4 * i + j, c], want), (H, W, i, j, c)
        assert np.array_equal(sig.sum(-1), np.repeat(S.region_pixels(H, W)[:, None], 3, 1))
    for kind in S.CONTENTS:
        fr = S.content_frames(kind, 2, 23, 37)
        assert all(np.array_equal(S.signature(f), S.signature_fast(f)) for f in fr), kind


def test_region_borders():
    assert S.edges(23) == [0, 5, 11, 17, 23] and S.edges(37) == [0, 9, 18, 27, 37]
    assert S.region_pixels(4, 4).tolist() == [1] * 16
    assert S.signature(S.content_frames("noise", 1, 4, 4)[0]).sum(-1).tolist() == [[1, 1, 1]] * 16
    for H, W in ((23, 37), (5, 7), (64, 64)):
        f = S.sixteen_constants(H, W)
        sig, N = S.signature(f), S.region_pixels(H, W)
        for r in range(16):
            for c in range(3):
                assert np.flatnonzero(sig[r, c]).tolist() == [(16 * r + 5 * c) >> 3] and sig[r, c].max() == N[r], (H, W, r, c)
    assert S.region_pixels(23, 37).sum() == 23 * 37 and S.region_pixels(23, 37)[0] == 5 * 9 and S.region_pixels(23, 37)[15] == 6 * 10


def test_distance_is_the_cumulative_l1():
    rng = np.random.default_rng(3)
    H, W = 23, 37
    a, b = S.signatures(S.content_frames("noise", 2, H, W))
    d = S.region_distances(a, b)
    want = np.abs(np.cumsum(a.astype(np.int64), -1) - np.cumsum(b.astype(np.int64), -1))[:, :, :31].sum((1, 2))
    assert d == want.tolist()
    N = S.region_pixels(H, W)
    for drop in (0, 1, 4, 15):
        keep = np.lexsort((np.arange(16), want))[:16 - drop]
        assert S.distance(a, b, H, W, drop) == F32(want[keep].sum() / (93.0 * N[keep].sum()))
        assert S.distance(a, a, H, W, drop) == 0.0 and not np.signbit(S.distance(a, a, H, W, drop))
    pairs = {name: (x, y) for name, x, y in S.built_signature_pairs(H, W)}
    assert S.distance(*pairs["extreme"], H, W, 0) == 1.0 and S.distance(*pairs["extreme_swapped"], H, W, 0) == 1.0
    assert S.distance(*pairs["equal"], H, W, 0) == 0.0
    # one changed region: dropped with drop >= 1, and alone it weighs 93 N_5 of 93 H W
    assert S.distance(*pairs["one_region"], H, W, 0) == F32(N[5] / (H * W))
    assert all(S.distance(*pairs["one_region"], H, W, drop) == 0.0 for drop in (1, 4, 15))
    del rng


def test_ties_go_by_region_index():
    H = W = 64                                                  # every N_r is 256
    pairs = {name: (x, y) for name, x, y in S.built_signature_pairs(H, W)}
    a, b = pairs["pairs_tied"]
    d = S.region_distances(a, b)
    assert d == [3 * 256 * (1 + (r // 2) % 3) for r in range(16)]
    for drop in (0, 1, 4, 15):
        # regions with d = 3 N: 0 1 6 7 12 13; 6 N: 2 3 8 9 14 15; 9 N: 4 5 10 11 -- by (d, r)
        order = [0, 1, 6, 7, 12, 13, 2, 3, 8, 9, 14, 15, 4, 5, 10, 11][:16 - drop]
        assert S.distance(a, b, H, W, drop) == F32(sum(d[r] for r in order) / (93.0 * 256 * len(order))), drop
    # where N_r differ, equal d_r with different N_r: the tie's order decides the denominator
    H, W = 23, 37
    N = S.region_pixels(H, W)
    a = np.zeros((16, 3, 32), np.int32)
    a[:, :, 0] = N[:, None]
    b = a.copy()
    for r in (3, 12):                                           # N_3 = 50, N_12 = 54: move 10 pixels of one channel one bin up
        b[r, 0, 0] -= 10
        b[r, 0, 1] += 10
    assert N[3] != N[12] and S.region_distances(a, b)[3] == S.region_distances(a, b)[12] == 10
    assert S.distance(a, b, H, W, 1) == F32(10 / (93.0 * (N.sum() - N[12])))      # region 12 is the one dropped
    assert S.distance(a, b, H, W, 15) == 0.0 and S.distance(a, b, H, W, 14) == 0.0


def test_cut_rule():
    thr = F32(0.12)
    below = np.nextafter(thr, F32(0))
    dist = np.array([2.0, 0.5, thr, below, 0.0, 0.5, 0.5, 0.0, 0.5, 0.5, 0.5], F32)
    cut, shot = S.scan(dist, thr, 1)
    assert cut.tolist() == [0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1] and shot.tolist() == np.cumsum(cut).tolist()
    # a flash: frames 5 and 6 both differ from their predecessors; min_shot = 2 keeps the second from cutting, 3 the third
    assert S.scan(dist, thr, 2)[0].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    assert S.scan(dist, thr, 3)[0].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0]
    # the first cut is never suppressed, however large min_shot; the first frame is never a cut, whatever the threshold
    assert S.scan(dist, thr, 1000)[0].tolist() == [0, 1] + [0] * 9
    assert S.scan(dist, -1.0, 1)[0].tolist() == [0] + [1] * 10 and S.scan(dist, 3.0, 1)[0].sum() == 0
    assert S.scan(np.array([2.0, 2.0], F32), 0.0, 1)[0].tolist() == [0, 0]


def test_scene_clip_has_its_cuts():
    frames, starts = S.scene_clip()
    sh = S.Shots(frames.shape[1], frames.shape[2])
    out = sh.update(S.signatures(frames))
    assert np.flatnonzero(out["cut"]).tolist() == starts and out["shot"][-1] == 2 and out["dist"][0] == 2.0
    inside = np.delete(out["dist"], [0] + starts)
    assert inside.max() < 0.06 and out["dist"][starts].min() > 0.15     # (what the clip is built to be, not a calibration)


def test_cut_tracking_reference_is_the_plain_tracker_without_cuts():
    for name, (clip, cuts) in S.cut_clips().items():
        none = S.track_with_cuts(clip["counts"], clip["boxes"], clip["emb"], np.zeros_like(cuts), clip["iou_min"], clip["sim_min"], clip["max_age"])
        r = T.run_clip(clip["counts"], clip["boxes"], clip["emb"], clip["iou_min"], clip["sim_min"], clip["max_age"], lazy=True)
        assert np.array_equal(none["track"], r["track"]) and np.array_equal(none["table"], r["tracker"].table_array()), name
        got = S.track_with_cuts(clip["counts"], clip["boxes"], clip["emb"], cuts, clip["iou_min"], clip["sim_min"], clip["max_age"])
        if name == "clip_start":
            assert np.array_equal(got["track"], r["track"]) and np.array_equal(got["table"], none["table"])
        else:
            assert got["next_id"] > none["next_id"], name
    clip, cuts = S.cut_clips()["one_face_drift"]
    got = S.track_with_cuts(clip["counts"], clip["boxes"], clip["emb"], cuts)
    assert got["track"].tolist() == [0] * 20 + [1] * 22 + [2] * 18
    assert got["table"][:, 3].tolist() == [19, 21, 17] and got["table"][:, 4].tolist() == [4, 6, 2]      # run, hits per shot


# ---- csrc/trl_shots.h on the host ---------------------------------------------------------------------------------------------------------
def _compile(tmp, sanitize: bool):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp / ("shots_san" if sanitize else "shots"))
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(ROOT, "tests", "shots_main.cpp"),
           "-o", out]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and sanitize:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def shots_program(request, tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("shots"), request.param == "sanitized")


def _run(program, path, script):
    r = subprocess.run([program, str(path)], input=script, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return r.stdout.splitlines()


def _hex(v):
    return f"{int(np.array(v, F32).view(np.uint32)):08x}"


def test_header_signatures_equal_reference(shots_program, tmp_path):
    for H, W in S.SIZES[:4]:
        frames = np.concatenate([S.content_frames(kind, 1, H, W) for kind in S.CONTENTS])
        path = tmp_path / f"f{H}x{W}.bin"
        path.write_bytes(frames.tobytes())
        bands = (1, 2, 3, 7, H)
        lines = _run(shots_program, path, "".join(f"S {len(frames)} {H} {W} {b}\n" for b in bands))
        want = S.signatures(frames).reshape(len(frames), -1)
        assert len(lines) == len(bands) * len(frames)
        for k, line in enumerate(lines):
            assert [int(v) for v in line.split()] == want[k % len(frames)].tolist(), (H, W, bands[k // len(frames)], k % len(frames))


def test_header_distance_equals_reference(shots_program, tmp_path):
    (tmp_path / "none.bin").write_bytes(b"")
    cases = []
    for H, W in ((23, 37), (64, 64)):
        sigs = S.signatures(np.concatenate([S.content_frames(kind, 2, H, W) for kind in ("noise", "ramp_x", "checker", "sixteen")]))
        pairs = [(f"frames{i}", sigs[i], sigs[i + 1]) for i in range(len(sigs) - 1)] + S.built_signature_pairs(H, W)
        cases += [(H, W, drop, name, a, b) for name, a, b in pairs for drop in ((0, 1, 4, 15) if name.startswith("frames") else range(16))]
    script = "".join(f"D {H} {W} {drop}\n{' '.join(map(str, a.reshape(-1)))}\n{' '.join(map(str, b.reshape(-1)))}\n" for H, W, drop, _, a, b in cases)
    lines = _run(shots_program, tmp_path / "none.bin", script)
    assert len(lines) == len(cases)
    for (H, W, drop, name, a, b), line in zip(cases, lines):
        assert line == _hex(S.distance(a, b, H, W, drop)), (H, W, drop, name)


def _windows(n):
    rng = np.random.default_rng(n)
    yield [n]
    yield [1] * n
    yield [0, 2, 0, 0, 7, n - 9, 0]
    for _ in range(3):
        cuts = sorted(rng.integers(0, n + 1, 5).tolist())
        yield [b - a for a, b in zip([0] + cuts, cuts + [n])]


def test_header_cut_scan_equals_reference_for_any_windows(shots_program, tmp_path):
    frames, starts = S.scene_clip()
    n, H, W = frames.shape[:3]
    # a flash: frame 20 is white
    flash = frames.copy()
    flash[20] = 255
    sigs = {"scenes": S.signatures(frames), "flash": S.signatures(flash)}
    for clip, fr in (("scenes", frames), ("flash", flash)):
        path = tmp_path / f"{clip}.bin"
        path.write_bytes(fr.tobytes())
        plain = S.Shots(H, W).update(sigs[clip])
        at = float(plain["dist"][starts[0]])                    # a threshold that IS a distance of the clip, and the float below it
        for thr, drop, min_shot in ((0.12, 4, 1), (0.12, 4, 2), (0.12, 0, 3), (at, 4, 1), (float(np.nextafter(F32(at), F32(2))), 4, 1), (0.0, 15, 1)):
            ref = S.Shots(H, W, thr, drop, min_shot).update(sigs[clip])
            cut, shot = S.scan(ref["dist"], thr, min_shot)
            assert np.array_equal(cut, ref["cut"]) and np.array_equal(shot, ref["shot"])
            want = [f"{_hex(d)} {c} {s}" for d, c, s in zip(ref["dist"], ref["cut"], ref["shot"])]
            for w in _windows(n):
                lines = _run(shots_program, path, f"U {n} {H} {W} {_hex(thr)} {drop} {min_shot} {len(w)} {' '.join(map(str, w))}\n")
                assert lines[:-1] == want, (clip, thr, drop, min_shot, w)
                last = np.flatnonzero(ref["cut"])
                assert [int(v) for v in lines[-1].split()][::2] == [n, int(ref["cut"].sum())]
                assert last.size == 0 or int(lines[-1].split()[1]) == last[-1]
        if clip == "scenes":
            ref = S.Shots(H, W, at, 4, 1).update(sigs[clip])
            assert ref["cut"][starts[0]] == 1                   # dist == threshold cuts ...
            assert S.Shots(H, W, np.nextafter(F32(at), F32(2)), 4, 1).update(sigs[clip])["cut"][starts[0]] == 0      # ... the float below does not
        else:
            ref = S.Shots(H, W).update(sigs[clip])
            assert ref["cut"][20] == 1 and ref["cut"][21] == 1 and S.Shots(H, W, min_shot=2).update(sigs[clip])["cut"][20:22].tolist() == [1, 0]


def test_header_cut_tracks_equal_the_per_shot_reference(shots_program, tmp_path):
    (tmp_path / "none.bin").write_bytes(b"")
    for name, (clip, cuts) in S.cut_clips().items():
        for emb_on in (True, False):
            emb = clip["emb"] if emb_on and name != "crowd" else None      # (the table of all pair similarities: small clips only)
            m = len(clip["boxes"])
            script = [f"T {int(emb is not None)} {_hex(clip['iou_min'])} {_hex(clip['sim_min'])} {clip['max_age']} {len(cuts)} {m}"]
            script += [f"{int(c)} {int(k)}" for c, k in zip(clip["counts"], cuts)]
            script += [" ".join(_hex(v) for v in b) for b in clip["boxes"]]
            if emb is not None:
                script += [" ".join(_hex(v) for v in row) for row in T.pair_sims(emb)]
            lines = _run(shots_program, tmp_path / "none.bin", "\n".join(script) + "\n")
            ref = S.track_with_cuts(clip["counts"], clip["boxes"], emb, cuts, clip["iou_min"], clip["sim_min"], clip["max_age"])
            got = [ln.split() for ln in lines[:m]]
            assert [int(g[0]) for g in got] == ref["track"].tolist(), (name, emb_on)
            assert [g[1] for g in got] == [_hex(v) for v in ref["sim"]], (name, emb_on)
            assert [int(g[2]) for g in got] == ref["flag"].tolist(), (name, emb_on)
            assert [int(v) for v in lines[m].split()] == [ref["next_id"], ref["dropped"]], (name, emb_on)
            assert [[int(v) for v in ln.split()] for ln in lines[m + 1:]] == ref["table"].tolist(), (name, emb_on)


# ---- the ABI's host side ------------------------------------------------------------------------------------------------------------------
def test_abi_rejections_need_no_device():
    import truely_amd
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_shots_workspace", "trl_frame_signatures", "trl_signature_distance", "trl_shots_update", "trl_track_update_cuts"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    section = hdr[hdr.index("---- Shots"):]
    assert "PLACEHOLDERS" in section and "dissolves" in section and "15 bytes" in section
    assert all(hasattr(truely_amd, n) for n in ("frame_signatures", "signature_distance", "ShotParams", "ShotDetector", "detect_shots"))
    lib = _lib.load()
    assert lib.trl_abi_version() == 7
    ws = lib.trl_shots_workspace
    assert ws(1, 720, 1280, 0) > 0 and ws(0, 720, 1280, 0) == ws(1, 720, 1280, 0) and ws(256, 720, 1280, 0) >= 256 * 4 * 1536
    assert ws(1, 4, 4, 0) == 4 * 1536 and ws(1, 64, 64, 1) == 16 * 4 * 1536 and ws(1, 64, 64, 16) == 4 * 1536
    assert [ws(-1, 8, 8, 0), ws(65536, 8, 8, 0), ws(1, 3, 8, 0), ws(1, 8, 3, 0), ws(1, 16385, 8, 0), ws(1, 8, 16385, 0), ws(1, 8, 8, -1)] == [0] * 7
    buf = (C.c_longlong * 8192)()
    p = C.addressof(buf)
    fs = lambda frames=p, n=1, H=8, W=8, band=0, ws=p, wsb=65536, sig=p: lib.trl_frame_signatures(frames, n, H, W, band, ws, wsb, sig, None)
    bad = [fs(frames=None), fs(sig=None), fs(ws=None), fs(ws=p + 4), fs(wsb=4 * 1536 * 2 - 1), fs(n=-1), fs(n=65536), fs(H=3), fs(W=3), fs(H=16385),
           fs(W=16385), fs(band=-1), fs(n=0, band=-1), fs(n=0, H=3)]
    sd = lambda a=p, b=p, pairs=1, H=8, W=8, drop=4, dist=p: lib.trl_signature_distance(a, b, pairs, H, W, drop, dist, None)
    bad += [sd(a=None), sd(b=None), sd(dist=None), sd(pairs=-1), sd(H=3), sd(W=16385), sd(drop=-1), sd(drop=16), sd(pairs=0, drop=16)]
    prm = lambda threshold=0.12, drop=4, min_shot=1: _lib.TrlShotsParams(threshold, drop, min_shot)
    su = lambda state=p, sig=p, n=1, H=8, W=8, params=None, dist=p, cut=p, shot=p: \
        lib.trl_shots_update(state, sig, n, H, W, None if params is None else C.byref(params), dist, cut, shot, None)
    bad += [su(state=None), su(state=p + 4), su(sig=None), su(dist=None), su(cut=None), su(shot=None), su(n=-1), su(H=3), su(W=3), su(H=16385),
            su(params=prm(threshold=float("nan"))), su(params=prm(threshold=float("inf"))), su(params=prm(threshold=float("-inf"))),
            su(params=prm(drop=-1)), su(params=prm(drop=16)), su(params=prm(min_shot=0)), su(n=0, params=prm(min_shot=0)), su(n=0, state=None)]
    tc = lambda state=p, boxes=p, counts=p, cut=p, n=1, m=1, emb=None, iou=0.1, sim=0.4, age=3, track=p, s=p, flag=p, table=p, cap=1: \
        lib.trl_track_update_cuts(state, boxes, counts, cut, n, m, emb, iou, sim, age, track, s, flag, table, cap, None)
    bad += [tc(state=None), tc(state=p + 4), tc(n=-1), tc(m=-1), tc(age=-1), tc(cap=-1), tc(iou=float("nan")), tc(counts=None), tc(boxes=None),
            tc(track=None), tc(table=None)]
    assert all(b != 0 for b in bad) and len(set(bad)) == 1, bad
    assert b"trl_track_update_cuts" in lib.trl_last_error()
    # nothing to do is no error, and needs no device either
    assert fs(n=0) == 0 and fs(n=0, frames=None, sig=None, ws=None, wsb=0) == 0
    assert sd(pairs=0) == 0 and sd(pairs=0, a=None, b=None, dist=None) == 0
    assert su(n=0) == 0 and su(n=0, sig=None, dist=None, cut=None, shot=None) == 0
    for kw in (dict(threshold=float("nan")), dict(drop=16), dict(drop=-1), dict(min_shot=0)):
        with pytest.raises(ValueError):
            truely_amd.ShotParams(**kw)
    d = truely_amd.ShotParams()
    assert (d.threshold, d.drop, d.min_shot) == (0.12, 4, 1) == tuple(S.DEFAULTS.values())
