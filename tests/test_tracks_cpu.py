"""The face tracker without a GPU: tests/track_ref.py (the reference the GPU tests hold k_track_update to) against properties it
must have, against the drift state machine on one-face clips, csrc/trl_tracks.h -- the decisions of k_track_update -- built for the
host with sanitizers and run against that reference on every built clip, and the ABI's host side."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import drift_ref as D
import track_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "truely-real-time-ai-generated-video-detection-framework-for-social-platforms_amd", "csrc")
F32 = np.float32


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


# ---- the reference's arithmetic ---------------------------------------------------------------------------------------------------
def test_dot512_equals_the_oracle(oracle):
    rng = np.random.default_rng(0)
    a = rng.standard_normal((40, 512)).astype(F32)
    b = (rng.standard_normal((40, 512)) * rng.choice([1e-3, 1.0, 1e3], (40, 1))).astype(F32)
    b[3] = a[3]
    a[5] = 0
    got = T.dot512(a, b)
    want = np.array([oracle.dot512(x, y) for x, y in zip(a, b)], F32)
    assert np.array_equal(_bits(got), _bits(want))
    for kind in ("zero", "nan_elem", "inf_elem", "sim_pos_inf", "scaled_up"):      # rows that are no ordinary numbers
        emb, _ = D.special_rows()[kind]
        k = D.SPECIAL_AT
        got = T.dot512(emb[k - 1:k + 1], emb[k:k + 2])
        want = np.array([oracle.dot512(emb[k - 1], emb[k]), oracle.dot512(emb[k], emb[k + 1])], F32)
        assert np.array_equal(got, want, equal_nan=True), kind


def test_iou_is_the_known_fraction():
    a = T.grid_box(0, 0)
    assert T.iou(a, a) == 1 and T.iou(a, T.grid_box(20, 0)) == 0 and T.iou(a, T.grid_box(10, 0)) == 0
    assert T.iou(a, T.grid_box(6, 0)) == F32(F32(40) / F32(160))
    assert T.iou(a, T.grid_box(0, 0, 12, 12)) == F32(F32(100) / F32(144))
    assert np.isnan(T.iou([5, 5, 5, 9], [5, 5, 5, 9])) and T.iou(a, [5, 5, 5, 9]) == 0


# ---- properties of the reference --------------------------------------------------------------------------------------------------
def _random_clip(rng, frames, most, values):
    """Equal boxes, and a table of pair similarities drawn from `values`: the keys alone decide."""
    counts = rng.integers(0, most + 1, frames).astype(np.int32)
    m = int(counts.sum())
    boxes = np.tile(np.array(T.grid_box(0, 0), F32), (m, 1))
    sims = rng.choice(np.array(values, F32), (m, m))
    return counts, boxes, sims


VALUES = (-0.0, 0.0, 0.5, 0.5, 1.0, float("nan"), -1.0, 0.25, 0.25)


def _all_clips():
    for name, c in T.cases().items():
        yield name, c["counts"], T.run_clip(c["counts"], c["boxes"], c["emb"], c["iou_min"], c["sim_min"], c["max_age"])
    rng = np.random.default_rng(7)
    for i in range(20):
        counts, boxes, sims = _random_clip(rng, 12, 6, VALUES)
        yield f"random{i}", counts, T.run_clip(counts, boxes, None, 0.0, (-np.inf, 0.25)[i % 2], (0, 1, T.INT32_MAX)[i % 3], sims=sims)


def test_ids_are_dense_and_no_track_is_shared():
    for name, counts, r in _all_clips():
        track, off, seen = r["track"], 0, -1
        for c in counts:
            row = track[off:off + c]
            live = row[row >= 0]
            assert len(set(live.tolist())) == len(live), name                     # no two detections of a frame share a track
            assert (row[:T.SLOTS] >= 0).all() and (row[T.SLOTS:] == -1).all(), name
            for t in row:                                                         # a new id is the next integer
                if t > seen:
                    assert t == seen + 1, name
                    seen = t
            off += c
        assert seen + 1 == r["tracker"].next_id, name
        tab = r["tracker"].table_array()
        assert (tab[:, 2] == np.bincount(track[track >= 0], minlength=len(tab))).all(), name   # n_obs counts the track's rows


def _stable_matchings(keys):
    """Every matching of the admissible pairs in which each pair outside it is blocked: it shares its track or its detection with
    a pair of the matching that comes before it in the order.  (The greedy matching is one: a pair it passes over was unavailable
    when its turn came.  There is no other: the first pair of the order blocks or belongs, and so on by induction.)"""
    order = lambda p: (-float(keys[p]) + 0.0, p[0], p[1])
    pairs, out = list(keys), []
    for r in range(len(pairs) + 1):
        for sub in itertools.combinations(pairs, r):
            if len({p[0] for p in sub}) < r or len({p[1] for p in sub}) < r:
                continue
            if all(any(order(q) < order(p) and (q[0] == p[0] or q[1] == p[1]) for q in sub) for p in pairs if p not in sub):
                out.append({p[1]: p[0] for p in sub})
    return out


def test_greedy_equals_brute_force_on_small_matrices():
    rng = np.random.default_rng(3)
    for trial in range(300):
        nt, nd = rng.integers(1, 4, 2)
        ids = rng.permutation(6)[:nt]
        keys = {}
        for t in ids:
            for d in range(nd):
                k = rng.choice(np.array(VALUES, F32))
                if not np.isnan(k):
                    keys[(int(t), d)] = k
        stable = _stable_matchings(keys)
        assert stable == [T.greedy(keys)], (trial, keys)


# ---- one face per frame: the drift state machine ----------------------------------------------------------------------------------
def _one_face(emb, valid, frame_count, fps=30):
    n = len(valid)
    emb = np.asarray(emb, F32)[np.asarray(valid, bool)]
    boxes = np.tile(np.array(T.grid_box(3, 4), F32), (len(emb), 1))
    r = T.run_clip(np.asarray(valid, np.int32), boxes, emb, 0.0, -np.inf, T.INT32_MAX, lazy=True)
    tr = r["tracker"]
    # drift_ref's side: the similarity of every valid frame with the last valid one before it
    prev = D.pair_index(valid)
    sims = np.full(n, T.NO_SIM, F32)
    full = np.zeros((n, 512), F32)
    full[np.asarray(valid, bool)] = emb
    for i in np.flatnonzero(prev >= 0):
        sims[i] = T.cosine(T.dot512(full[i], full[prev[i]])[0], T.dot512(full[i], full[i])[0], T.dot512(full[prev[i]], full[prev[i]])[0])
    flags, run, hits = D.state_machine(D.per_frame(sims, valid))
    v = np.asarray(valid, bool)
    assert tr.next_id == 1 and (r["track"] == 0).all()
    assert np.array_equal(_bits(r["sim"]), _bits(sims[v])) and np.array_equal(r["flag"], flags[v])
    assert tr.table[0][3:5] == [run, hits] and tr.table[0][2] == int(v.sum())
    sc, summary = tr.scores(frame_count, fps)
    assert sc[0] == D.score(hits, run, frame_count, fps)[0] and summary[:2] == [sc[0], 0]
    return run, hits


def test_one_face_is_the_drift_state_machine():
    for h, r in ((0, 0), (3, 16), (5, 2), (20, 30), (0, 15)):
        emb, valid = D.onehot_sequence(h, r)
        assert _one_face(emb, valid, len(valid) * 4) == (r, h)
    emb, valid = D.onehot_rows([D.DRIFT] * 17 + [D.NOFACE, D.NOFACE, D.DRIFT, D.SAME, D.NOFACE] + [D.DRIFT] * 20)
    _one_face(emb, valid, 400)
    pairs, _ = D.threshold_sweep()
    emb, valid = D.sweep_rows(pairs[384:417])                                      # the 33 pairs around 0.99f: both sides of it
    run, hits = _one_face(emb, valid, len(valid) * 4)
    s = np.array([T.cosine(T.dot512(p[1], p[0])[0], T.dot512(p[1], p[1])[0], T.dot512(p[0], p[0])[0]) for p in pairs[384:417]], F32)
    assert (s < F32(0.99)).any() and (s == F32(0.99)).any() and (s > F32(0.99)).any()


# ---- csrc/trl_tracks.h on the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tracks_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("tracks") / "tracks")
    base = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "tracks_main.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(base + san, capture_output=True, text=True).returncode != 0:
        subprocess.run(base, check=True)
    return out


def _hex(a):
    return " ".join(f"{int(v):08x}" for v in _bits(a).ravel())


def _run_program(program, clips):
    """clips: (name, counts, boxes, sims | None, iou_min, sim_min, max_age, table_cap).  Each equals track_ref."""
    script = []
    for _name, counts, boxes, sims, iou_min, sim_min, max_age, cap in clips:
        m = len(boxes)
        script.append(f"{int(sims is not None)} {_hex([iou_min])} {_hex([sim_min])} {max_age} {cap} {len(counts)} {m}")
        script.append(" ".join(str(int(c)) for c in counts))
        script += [_hex(b) for b in boxes]
        if sims is not None:
            script += [_hex(row) for row in sims]
    r = subprocess.run([program], input="\n".join(script) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = iter(r.stdout.splitlines())
    for name, counts, boxes, sims, iou_min, sim_min, max_age, cap in clips:
        want = T.run_clip(counts, boxes, None, iou_min, sim_min, max_age, table_cap=cap, sims=sims)
        tr = want["tracker"]
        for i in range(len(boxes)):
            track, bits, flag = next(lines).split()
            assert (int(track), int(bits, 16), int(flag)) == (want["track"][i], int(_bits(want["sim"][i])), want["flag"][i]), (name, i)
        assert [int(v) for v in next(lines).split()] == [tr.next_id, tr.dropped, tr.table_overflow], name
        tab = tr.table_array(min(cap, tr.next_id))
        for row in tab:
            assert [int(v) for v in next(lines).split()] == row.tolist(), name
    assert next(lines, None) is None


def test_tracks_header_equals_reference(tracks_program):
    """trl_tracks.h composed as in k_track_update, on every built clip (with the clip's table of all pair similarities from the
    reference's dot512) and on random key tables with ties, -0 / +0 and NaN; with a table that holds every id and one that does not."""
    clips = []
    for name, c in T.cases().items():
        sims = None if c["emb"] is None else T.pair_sims(c["emb"])
        for cap in (1024, 3, 0):
            clips.append((name, c["counts"], c["boxes"], sims, c["iou_min"], c["sim_min"], c["max_age"], cap))
    rng = np.random.default_rng(11)
    for i in range(40):
        counts, boxes, sims = _random_clip(rng, 12, (6, 6, 70)[i % 3] if i < 6 else 6, VALUES)
        clips.append((f"random{i}", counts, boxes, sims, 0.0, (-np.inf, 0.25)[i % 2], (0, 1, T.INT32_MAX)[i % 3], 4096))
    _run_program(tracks_program, clips)


def test_cases_do_what_they_are_meant_to():
    c = T.cases()
    run = lambda n, **kw: T.run_clip(c[n]["counts"], c[n]["boxes"], c[n]["emb"], c[n]["iou_min"], c[n]["sim_min"], c[n]["max_age"], **kw)
    r = run("alternate2")
    assert r["track"].reshape(-1, 2).tolist() == [[0, 1] if t % 2 == 0 else [1, 0] for t in range(24)]     # the first row changes person
    assert run("alternate3")["tracker"].next_id == 3
    assert run("crossing_sim")["track"].tolist() == [0, 1] * 8                                          # follows the faces
    assert run("crossing_iou")["track"].tolist() == [0, 1] * 3 + [1, 0] * 3 + [0, 1] * 2                # follows the boxes
    assert run("crossing_gate")["tracker"].next_id == 4
    assert run("ties")["track"].tolist() == [0, 1, 0, 1, 2, 0, 1, 2, 3, 4, 0, 1, 0, 1, 5, 6, 7]
    r = run("turnover")["tracker"]
    assert r.evicted[:40] == list(range(32)) + list(range(32, 40)) and len(r.evicted) == 104            # last seen earliest, then by id
    assert run("counts_63_64_65")["tracker"].dropped == 3 and run("crowd64")["tracker"].next_id == 64
    assert run("age2")["track"].tolist()[:9] == [0, 1, 1, 1, 0, 1, 1, 1, 1] and run("age2")["tracker"].next_id == 5
    assert run("age_never")["tracker"].next_id == 2
    r = run("drifters")["tracker"]
    assert [r.table[i][3:5] for i in range(3)] == [[0, 0], [39, 24], [39, 24]] and r.scores(160, 30)[1] == [90, 1, 3, 0]
    assert run("slot_reuse")["tracker"].table[2][5] == -1 and run("slot_reuse")["tracker"].table_array()[2, 0] == 2


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_tracker():
    from truely_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "truely_hip.h")).read()
    names = {"trl_track_update", "trl_track_scores"}
    assert names <= set(re.findall(r"\b(trl_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.EXPORTS)
    assert "#define TRL_ABI_VERSION 7\n" in hdr
    assert re.search(r"#define TRL_TRACK_SLOTS (\d+)", hdr).group(1) == str(T.SLOTS)
    assert re.search(r"#define TRL_TRACK_STATE_BYTES (\d+)", hdr).group(1) == str(T.STATE_BYTES)
    lib = _lib.load()
    assert lib.trl_abi_version() == 7
    # bad arguments are refused before anything is queued (no device is touched)
    assert lib.trl_track_update(None, None, None, 0, 0, None, 0.0, 0.0, 0, None, None, None, None, 0, None) != 0
    assert b"trl_track_update" in lib.trl_last_error()
    assert lib.trl_track_update(None, None, None, -1, 0, None, 0.0, 0.0, 0, None, None, None, None, 0, None) != 0
    assert lib.trl_track_scores(None, None, 0, 0, 30, None, None, None) != 0
