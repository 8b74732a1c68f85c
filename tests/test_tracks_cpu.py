"""The face tracker without a GPU: tests/track_ref.py (the reference the GPU tests hold k_track_update to) against properties it
must have, against the drift state machine on one-face clips, csrc/trl_tracks.h -- the decisions of k_track_update -- built for the
host with sanitizers and run against that reference on every built clip, the dense clips (the reference against float64 and
rational arithmetic, and what each clip is meant to contain), and the ABI's host side."""
import itertools
import os
import re
import shutil
import subprocess
from fractions import Fraction

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


# ---- the dense clips: the conditions under which tests/test_gpu_tracks.py's dense tests mean anything ------------------------------
ULP = 2.0 ** -24
DENSE_WITH_EMB = tuple(n for n in T.DENSE if n != "dense8_emb_off")


@pytest.mark.parametrize("name", DENSE_WITH_EMB)
def test_dense_sims_against_float64(name):
    """Every similarity of the reference within 40 x 2^-24 of the float64 cosine.  A dot is 8 fma and 6 adds per element of the
    result, each norm the same, then two square roots, a product and a quotient: about 32 roundings of a value of magnitude <= 1
    to first order (the terms of a dot are all below the norms' product), and 40 leaves room for the second order.
    Largest errors measured, in units of 2^-24: dense8 3.9, dense_crowd 3.7, dense_drift 4.2."""
    e = T.dense_cases()[name]["emb"].astype(np.float64)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    err = np.abs(T.dense_sims(name).astype(np.float64) - e @ e.T).max() / ULP
    print(f"{name}: largest |sim - float64 cosine| = {err:.2f} x 2^-24 over {len(e) ** 2} pairs")
    assert err <= 40


def _exact_iou(a, b):
    """The IoU of two float32 boxes as a rational number."""
    a, b = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
    w, h = max(min(a[2], b[2]) - max(a[0], b[0]), 0), max(min(a[3], b[3]) - max(a[1], b[1]), 0)
    return w * h / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - w * h)


@pytest.mark.parametrize("name", T.DENSE)
def test_dense_ious_against_rationals(name):
    """Every IoU the reference looks at within a relative 20 x 2^-24 of the exact value: four differences, two areas, w, h (the
    differences again), inter, the sum and the difference of the denominator -- whose cancellation is bounded, inter being at most
    the smaller area -- and the quotient: 16 roundings to first order.  A pair that does not overlap gives exactly 0.
    Largest relative errors measured, in units of 2^-24: dense8 3.0, dense_crowd 4.2, dense_drift 3.0."""
    boxes = T.dense_cases()[name]["boxes"]
    worst = n = 0
    for _f, _id, trk, det, got, _sim, _key in T.dense_ref(name)["tracker"].log:
        want = _exact_iou(boxes[trk], boxes[det])
        if want == 0:
            assert got == 0
        else:
            worst, n = max(worst, abs(Fraction(float(got)) - want) / want), n + 1
    worst = float(worst) / ULP
    print(f"{name}: largest relative |iou - exact| = {worst:.2f} x 2^-24 over {n} overlapping pairs")
    assert n and worst <= 20


def test_tracks_header_equals_reference_on_dense_clips(tracks_program):
    """trl_tracks.h on the host, on every dense clip and gate variant: the header's IoU on boxes that are no integers, and its
    gates with a threshold on a computed value and on the value's two neighbours."""
    clips = []
    for name in T.DENSE + T.GATE_NAMES:
        c = T.dense_clip(name)
        clips.append((name, c["counts"], c["boxes"], T.dense_sims(name), c["iou_min"], c["sim_min"], c["max_age"], 1024))
    _run_program(tracks_program, clips)


def _frames_of(clip):
    return np.repeat(np.arange(len(clip["counts"])), clip["counts"])


def _id_at(clip, ref, person, frame):
    """The track of `person`'s detection in `frame`."""
    (row,) = np.flatnonzero((clip["person"] == person) & (_frames_of(clip) == frame))
    return int(ref["track"][row])


def test_dense_clips_have_no_exact_values():
    for name, c in T.dense_cases().items():
        assert not (c["boxes"] == np.round(c["boxes"])).any(), name
        if c["emb"] is not None:
            assert (c["emb"] != 0).all() and c["emb"].dtype == F32, name
        # the people of a frame stand in another order in the next
        order = [c["person"][_frames_of(c) == t].tolist() for t in range(len(c["counts"]))]
        assert sum(a != b for a, b in zip(order, order[1:])) >= len(order) // 2, name
    n2 = T.dot512(T.dense_cases()["dense8"]["emb"], T.dense_cases()["dense8"]["emb"])
    assert n2.min() < 2.0 ** -38 and n2.max() > 2.0 ** 38 and ((n2 > 0.5) & (n2 < 2)).any()


def test_dense8_contains_what_it_is_meant_to():
    c, r = T.dense_cases()["dense8"], T.dense_ref("dense8")
    log = r["tracker"].log
    iou_min, sim_min, max_age = F32(c["iou_min"]), F32(c["sim_min"]), c["max_age"]
    # pairs with a positive IoU, and those whose bits a contracted denominator would change
    positive = [e for e in log if e[4] > 0]
    changed = sum(bool(_bits(T.iou_contracted(c["boxes"][e[2]], c["boxes"][e[3]])) != _bits(e[4])) for e in positive)
    print(f"dense8: {len(positive)} pairs with a positive IoU, {changed} change under the contracted denominator")
    assert len(positive) >= 100 and changed >= 5
    # each gate rejects a pair that the other admits
    assert any(e[4] < iou_min and e[5] >= sim_min for e in log) and any(e[4] >= iou_min and e[5] < sim_min for e in log)
    # absences: exactly max_age frames -- the track goes on; max_age + 1 -- a new id.  Shorter ones go on as well.
    seen = set()
    for k, absent in T.DENSE8_ABSENT.items():
        gaps = [t for t in absent if t - 1 not in absent]
        for a in gaps:
            b = next(t for t in range(a, 99) if t not in absent)
            seen.add(b - a)
            assert (_id_at(c, r, k, a - 1) == _id_at(c, r, k, b)) == (b - a <= max_age), (k, a, b)
    assert {1, max_age, max_age + 1} <= seen and len(T.DENSE8_ABSENT) >= 2
    k, t = T.DENSE8_JUMP                                                             # the IoU gate alone ends a track
    assert _id_at(c, r, k, t - 1) != _id_at(c, r, k, t) == _id_at(c, r, k, t + 1)
    # apart from those, one track per person
    for k in set(range(8)) - set(T.DENSE8_ABSENT) - {T.DENSE8_JUMP[0]}:
        assert len(set(r["track"][c["person"] == k].tolist())) == 1, k


def test_dense8_emb_off_has_to_choose():
    r = T.dense_ref("dense8_emb_off")
    keys = {}
    for f, _id, _trk, det, _iou, _sim, key in r["tracker"].log:
        if key is not None:
            keys.setdefault((f, det), set()).add(float(key))
    assert sum(len(v) >= 2 for v in keys.values()) >= 24
    assert (r["sim"] == T.NO_SIM).all() and not r["flag"].any()


def test_dense_crowd_contains_what_it_is_meant_to():
    r = T.dense_ref("dense_crowd")
    tr, states = r["tracker"], r["states"]
    assert [b["head"][2] - a["head"][2] for a, b in zip(states, states[1:])] == [2, 2, 2, 2, 0] and tr.dropped == 8
    assert len(tr.evicted) >= 1 and all(s["slots"][:, 0].all() for s in states[1:])
    assert tr.next_id > 66 + 40                                                    # people dropped in one frame are strangers in the next
    assert (r["track"][:264].reshape(4, 66)[:, 64:] == -1).all()


def test_dense_drift_contains_what_it_is_meant_to():
    c, r = T.dense_cases()["dense_drift"], T.dense_ref("dense_drift")
    tr = r["tracker"]
    assert tr.next_id == 3
    ids = [_id_at(c, r, k, 0) for k in range(3)]
    sims = [r["sim"][(c["person"] == k) & (_frames_of(c) > 0)] for k in range(3)]
    assert (sims[0] >= F32(0.99)).all() and tr.table[ids[0]][3:5] == [0, 0]
    assert (sims[1] < F32(0.99)).any() and (sims[1] >= F32(0.99)).any()
    assert (sims[2] < F32(0.99)).all() and tr.table[ids[2]][3] == 39 and tr.table[ids[2]][4] >= 1
    sc, summary = tr.scores(160, 30)
    assert len(set(sc.tolist())) > 1 and summary[1] == ids[2]
    assert any(e[6] is not None and r["track"][e[3]] != e[1] for e in tr.log)      # admissible pairs of two people: the keys decided


@pytest.mark.parametrize("base,gate", T.GATES)
def test_gate_variants(base, gate):
    """A gate on a computed value: at the value and at its lower neighbour the pair matches (and the two clips' answers are the
    same), at the upper neighbour it does not, and a new track takes the detection.  An IoU gate stands on a value that a
    contracted denominator changes."""
    c, plain = T.dense_cases()[base], T.dense_ref(base)
    below, at, above = (T.dense_clip(f"{base}:{gate}:{side}") for side in T.SIDES)
    assert F32(below[gate]) < F32(at[gate]) < F32(above[gate])
    assert np.nextafter(F32(at[gate]), F32(0)) == below[gate] and np.nextafter(F32(at[gate]), F32(1)) == above[gate]
    det, trk = at["pair"]
    assert plain["track"][det] == plain["track"][trk]
    for side in T.SIDES:                                                           # the pair is looked at, with the gate's value
        log = T.dense_ref(f"{base}:{gate}:{side}")["tracker"].log
        (value,) = {int(_bits(e[4 if gate == "iou_min" else 5])) for e in log if (e[3], e[2]) == (det, trk)}
        assert value == int(_bits(at[gate])), side
    if gate == "iou_min":
        assert all(T.iou_contracted(c["boxes"][trk], c["boxes"][det], *form) != at[gate] for form in T.CONTRACTIONS)
        assert T.iou(c["boxes"][trk], c["boxes"][det]) == at[gate]
    r_below, r_at, r_above = (T.dense_ref(f"{base}:{gate}:{side}") for side in T.SIDES)
    assert r_below["track"][det] == r_below["track"][trk] and r_at["track"][det] == r_at["track"][trk]
    assert np.array_equal(r_below["track"], r_at["track"]) and np.array_equal(_bits(r_below["sim"]), _bits(r_at["sim"]))
    assert r_above["track"][det] != r_above["track"][trk] and r_above["tracker"].next_id > r_at["tracker"].next_id


def test_state_block_of_a_snapshot():
    """track_ref.state_block: the layout of csrc/trl_tracks.h, and which bytes a comparison leaves out."""
    c, r = T.dense_cases()["dense8"], T.dense_ref("dense8")
    buf, compared = T.state_block(r["states"][0], c["emb"])
    assert len(buf) == T.STATE_BYTES and compared.all() and not buf.view(np.int32).reshape(-1)[:8].any()
    words = buf[32:32 + 64 * 64].view(np.int32).reshape(64, 16)
    assert (words[:, 7] == -1).all() and not np.delete(words, 7, axis=1).any() and not buf[32 + 64 * 64:].any()
    snap = r["states"][-1]
    buf, compared = T.state_block(snap, c["emb"])
    words = buf[32:32 + 64 * 64].view(np.int32).reshape(64, 16)
    used, held = snap["slots"][:, 0] == 1, snap["slots"][:, 7] >= 0
    assert used.sum() == 8 and held.sum() > 8                                      # slots freed by ageing that keep their fields
    assert buf[:8].view(np.int64)[0] == 24 and buf[8:12].view(np.int32)[0] == r["tracker"].next_id
    blocks, cmp_blocks = buf[32 + 64 * 64:].view(F32).reshape(64, 512), compared[32 + 64 * 64:].reshape(64, 2048)
    for s in range(64):
        assert cmp_blocks[s].all() == (used[s] or not held[s]) and cmp_blocks[s].any() == cmp_blocks[s].all()
        if used[s]:
            row = snap["slots"][s, 7]
            assert np.array_equal(blocks[s], c["emb"][row]) and words[s, 12:13].view(F32)[0] == T.dot512(c["emb"][row], c["emb"][row])[0]
            assert np.array_equal(words[s, 8:12].view(F32), c["boxes"][row])
        elif not held[s]:
            assert not blocks[s].any()
    assert compared[:32 + 64 * 64].all()


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
