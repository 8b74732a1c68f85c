"""The drift state machine without a GPU.  tests/test_gpu_drift.py holds the kernels to the oracle (bit for bit) and to
tests/drift_ref.py (a transcription of server/model.py:60-95); this file holds the ORACLE to that transcription on the same built
inputs, and asserts the properties of those inputs that make the GPU tests mean something.

The float32 similarity against the float64 cosine, for rows whose norms lie in [0.5, 2] (u = 2^-24, first order):
    a dot is 8 fma and 6 adds deep (oracle/trl_oracle.c orc_dot512: 8 elements per lane, a 64-lane tree), so its error is at most
    14u * sum|a_i b_i| <= 14u * |a||b|, i.e. 14u relative to the denominator; each norm carries 14u / 2 = 7u from its dot and u
    from the square root; the product of the norms and the division add u each:  14 + 2 * 8 + 2 = 32u = 1.91e-6."""
import numpy as np
import pytest

import drift_ref as D

F32 = np.float32


def check_oracle(oracle, emb, valid, frame_count=None, fps=30):
    """oracle.drift_score against the transcription run on the oracle's own similarities; the similarities against cos64."""
    n = len(valid)
    ref = oracle.drift_score(emb, valid, n * 4 if frame_count is None else frame_count, fps)
    sims = ref["sims"]
    per = D.per_frame(sims, valid)
    none = np.array([p is None for p in per], bool)
    assert np.array_equal(sims == F32(2.0), none)                    # 2.0 exactly where model.py makes no comparison
    flags, run, hits = D.state_machine(per)
    assert np.array_equal(ref["flags"], flags) and (ref["run"], ref["hits"]) == (run, hits)
    assert ref["score"] == D.score(hits, run, ref_frame_count(n, frame_count), fps)[0]
    prev = D.pair_index(valid)
    norms = np.linalg.norm(np.asarray(emb, np.float64), axis=1)
    worst = 0.0
    for i in np.flatnonzero(~none):
        c = D.cos64(emb[i], emb[prev[i]])
        assert np.isnan(sims[i]) == np.isnan(c), (i, sims[i], c)
        if 0.5 <= norms[i] <= 2 and 0.5 <= norms[prev[i]] <= 2:
            worst = max(worst, abs(float(sims[i]) - c))
    assert worst <= D.BOUND, worst
    return ref


def ref_frame_count(n, frame_count):
    return n * 4 if frame_count is None else frame_count


def test_threshold_is_the_same_in_float32_and_float64():
    t = F32(0.99)
    assert float(t) > D.THR_SIM and float(np.nextafter(t, F32(0))) < D.THR_SIM
    flags, run, hits = D.state_machine([None] + [0.0] * 15 + [float("nan")] + [0.0] * 16 + [float("inf")] + [float("-inf")])
    assert (run, hits) == (1, 1) and flags.tolist() == [0] * 32 + [1, 0, 0]       # NaN and +inf reset, -inf is a drift step


def test_total_closed_form_equals_the_generator():
    for step in range(1, 10):
        for fc in range(0, 200):
            assert D.total_frames(fc, step) == D.total_frames_literal(fc, step)
    assert D.score(5, 1, 30, 1) == (16, 30) and D.score_exact(5, 1, 30, 1) == 17


@pytest.mark.parametrize("r", D.TABLE_RUNS)
def test_onehot_sequences_end_where_they_say(oracle, r):
    for h in (max(0, r - 15), max(0, r - 15) + 1, 17, 80):
        if h < r - 15:
            continue
        steps = D.onehot_steps(h, r)
        emb, valid = D.onehot_rows(steps)
        flags, run, hits = D.state_machine(D.onehot_sims(steps))
        assert (hits, run) == (h, r)
        ref = check_oracle(oracle, emb, valid)
        assert (ref["hits"], ref["run"]) == (h, r) and np.array_equal(ref["flags"], flags)
        want = np.array([2.0 if s is None else s for s in D.onehot_sims(steps)], F32)
        assert np.array_equal(ref["sims"], want)                     # exactly 0.0 / 1.0 / 2.0
    with pytest.raises(ValueError):
        D.onehot_steps(0, 16)


def test_run_boundary(oracle):
    for k, hits in ((15, 0), (16, 1), (17, 2)):
        emb, valid = D.onehot_rows([D.DRIFT] * k + [D.SAME])
        ref = check_oracle(oracle, emb, valid)
        assert (ref["hits"], ref["run"]) == (hits, 0)
        assert np.flatnonzero(ref["flags"]).tolist() == list(range(16, k + 1))


@pytest.mark.parametrize("name", D.EDGE_CLIPS)
def test_chunk_edge_clips(oracle, name):
    steps = D.edge_steps(name)
    emb, valid = D.onehot_rows(steps)
    assert len(emb) == D.EDGE_N
    ref = check_oracle(oracle, emb, valid)
    flags, run, hits = D.state_machine(D.onehot_sims(steps))
    assert np.array_equal(ref["flags"], flags) and (ref["run"], ref["hits"]) == (run, hits) and run == 16
    assert flags[8192] == 1 and flags[8191] == 0
    if name.startswith("run15_at_"):
        f = int(name[9:])
        assert flags[f - 15:f + 2].tolist() == [0] * 16 + [1]
    elif name.startswith("reset_at_"):
        f = int(name[9:])
        assert flags[f - 1] == 1 and flags[f] == 0 and flags[f + 16] == 1 and flags[f + 15] == 0
    else:
        assert (valid[4090:4101] == 0).all() and np.isnan(emb[4090:4101]).all()
        first = 4101 + (11 if name == "gap" else 16)                 # the run stood at 4 on frame 4089
        assert flags[first] == 1 and not flags[4086:first].any()


def test_threshold_sweep_straddles_the_threshold(oracle):
    pairs, c64 = D.threshold_sweep()
    emb, valid = D.sweep_rows(pairs)
    ref = check_oracle(oracle, emb, valid)
    s = ref["sims"][D.SWEEP_PAIR::D.SWEEP_BLOCK]
    assert len(s) == 801 and np.abs(s - c64).max() <= D.BOUND
    t = F32(0.99)
    ulps = (s.astype(np.float64) - float(t)) / float(np.spacing(t))
    assert ((s < t).sum(), (s == t).sum(), (s > t).sum()) == (398, 3, 400)
    assert (s == t).sum() >= 1 and ((ulps < 0) & (ulps >= -2)).sum() >= 2 and ((ulps > 0) & (ulps <= 2)).sum() >= 2
    # the run stands at 15 when the pair is compared: the pair alone decides its flag
    assert np.array_equal(ref["flags"][D.SWEEP_PAIR::D.SWEEP_BLOCK], (s < t).astype(np.uint8))
    assert not ref["flags"].reshape(-1, D.SWEEP_BLOCK)[:, 1:D.SWEEP_PAIR].any()


def test_special_rows(oracle):
    sp = D.special_rows()
    k = D.SPECIAL_AT
    got = {kind: check_oracle(oracle, *sp[kind]) for kind in D.SPECIAL_KINDS}
    sims = {kind: got[kind]["sims"] for kind in got}
    for kind in ("zero", "nan_elem", "inf_elem"):
        assert np.isnan(sims[kind][k:k + 2]).all() and np.isnan(sims[kind]).sum() == 2
    assert (sims["sim_pos_inf"][k:k + 2] == np.inf).all() and (sims["sim_neg_inf"][k:k + 2] == -np.inf).all()
    for kind in ("scaled_up", "scaled_down"):
        assert sims[kind].tobytes() == sims["plain"].tobytes()
    for kind in D.SPECIAL_KINDS:                                      # inside a drifting run longer than 16
        others = np.delete(sims[kind], [0, k, k + 1])
        assert (others < F32(0.5)).all() and k > 17 and D.SPECIAL_N - k > 18
    # NaN and +inf reset the run (model.py:62-65); -inf and the scaled rows do not
    for kind in ("zero", "nan_elem", "inf_elem", "sim_pos_inf"):
        assert (got[kind]["run"], got[kind]["hits"]) == (28, 27)
    for kind in ("plain", "sim_neg_inf", "scaled_up", "scaled_down"):
        assert (got[kind]["run"], got[kind]["hits"]) == (59, 44)
    # what a rule that skips every similarity that is not <= 1.5 would give on the zero row: the divergence these tests exist for
    skipping = [None if (s is None or not s <= 1.5) else s for s in D.per_frame(sims["zero"], sp["zero"][1])]
    assert D.state_machine(skipping)[1:] == (57, 42)
    emb, valid, at = D.special_clip()
    check_oracle(oracle, emb, valid)
    assert at.tolist() == [60 * i + 30 for i in range(8)]


def test_random_valid_masks(oracle):
    rng = np.random.default_rng(4)
    base = rng.standard_normal(512)
    for n, p_face, frame_count, fps in ((300, 0.9, 1200, 30), (300, 0.5, 901, 25), (40, 0.2, 40, 6)):
        noise = np.where((np.arange(n) // 40) % 2 == 0, 0.5, 0.01)
        emb = (base[None] + rng.standard_normal((n, 512)) * noise[:, None]).astype(F32)
        emb /= np.linalg.norm(emb, axis=1, keepdims=True)
        valid = (rng.uniform(size=n) < p_face).astype(np.uint8)
        emb[valid == 0] = np.nan                                      # rows without a face are never read
        ref = check_oracle(oracle, emb, valid, frame_count, fps)
        assert ref["hits"] > 0 or p_face < 0.5


def test_score_table_against_the_oracle(oracle):
    table = D.score_table()
    assert len(table) == 31257
    by_seq = {}
    for h, r, fc, fps in table:
        by_seq.setdefault((h, r), []).append((fc, fps))
    for (h, r), rest in by_seq.items():
        emb, valid = D.onehot_sequence(h, r)
        for fc, fps in dict.fromkeys(rest):
            ref = oracle.drift_score(emb, valid, fc, fps)
            assert (ref["hits"], ref["run"]) == (h, r)
            assert ref["score"] == D.score(h, r, fc, fps)[0], (h, r, fc, fps)
    for case in (*D.DEGENERATE_CASES, D.HUGE_CASE, D.CLAMP_CASE):
        h, r, fc, fps = case
        assert oracle.drift_score(*D.onehot_sequence(h, r), fc, fps)["score"] == D.score(*case)[0]
    assert [D.score(*c)[0] for c in D.DEGENERATE_CASES] == [0, 0, 0] and D.score(*D.CLAMP_CASE) == (100, 100)


def test_gpu_subset_keeps_what_matters():
    table, sub = D.score_table(), D.score_subset()
    sens = [c for c in table if D.rounding_sensitive(c)]
    assert len(sens) == 97 and (5, 1, 30, 1) in sens
    assert sum(D.rounding_sensitive(c) for c in sub if c in set(sens)) >= 90 and set(sens) <= set(sub)
    assert len(sub) <= 300
    assert {(fc, fps) for _, _, fc, fps in table} <= {(fc, fps) for _, _, fc, fps in sub}
    h, r, fc, fps = D.CLAMP_CASE                                      # both clamps bind
    pct = 100 * h / D.total_frames(fc, max(1, fps // 7))
    assert pct * r / 15 > 100 and pct + 100 * 0.3 > 100 and D.CLAMP_CASE in sub
    assert set(D.DEGENERATE_CASES) <= set(sub) and D.HUGE_CASE in sub and D.HUGE_CASE[2] == 2 ** 33


def test_compared_counts_every_value_but_the_sentinel():
    from truely_amd.model import compared
    got = compared(np.array([2.0, 1.0, 0.99, np.nan, np.inf, -np.inf, 1.5], F32))
    assert got.tolist() == [False, True, True, True, True, True, True]
