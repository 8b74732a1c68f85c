"""trl_drift_score / trl_drift_update (drift_sims_kernel, drift_scan_kernel) on the built cases of tests/drift_ref.py: similarities
within an ulp of the threshold, rows whose similarities are NaN / +inf / -inf, runs that stop at 15 or reach 16 on a window cut
or on the scan's 4096-element chunk border, the score where int() depends on double rounding, and the NULL-buffer paths.

Similarities: bit for bit the oracle's (NaN = NaN), and within 32 * 2^-24 of the float64 cosine (derivation: test_drift_cpu.py).
Flags, run and hits: the oracle's AND those of the transcription of server/model.py (drift_ref.state_machine), which
test_drift_cpu.py holds the oracle to.  The largest input is 8193 x 512 floats."""
import ctypes as C

import numpy as np
import pytest

import drift_ref as D

pytestmark = pytest.mark.gpu
F32 = np.float32
_REF = {}


def _t(x):
    import torch
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, order="C"))   # (a copy: the built cases are read-only)


def ref_of(oracle, key, emb, valid, frame_count, fps):
    """The oracle's answer for a built clip, computed once per session and never changed."""
    if key not in _REF:
        r = oracle.drift_score(emb, valid, frame_count, fps)
        for a in (r["sims"], r["flags"]):
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def check(got, ref, emb, valid, what=""):
    """``got``: sims / flags (numpy) and run / hits / score of the device for the whole clip ``emb, valid``."""
    sims, flags = got["sims"], got["flags"]
    assert np.array_equal(sims, ref["sims"], equal_nan=True), what
    prev = D.pair_index(valid)
    norms = np.linalg.norm(np.asarray(emb, np.float64), axis=1)
    with np.errstate(all="ignore"):
        ok = (prev >= 0) & (norms >= 0.5) & (norms <= 2)
        ok[ok] &= (norms[prev[ok]] >= 0.5) & (norms[prev[ok]] <= 2)
    idx = np.flatnonzero(ok)
    a, b = np.asarray(emb[idx], np.float64), np.asarray(emb[prev[idx]], np.float64)
    cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    assert len(idx) == 0 or np.abs(sims[idx] - cos).max() <= D.BOUND, what
    want_flags, run, hits = D.state_machine(D.per_frame(sims, valid))
    assert (got["run"], got["hits"]) == (run, hits) == (ref["run"], ref["hits"]), (what, got["run"], got["hits"], run, hits)
    if flags is not None:
        assert np.array_equal(flags, want_flags) and np.array_equal(flags, ref["flags"]), what
    assert got["score"] == ref["score"], what


def run_score(engine, emb, valid, frame_count, fps=30):
    d = engine.drift_score(_t(emb), _t(valid), frame_count, fps)
    return dict(d, sims=d["sims"].cpu().numpy(), flags=d["flags"].cpu().numpy())


def run_update(engine, emb, valid, cuts, per_frame=4, fps=30, want_flags=True):
    """The clip through trl_drift_update in the windows cuts[k]..cuts[k+1] (0 and n are added)."""
    import torch
    n = len(valid)
    d_emb, d_valid = _t(emb).to(engine.device), _t(valid).to(engine.device)
    cuts = sorted({0, n, *[c for c in cuts if 0 <= c <= n]})
    state = engine.drift_state()
    sims, flags, d = [], [], None
    for a, b in zip(cuts[:-1], cuts[1:]):
        d = engine.drift_update(state, d_emb[a:b], d_valid[a:b], b * per_frame, fps, want_flags=want_flags)
        sims.append(d["sims"])
        flags.append(d["flags"])
    return {"sims": torch.cat(sims).cpu().numpy(), "flags": torch.cat(flags).cpu().numpy() if want_flags else None,
            "run": d["run"], "hits": d["hits"], "score": d["score"], "total": d["total"]}


# ---- similarities that are no ordinary numbers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.SPECIAL_KINDS)
def test_special_rows_score(engine, oracle, kind):
    """A valid row whose similarity with both neighbours is NaN (a zero row, a NaN or +inf element) or +inf (a norm that underflows)
    is a comparison that is not below 0.99: the run resets (model.py:62-65).  -inf is a drift step; a row scaled by 2^40 or 2^-40
    gives the bits of the unscaled row."""
    emb, valid = D.special_rows()[kind]
    n = len(valid)
    got = run_score(engine, emb, valid, n * 4)
    print(f"{kind}: device run, hits = {got['run']}, {got['hits']}")
    check(got, ref_of(oracle, ("special", kind), emb, valid, n * 4, 30), emb, valid, kind)
    k = D.SPECIAL_AT
    if kind in ("zero", "nan_elem", "inf_elem"):
        assert np.isnan(got["sims"][k:k + 2]).all()
    if kind in ("zero", "nan_elem", "inf_elem", "sim_pos_inf"):
        assert (got["run"], got["hits"]) == (28, 27) and not got["flags"][k:k + 17].any() and got["flags"][k + 17] == 1
    else:
        assert (got["run"], got["hits"]) == (59, 44) and got["flags"][16:].all()
    if kind.startswith("scaled"):
        assert got["sims"].tobytes() == ref_of(oracle, ("special", "plain"), *D.special_rows()["plain"], n * 4, 30)["sims"].tobytes()


@pytest.mark.parametrize("where", ("last_of_window", "first_of_window"))
def test_special_rows_update(engine, oracle, where):
    """The same rows in one clip through trl_drift_update: each special row is the last row of a window (it becomes the carried
    embedding and the next window's first comparison is with it) or the first row of one (it is compared with the carried one)."""
    emb, valid, at = D.special_clip()
    n = len(valid)
    cuts = at + 1 if where == "last_of_window" else at
    got = run_update(engine, emb, valid, cuts.tolist())
    check(got, ref_of(oracle, "special_clip", emb, valid, n * 4, 30), emb, valid, where)


# ---- similarities within an ulp of the threshold ----------------------------------------------------------------------------------
def _sweep_halves():
    pairs, _ = D.threshold_sweep()
    return [(k, *D.sweep_rows(pairs[a:b])) for k, (a, b) in enumerate(((0, 401), (401, 801)))]


def test_threshold_sweep_score(engine, oracle):
    """801 pairs whose similarity steps through 0.99f (3 equal to it, 2 and 5 within 2 ulp on either side), each compared with the
    run at 15: the flag of the pair's frame is the comparison `sim < 0.99f` itself."""
    below = 0
    for k, emb, valid in _sweep_halves():
        n = len(valid)
        got = run_score(engine, emb, valid, n * 4)
        check(got, ref_of(oracle, ("sweep", k), emb, valid, n * 4, 30), emb, valid)
        s = got["sims"][D.SWEEP_PAIR::D.SWEEP_BLOCK]
        assert np.array_equal(got["flags"][D.SWEEP_PAIR::D.SWEEP_BLOCK], (s < F32(0.99)).astype(np.uint8))
        below += int((s < F32(0.99)).sum())
    assert below == 398


def test_threshold_sweep_update(engine, oracle):
    """... and with window cuts between the two rows of a pair (every 7th pair; the pair is compared across the carry), after a
    pair, and in the middle of a run."""
    for k, emb, valid in _sweep_halves():
        n = len(valid)
        cuts = [D.SWEEP_BLOCK * b + D.SWEEP_PAIR for b in range(0, n // D.SWEEP_BLOCK, 7)]
        cuts += [D.SWEEP_BLOCK * b for b in range(3, n // D.SWEEP_BLOCK, 11)] + [D.SWEEP_BLOCK * b + 9 for b in range(5, n // D.SWEEP_BLOCK, 13)]
        got = run_update(engine, emb, valid, cuts)
        check(got, ref_of(oracle, ("sweep", k), emb, valid, n * 4, 30), emb, valid)


# ---- launch and chunk edges -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_clips(engine):
    """name -> (steps, emb, valid, device emb, device valid): uploaded once, sliced on the device."""
    out = {}
    for name in D.EDGE_CLIPS:
        steps = D.edge_steps(name)
        emb, valid = D.onehot_rows(steps)
        out[name] = (steps, emb, valid, _t(emb).to(engine.device), _t(valid).to(engine.device))
    return out


def _onehot_want(steps, n):
    per = D.onehot_sims(steps)[:n]
    flags, run, hits = D.state_machine(per)
    return np.array([2.0 if s is None else s for s in per], F32), flags, run, hits


@pytest.mark.parametrize("n", D.EDGE_SIZES)
def test_every_launch_size(engine, oracle, edge_clips, n):
    """n = 0..5 (the similarity kernel's blocks of four frames) and one element either side of one and two scan chunks: prefixes of
    a clip whose run stands at 15 on element 4095 (and 8191) and makes its first hit on 4096 (and 8192)."""
    steps, emb, valid, d_emb, d_valid = edge_clips["run15_at_4095"]
    sims, flags, run, hits = _onehot_want(steps, n)
    if n == 0:                                                       # no rows: through the C entry point with live pointers
        import torch
        res = torch.full((4,), -1, dtype=torch.int32, device=engine.device)
        st = engine.lib.trl_drift_score(engine._h, C.c_void_p(d_emb.data_ptr()), C.c_void_p(d_valid.data_ptr()), 0, 400, 30,
                                        None, None, C.c_void_p(res.data_ptr()), engine._stream())
        assert st == 0 and res.cpu().tolist() == [0, 0, 0, 100]
        d = engine.drift_update(engine.drift_state(), None, None, 400, 30)
        assert (d["score"], d["run"], d["hits"], d["total"]) == (0, 0, 0, 100)
        return
    got = run_score(engine, d_emb[:n], d_valid[:n], n * 4)
    assert np.array_equal(got["sims"], sims) and np.array_equal(got["flags"], flags) and (got["run"], got["hits"]) == (run, hits)
    check(got, ref_of(oracle, ("edge", "run15_at_4095", n), emb[:n], valid[:n], n * 4, 30), emb[:n], valid[:n])
    if n >= 4097:
        assert flags[4096] == 1 and not flags[4080:4096].any()


@pytest.mark.parametrize("name", D.EDGE_CLIPS)
def test_chunk_border_decisions(engine, oracle, edge_clips, name):
    """A run of exactly 15 on the last element of a scan chunk, its first hit on the first element of the next (and both shifted
    by one either way), a reset on the border, a faceless gap across it -- in one call, and through trl_drift_update cut at
    4095, 4096 and 4097.  The expected similarities (0.0, 1.0, 2.0), flags and counters are known without arithmetic."""
    steps, emb, valid, d_emb, d_valid = edge_clips[name]
    n = D.EDGE_N
    sims, flags, run, hits = _onehot_want(steps, n)
    ref = ref_of(oracle, ("edge", name, n), emb, valid, n * 4, 30)
    got = run_score(engine, d_emb, d_valid, n * 4)
    assert np.array_equal(got["sims"], sims) and np.array_equal(got["flags"], flags) and (got["run"], got["hits"]) == (run, hits)
    check(got, ref, emb, valid, name)
    for cut in (4095, 4096, 4097):
        got = run_update(engine, d_emb, d_valid, [cut])
        assert np.array_equal(got["sims"], sims) and np.array_equal(got["flags"], flags), (name, cut)
        assert (got["run"], got["hits"], got["score"]) == (run, hits, ref["score"]), (name, cut)


def test_run_boundary(engine):
    """15 drifting comparisons and a reset: no hit.  16: one hit, flagged on the 16th comparison's frame only."""
    for k, want in ((15, []), (16, [16]), (17, [16, 17])):
        emb, valid = D.onehot_rows([D.DRIFT] * k + [D.SAME])
        got = run_score(engine, emb, valid, 400)
        assert (got["run"], got["hits"]) == (0, len(want)) and np.flatnonzero(got["flags"]).tolist() == want
        assert got["sims"].tolist() == [2.0] + [0.0] * k + [1.0]
        got = run_update(engine, emb, valid, [16, 17])
        assert (got["run"], got["hits"]) == (0, len(want)) and np.flatnonzero(got["flags"]).tolist() == want


# ---- the score --------------------------------------------------------------------------------------------------------------------
def test_score_table(engine):
    """Per (hits, run): one trl_drift_update with the one-hot clip that ends there; then the score alone is recomputed from the
    carried counters for every (frame_count, fps) of the subset -- all 97 cases of the table whose int() depends on the rounding
    of the double arithmetic, every frame_count / fps edge, both clamps, frame_count = 0, fps <= 0 and a frame_count of 2^33."""
    by_seq = {}
    for h, r, fc, fps in D.score_subset():
        by_seq.setdefault((h, r), []).append((fc, fps))
    ran = sens = 0
    for (h, r), rest in by_seq.items():
        emb, valid = D.onehot_sequence(h, r)
        state = engine.drift_state()
        d = engine.drift_update(state, _t(emb), _t(valid), len(valid), 7)
        assert (d["hits"], d["run"]) == (h, r)
        for fc, fps in rest:
            d = engine.drift_update(state, None, None, fc, fps)
            score, total = D.score(h, r, fc, fps)
            assert (d["score"], d["hits"], d["run"]) == (score, h, r), (h, r, fc, fps, d["score"], score)
            if (h, r, fc, fps) != D.HUGE_CASE:                       # (its total does not fit the int32 it is reported in)
                assert d["total"] == total, (h, r, fc, fps)
            ran += 1
            sens += fc > 0 and fps > 0 and fc < 2 ** 31 and D.rounding_sensitive((h, r, fc, fps))
    print(f"score table: {ran} cases, {sens} of them rounding-sensitive, {len(by_seq)} clips")
    assert ran == len(D.score_subset()) and sens >= 90


# ---- NULL buffers and stale memory ------------------------------------------------------------------------------------------------
def test_null_sims_and_flags(engine, oracle, edge_clips):
    """d_sims == NULL (the library's own similarity buffer, grown from 5 to 4097 rows and reused for 3) and d_flags == NULL give
    the d_result of the call with buffers -- with the workspaces and the LDS of every CU full of NaN patterns beforehand."""
    import torch
    steps, emb, valid, d_emb, d_valid = edge_clips["run15_at_4095"]
    lib, h = engine.lib, engine._h

    def call(n, sims, flags, off=0):
        res = torch.full((4,), -1, dtype=torch.int32, device=engine.device)
        e, v = d_emb[off:off + n], d_valid[off:off + n]
        st = lib.trl_drift_score(h, C.c_void_p(e.data_ptr()), C.c_void_p(v.data_ptr()), n, n * 4, 30,
                                 C.c_void_p(sims.data_ptr()) if sims is not None else None,
                                 C.c_void_p(flags.data_ptr()) if flags is not None else None, C.c_void_p(res.data_ptr()), engine._stream())
        assert st == 0
        return res.cpu().tolist()

    engine.poison_workspaces(0xFF)
    for n, off in ((5, 0), (4097, 0), (3, 0), (40, 4070)):
        _, want_flags, run, hits = _onehot_want(steps[off:], n)
        sims = torch.empty((n,), dtype=torch.float32, device=engine.device)
        flags = torch.zeros((n,), dtype=torch.uint8, device=engine.device)
        full = call(n, sims, flags, off)
        assert full[1:3] == [run, hits] and full[0] == D.score(hits, run, n * 4, 30)[0] and full[3] == n
        f2 = torch.zeros_like(flags)
        assert call(n, None, f2, off) == full and np.array_equal(f2.cpu().numpy(), want_flags)
        assert call(n, None, None, off) == full
        assert call(n, sims, None, off) == full
    n = 4097
    got = run_update(engine, d_emb[:n], d_valid[:n], [5, 4096], want_flags=False)
    ref = ref_of(oracle, ("edge", "run15_at_4095", n), emb[:n], valid[:n], n * 4, 30)
    check(got, ref, emb[:n], valid[:n], "want_flags=False")
    assert got["hits"] > 3000
