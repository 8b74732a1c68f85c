"""Reference of the drift state machine (trl_drift_score / trl_drift_update: drift_sims_kernel, drift_scan_kernel) and the built
inputs its tests share.  numpy only: no GPU, no oracle.

The reference is a literal transcription of server/model.py:60-66,70,75,86-95 (with the early returns of :31 and :83):

    state_machine   one entry per sampled frame, None where model.py makes no comparison (no face, or no previous embedding);
                    `face_similarity < 0.99` with Python's comparison, so a NaN similarity is NOT below the threshold and resets
                    the run (model.py:62-65), +inf resets it too and -inf is a drift step
    score           model.py:86-95 in Python floats
    cos64           the cosine of model.py:61 in float64

`face_similarity` is a float32 and 0.99 a Python float.  Whether numpy compares them in float32 (0.99 rounded to 0.99f =
0.9900000095...) or in float64 makes no difference for any float32 value: the largest float32 below 0.99f is below 0.99 too, and
0.99f itself is above 0.99, hence "not below" under both rules (test_drift_cpu.py asserts the two facts).

The builders make inputs on which every decision of the state machine is known in advance:

    onehot_rows / onehot_sequence   rows that alternate between two one-hot embeddings: every similarity is exactly 0.0 (a drift
                                    step) or exactly 1.0 (a repeated row: the run resets)
    threshold_sweep / sweep_rows    pairs whose cosine steps through 0.99 in steps of a fraction of an ulp, each compared when the
                                    run stands at exactly 15, so that the pair's similarity alone decides between a hit and a reset
    special_rows                    valid rows whose similarities are NaN, +inf, -inf, or must survive a power-of-two scaling
    score_table / score_subset      (hits, run, frame_count, fps) cases of the score, among them every case of the table where
                                    int() of the double result differs from the floor of the exact rational value
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

F32 = np.float32
THR_SIM = 0.99        # model.py:16
THR_FRAMES = 15       # model.py:17
BOUND = 32 * 2.0 ** -24   # |f32 similarity - cos64| for rows with norms in [0.5, 2] (derivation: test_drift_cpu.py)


# ---- the transcription ------------------------------------------------------------------------------------------------------------
def state_machine(sims):
    """model.py:60-66,70: ``sims`` holds one entry per sampled frame, None where no comparison happens.  -> flags, run, hits."""
    deepfake_count = 0
    deep_fake_frame_count = 0
    flags = []
    for face_similarity in sims:
        flag = 0
        if face_similarity is not None:                              # model.py:60 (and :48,:54,:56: a face was embedded)
            if float(face_similarity) < THR_SIM:                     # model.py:62
                deepfake_count += 1
            else:
                deepfake_count = 0
            if deepfake_count > THR_FRAMES:                          # model.py:66
                deep_fake_frame_count += 1                           # model.py:70
                flag = 1
        flags.append(flag)
    return np.array(flags, np.uint8), deepfake_count, deep_fake_frame_count


def per_frame(sims, valid, has_prev: bool = False):
    """The argument of state_machine from an array of similarities: None where the frame has no face or no embedded predecessor
    (model.py:60,75).  The positions come from ``valid`` alone, never from a value in ``sims``."""
    out = []
    for s, v in zip(sims, valid):
        out.append(s if (v and has_prev) else None)
        has_prev = has_prev or bool(v)
    return out


def total_frames(frame_count: int, step: int) -> int:
    """model.py:86, closed form of ``sum(1 for i in range(frame_count) if i % step == 0)``."""
    return -(-frame_count // step) if frame_count > 0 else 0


@functools.lru_cache(maxsize=None)
def total_frames_literal(frame_count: int, frames_between_processing: int) -> int:
    return sum(1 for i in range(frame_count) if i % frames_between_processing == 0)   # model.py:86


def score(hits: int, run: int, frame_count: int, fps: int):
    """model.py:31,40,83-95 -> (score, total sampled frames); total is 0 where the reference returns before it counts."""
    if fps <= 0:                                                     # model.py:31
        return 0, 0
    frames_between_processing = max(1, int(fps / 7))                 # model.py:40
    if frame_count == 0:                                             # model.py:83
        return 0, 0
    if frame_count <= 4096:
        total_processed_frames = total_frames_literal(frame_count, frames_between_processing)
    else:                                                            # (the closed form: test_drift_cpu.py asserts them equal)
        total_processed_frames = total_frames(frame_count, frames_between_processing)
    if total_processed_frames == 0:
        return 0, 0
    deepfake_percentage = (hits / total_processed_frames) * 100
    confidence_factor = min(deepfake_percentage * (run / THR_FRAMES), 100)
    if frame_count > fps * 30:
        weighted_score = min(deepfake_percentage + confidence_factor * 0.5, 100)
    else:
        weighted_score = min(deepfake_percentage + confidence_factor * 0.3, 100)
    return max(0, min(100, int(weighted_score))), total_processed_frames


def score_exact(hits: int, run: int, frame_count: int, fps: int) -> int:
    """The same formula in exact rational arithmetic (0.5 = 1/2, 0.3 = 3/10): what the score would be without rounding."""
    step = max(1, fps // 7)
    total = total_frames(frame_count, step)
    pct = Fraction(100 * hits, total)
    conf = min(pct * Fraction(run, THR_FRAMES), Fraction(100))
    ws = min(pct + conf * (Fraction(1, 2) if frame_count > fps * 30 else Fraction(3, 10)), Fraction(100))
    return max(0, min(100, ws.numerator // ws.denominator))


def cos64(a, b) -> float:
    """model.py:61 in float64; NaN where the cosine is undefined (a zero row) or the rows hold NaN / inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def pair_index(valid, has_prev: bool = False):
    """For every frame the index of the row it is compared with (model.py:75), -1 where none; -2 = the carried row."""
    out, prev = [], (-2 if has_prev else -1)
    for i, v in enumerate(valid):
        out.append(prev if v else -1)
        if v:
            prev = i
    return np.array(out, np.int64)


# ---- one-hot rows -----------------------------------------------------------------------------------------------------------------
DRIFT, SAME, NOFACE = 1, 0, -1


def onehot_rows(steps):
    """A clip of len(steps) + 1 frames.  The first frame holds one-hot row 0; ``steps[k]`` makes frame k + 1 the OTHER one-hot row
    (DRIFT: similarity exactly 0.0), the SAME row (exactly 1.0) or a frame without a face (NOFACE: valid = 0, the row is filled
    with NaN -- nothing may read it).  -> emb (n, 512) float32, valid (n,) uint8."""
    steps = np.asarray(steps, np.int64)
    n = len(steps) + 1
    face = np.ones(n, bool)
    face[1:] = steps != NOFACE
    flip = np.zeros(n, np.int64)
    flip[1:] = steps == DRIFT
    which = np.cumsum(flip) & 1
    emb = np.zeros((n, 512), F32)
    emb[np.arange(n), which] = 1
    emb[~face] = np.nan
    return emb, face.astype(np.uint8)


def onehot_sims(steps):
    """The similarities of onehot_rows(steps), known without any arithmetic: None (no comparison) for the first frame and the
    faceless ones, else 0.0 or 1.0."""
    return [None] + [None if s == NOFACE else (0.0 if s == DRIFT else 1.0) for s in steps]


EDGE_N = 8193          # two full LDS chunks of the scan (4096 similarities each) and one element
EDGE_SIZES = (0, 1, 2, 3, 4, 5, 4095, 4096, 4097, 8192, 8193)
EDGE_CLIPS = ("run15_at_4094", "run15_at_4095", "run15_at_4096", "reset_at_4095", "reset_at_4096", "gap", "gap_reset")


def edge_steps(name: str):
    """Steps of an 8193-frame one-hot clip whose decisions sit on the scan's chunk borders (elements 4095 | 4096 and 8191 | 8192).
    Every clip resets at frames 1000, 3000 and 8176 (so the run stands at 15 on element 8191 and makes its first hit on 8192, the
    lone element of the third chunk), and

        run15_at_F      resets at F - 15: the run stands at exactly 15 on element F and the first hit falls on F + 1
        reset_at_F      a long run (hits on every frame since 3016) is reset on element F
        gap             a reset at 4085, then no face on 4090..4100: the run of 4 waits across the border and goes on at 4101
        gap_reset       the same, and frame 4101 repeats the row of 4089: a similarity of 1.0 across the gap and the border
    """
    steps = np.full(EDGE_N - 1, DRIFT, np.int64)

    def put(frame, what):
        steps[frame - 1] = what

    for f in (1000, 3000, 8176):
        put(f, SAME)
    if name.startswith("run15_at_"):
        put(int(name[9:]) - THR_FRAMES, SAME)
    elif name.startswith("reset_at_"):
        put(int(name[9:]), SAME)
    elif name in ("gap", "gap_reset"):
        put(4085, SAME)
        for f in range(4090, 4101):
            put(f, NOFACE)
        if name == "gap_reset":
            put(4101, SAME)
    else:
        raise KeyError(name)
    return steps


def onehot_steps(h: int, r: int):
    """Steps that end with ``hits == h`` and ``run == r``: 15 + h1 drift steps, one repeat, r drift steps, where the last stretch
    contributes max(0, r - 15) hits itself and the first one h1 = h - max(0, r - 15) >= 0."""
    h1 = h - max(0, r - THR_FRAMES)
    if h < 0 or r < 0 or h1 < 0:
        raise ValueError(f"no sequence ends with hits={h}, run={r}")
    return [DRIFT] * (THR_FRAMES + h1) + [SAME] + [DRIFT] * r


def onehot_sequence(h: int, r: int):
    """emb, valid (all ones) of a clip whose state machine ends with hits == h and run == r."""
    return onehot_rows(onehot_steps(h, r))


# ---- the threshold sweep ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def threshold_sweep(seed: int = 0, K: int = 400, step: float = 2e-7):
    """2K + 1 pairs (u, cos t * u + sin t * v), u and v orthonormal in float64, t = arccos(0.99) + k * step for k = -K..K, rounded
    to float32.  The cosine falls by about 2.8e-8 = 0.47 ulp of 0.99f per step.  With the defaults the float32 similarities are
    398 below 0.99f, 3 equal to it and 400 above, two or more within 2 ulp on either side (asserted in test_drift_cpu.py).
    -> (pairs (2K + 1, 2, 512) float32, cosines in float64 of the float32 rows)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(512)
    v = rng.standard_normal(512)
    u /= np.linalg.norm(u)
    v -= np.dot(u, v) * u
    v /= np.linalg.norm(v)
    t = np.arccos(THR_SIM) + np.arange(-K, K + 1) * step
    pairs = np.empty((2 * K + 1, 2, 512), F32)
    pairs[:, 0] = u.astype(F32)
    pairs[:, 1] = (np.cos(t)[:, None] * u + np.sin(t)[:, None] * v).astype(F32)
    pairs.setflags(write=False)
    return pairs, np.array([cos64(p[0], p[1]) for p in pairs])


SWEEP_BLOCK = 18   # rows per pair in sweep_rows
SWEEP_PAIR = 17    # offset of the pair's second row in its block: its similarity is the pair's


def sweep_rows(pairs):
    """Every pair behind 15 drift steps: a block is [e0, e0 (a repeat: the run resets), 14 alternating one-hot rows (run 14), u (its
    cosine with a one-hot row is one of its own elements, far below 0.99: run 15), w].  The similarity of w with u then decides:
    below 0.99f the run reaches 16 (a hit; the block's first row, compared with w, then makes another), otherwise it resets.
    -> emb (18 * len(pairs), 512), valid (all ones)."""
    head, _ = onehot_rows([SAME] + [DRIFT] * 14)
    assert len(head) == SWEEP_BLOCK - 2
    emb = np.empty((len(pairs), SWEEP_BLOCK, 512), F32)
    emb[:, :16] = head
    emb[:, 16:] = pairs
    return emb.reshape(-1, 512), np.ones(len(pairs) * SWEEP_BLOCK, np.uint8)


# ---- rows with similarities that are no ordinary numbers --------------------------------------------------------------------------
SPECIAL_N, SPECIAL_AT = 60, 30
SPECIAL_KINDS = ("plain", "zero", "nan_elem", "inf_elem", "sim_pos_inf", "sim_neg_inf", "scaled_up", "scaled_down")


def _unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x)).astype(F32)


@functools.lru_cache(maxsize=None)
def special_rows():
    """{kind: (emb (60, 512), valid (all ones))}: 60 unit rows with random signs and magnitudes within a factor of three of each
    other (no product of two elements comes near the denormal range, whatever the scaling below), so that consecutive rows have a
    cosine of about +-0.05 and the whole clip is one drifting run; row 30 is replaced:

        plain         B = the normalised sum of its two neighbours (cosine about 0.7 with both)
        zero          all zeros: 0 / 0 = NaN against both neighbours
        nan_elem      B with one NaN element
        inf_elem      B with one +inf element: inf / inf = NaN
        sim_pos_inf   B * 2^-80: dot(cur, cur) underflows to 0 in either denormal mode, the dot with a neighbour (about
                      0.7 * 2^-80) stays normal and is positive: similarity +inf
        sim_neg_inf   -B * 2^-80: similarity -inf, a drift step under every rule
        scaled_up     B * 2^40  \\  every product and partial sum of the three dots scales by an exact power of two, so the
        scaled_down   B * 2^-40 /  similarities must equal those of `plain` bit for bit
    """
    rng = np.random.default_rng(1)
    rows = rng.uniform(0.5, 1.5, (SPECIAL_N, 512)) * rng.choice([-1.0, 1.0], (SPECIAL_N, 512))
    rows = np.stack([_unit(r) for r in rows])
    k = SPECIAL_AT
    B = _unit(rows[k - 1].astype(np.float64) + rows[k + 1])
    nan_elem, inf_elem = B.copy(), B.copy()
    nan_elem[77] = np.nan
    inf_elem[300] = np.inf
    special = {"plain": B, "zero": np.zeros(512, F32), "nan_elem": nan_elem, "inf_elem": inf_elem,
               "sim_pos_inf": B * F32(2.0 ** -80), "sim_neg_inf": -B * F32(2.0 ** -80),
               "scaled_up": B * F32(2.0 ** 40), "scaled_down": B * F32(2.0 ** -40)}
    assert tuple(special) == SPECIAL_KINDS
    out = {}
    for kind, row in special.items():
        emb = rows.copy()
        emb[k] = row
        emb.setflags(write=False)
        out[kind] = (emb, np.ones(SPECIAL_N, np.uint8))
    return out


def special_clip():
    """All kinds one after the other as ONE clip.  -> emb, valid, the indices of the special rows."""
    sp = special_rows()
    emb = np.concatenate([sp[k][0] for k in SPECIAL_KINDS])
    at = np.arange(len(SPECIAL_KINDS)) * SPECIAL_N + SPECIAL_AT
    return emb, np.ones(len(emb), np.uint8), at


# ---- the score table --------------------------------------------------------------------------------------------------------------
TABLE_FPS = (1, 6, 7, 13, 14, 24, 25, 30, 60)
TABLE_RUNS = (0, 1, 14, 15, 16, 17, 30, 45)
H_MAX = 80


def table_frame_counts(fps: int):
    step = max(1, int(fps / 7))
    return (1, step, step + 1, fps * 30 - 1, fps * 30, fps * 30 + 1, 400, 1000, 2999)


@functools.lru_cache(maxsize=None)
def score_table():
    """Every (h, r, frame_count, fps) of the table: fps and r as above, frame_count around the sampling step and the 30-second
    weight switch, h from max(0, r - 15) (a run of r has made that many hits itself) to min(total, 80)."""
    out = []
    for fps in TABLE_FPS:
        step = max(1, int(fps / 7))
        for fc in table_frame_counts(fps):
            total = total_frames(fc, step)
            for r in TABLE_RUNS:
                for h in range(max(0, r - THR_FRAMES), min(total, H_MAX) + 1):
                    out.append((h, r, fc, fps))
    return tuple(out)


def rounding_sensitive(case) -> bool:
    """int() of the double result differs from the floor of the exact rational value."""
    return score(*case)[0] != score_exact(*case)


CLAMP_CASE = (80, 45, 400, 30)            # pct = 80, conf = min(240, 100), ws = min(80 + 30, 100): both clamps bind
HUGE_CASE = (40, 20, 2 ** 33, 1)          # total = 2^33 does not fit the int32 it is reported in: the score alone is defined
DEGENERATE_CASES = ((40, 20, 0, 30), (40, 20, 400, 0), (40, 20, 400, -1))   # model.py:83 and :31: score 0


@functools.lru_cache(maxsize=None)
def score_subset():
    """The cases the GPU runs: every rounding-sensitive case of the table, every (fps, frame_count) of it at least once (with a run
    past the threshold and as many hits as fit, up to 40), the clamp case and the degenerate and huge inputs."""
    table = score_table()
    out = [c for c in table if rounding_sensitive(c)]
    for fps in TABLE_FPS:
        step = max(1, int(fps / 7))
        for fc in table_frame_counts(fps):
            out.append((max(1, min(total_frames(fc, step), 40)), 16, fc, fps))
    assert set(out) <= set(table) and CLAMP_CASE in table
    out += [CLAMP_CASE, *DEGENERATE_CASES, HUGE_CASE]
    return tuple(dict.fromkeys(out))
