"""The fp16 conv3 screen of the fused PNet kernel bounds its error per input: E = sum over a cell's 3 x 3 x 16 conv2 inputs of
ghat[channel] |x| + B, where it used the cell's largest input, E = A X + B.  Fewer M-tiles confirm; no record
may change.  These tests compare every level's candidate records with the oracle's, screen on and off, at 120 x 160 and on levels
of 2 x 3 tiles whose bottom tile row holds 1 and 15 rows, in the halo-carry runs of 1, 2, 3 and 24; with thr0 chosen from a float32
model of d + E so that a chosen M-tile holds exactly 1, 2, 4, 5 and 32 flagged cells; with thr0 on the exact probability (and the
floats on either side) of cells placed in both output rows of an M-tile, in both M-tiles of a wave and on the last valid row and
column of an edge tile; for the five slope classes, a frame beyond fp16 between two ordinary ones and thr0 = 0.  Records cannot
tell which rule the kernel applies: the tuning build's counter of confirmed M-tiles (build() makes that library too) is held
between bounds derived from the screen's guarantee, below the replaced rule's count restated in numpy, and above the M-tiles
that hold a record."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import truely_amd
from truely_amd import _lib, weights
from slope_variants import slope_variant_blob
from test_gpu_pnet_screen_operands import _check_levels, _conv2_absmax, _engine, _levels, _oracle_maps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pnet_screen_audit import mtile_hits, pnet_maps, screen_bound, screen_weights  # noqa: E402

# (frames, H, W, seed): first levels 32 x 44 (2 x 3 tiles, 16 rows), 17 x 44 (2 x 3 tiles, 1 row in the last tile row) and 31 x 35 (2 x 3 tiles,
# 15 rows); test_geometry holds the sizes to that
SIZES = [(2, 120, 160, 41), (2, 72, 160, 17), (2, 117, 131, 29)]
RUNS = [1, 2, 3, 24]
COUNTS = [1, 2, 4, 5, 32]          # flagged cells of the chosen M-tile: few, a handful, one more, all of them
TUNING_LIB = os.path.join(os.path.dirname(_lib.LIB_PATH), "libtruely_hip_tuning.so")


@pytest.fixture(scope="module")
def clips(oracle):
    """[(frames, oracle maps)] of SIZES under the seeded weights; read-only"""
    out = []
    for (n, H, W, seed) in SIZES:
        fr = truely_amd.synthetic.synthetic_frames(n, H, W, seed=seed)
        out.append((fr, _oracle_maps(oracle, fr, H, W)))
    return out


@pytest.fixture(scope="module")
def model(oracle, blob, clips):
    """float32 model of the screen's inputs for every (clip, frame, level): (d, X, S) maps -- logit difference, largest |conv2
    input| and per-input error sum of each cell (tools/pnet_screen_audit.py) -- with (A, B); read-only"""
    t = weights.unpack_tensors(blob)
    A, B, _ = screen_bound(t)
    _g, ghat, _B, _ok = screen_weights(t)
    maps = []
    for (n, H, W, _seed), (fr, _m) in zip(SIZES, clips):
        maps.append([[pnet_maps(oracle.area_resample_norm(f, 0, H, 0, W, h, w), t, ghat) for (h, w) in _levels(oracle, H, W)] for f in fr])
    return maps, A, B


def test_geometry(clips):
    first = [maps[0][0][0].shape for (_fr, maps) in clips]
    assert first[0] == (32, 44)                                               # 120 x 160: 2 x 3 full tiles, every wave has both its M-tiles
    assert first[1][0] == 17 and 32 < first[1][1] <= 48                       # 2 x 3 tiles, one row in the bottom tile row
    assert first[2][0] == 31 and 32 < first[2][1] <= 48                       # 2 x 3 tiles, fifteen rows
    for (fr, _maps) in clips:
        assert len(fr) == 2 and fr.shape[1] <= 120 and fr.shape[2] <= 160


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("screen", [1, 0])
def test_levels_equal_the_oracle(blob, clips, screen, run):
    n = 0
    for thr in (0.6, 0.011):
        eng = _engine(blob, thr, screen, run)
        for (fr, maps) in clips:
            n += _check_levels(eng, maps, fr, thr, 0xFF)
    assert n > 0


def _thr_of(dthr):
    """thr0 whose prefilter bound ln(thr / (1 - thr)) - 0.05 is dthr"""
    return 1.0 / (1.0 + math.exp(-(dthr + 0.05)))


def _mtile_with(count, d, S, B):
    """an M-tile (2 output rows x 16 columns, all 32 cells inside the level) of the model maps and a bound dthr under which exactly
    `count` of its cells have d + S + B >= dthr, with the widest gap to the next cell on either side and thr0 inside [0.01, 0.99]"""
    v = d.astype(np.float64) + S + B
    best = None
    for y in range(0, v.shape[0] - 1, 2):
        for x in range(0, v.shape[1] - 15, 16):
            c = np.sort(v[y:y + 2, x:x + 16].reshape(-1))[::-1]
            lo = c[count] if count < 32 else c[31] - 0.2
            gap = c[count - 1] - lo
            dthr = 0.5 * (c[count - 1] + lo)
            if 0.011 < _thr_of(dthr) < 0.989 and (best is None or gap > best[0]):
                best = (gap, y, x, dthr)
    return best


@pytest.mark.parametrize("count", COUNTS)
def test_threshold_for_a_number_of_flagged_cells(blob, clips, model, count):
    """thr0 from the model so that one M-tile holds exactly `count` cells within the screen's margin (the model's d differs from the
    screen's by far less than the gap asked for): records with the screen on and off equal the oracle's"""
    maps, _A, B = model
    for ci, (fr, omaps) in enumerate(clips):
        d, _X, S = maps[ci][0][0]
        best = _mtile_with(count, d, S, B)
        assert best is not None and best[0] > 2e-2, (ci, count, best)      # (the screen's own error on these cells is ~1e-3)
        thr = _thr_of(best[3])
        flagged = (d.astype(np.float64) + S + B >= best[3])[best[1]:best[1] + 2, best[2]:best[2] + 16]
        assert int(flagged.sum()) == count
        for screen in (1, 0):
            _check_levels(_engine(blob, thr, screen, 3), omaps, fr, thr, 0xFF)


def _placed_cells(p):
    """cells of a level's probability map [oh][ow] by where the kernel computes them: output row 0 / 1 of an M-tile (the lane
    halves of its 32 cells), M-tiles 0..3 / 4..7 of a tile (a wave's first / second), and the last valid row and column of the
    level's edge tiles; of each class the cell whose probability is nearest 0.5"""
    oh, ow = p.shape
    yy, xx = np.mgrid[0:oh, 0:ow]
    ok = (p > 0.02) & (p < 0.98)
    classes = [(yy % 2 == r) & ((yy % 16 >= 8) == s) for r in (0, 1) for s in (False, True)]
    classes += [yy == oh - 1, xx == ow - 1, (yy == oh - 1) & (xx == ow - 1)]
    out = []
    for c in classes:
        c = c & ok if (c & ok).any() else c           # (inside the prefilter's range where the class has such a cell)
        out.append(np.unravel_index(np.argmin(np.where(c, np.abs(p - 0.5), np.inf)), p.shape))
    return out


@pytest.mark.parametrize("screen", [1, 0])
def test_threshold_on_placed_cells(blob, clips, screen):
    for (fr, omaps) in clips:
        p = omaps[0][0][0]
        for (y, x) in _placed_cells(p):
            v = np.float32(p[y, x])
            for thr in (np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))):
                _check_levels(_engine(blob, float(thr), screen, 3), omaps, fr, float(thr), 0xFF)


@pytest.mark.parametrize("variant", ["slopes_above_one", "negative_slopes", "mixed_signs", "negative_deep_only", "generalise_prelu"])
def test_prelu_variants(variant):
    from oracle.oracle import Oracle
    vblob = slope_variant_blob(variant)
    for (n, H, W, seed) in SIZES[1:]:
        fr = truely_amd.synthetic.synthetic_frames(2, H, W, seed=seed)
        maps = _oracle_maps(Oracle(vblob), fr, H, W)
        for screen in (1, 0):
            for run in (1, 24):
                _check_levels(_engine(vblob, 0.6, screen, run), maps, fr, 0.6, 0xFF)


def test_hot_frame_between_ordinary_ones():
    """the middle frame's conv2 activations leave the fp16 range (its items store the largest finite float, E reaches it and the
    M-tile confirms); its neighbours stay far inside"""
    from oracle.oracle import Oracle
    from truely_amd.engine import Engine
    n, H, W, seed = SIZES[1]
    base = truely_amd.synthetic.synthetic_frames(3, H, W, seed=seed)
    rng = np.random.default_rng(7)
    hot = np.repeat(np.repeat(rng.integers(0, 2, (H // 2, W // 2, 3)) * 255, 2, axis=0), 2, axis=1).astype(np.uint8)
    hot[: H // 3] = base[1][: H // 3]
    calm = [(f.astype(np.float32) * 0.125 + 112.0).astype(np.uint8) for f in (base[0], base[2])]
    fr = np.stack([calm[0], hot, calm[1]])
    t = weights.unpack_tensors(weights.synthetic_blob(0))
    orc0 = Oracle(weights.synthetic_blob(0))

    def absmax(tt, f):
        return max(_conv2_absmax(tt, orc0.area_resample_norm(f, 0, H, 0, W, h, w)) for (h, w) in _levels(orc0, H, W))

    k = np.float32(4.0 * 65504.0 / absmax(t, fr[1]))
    t["pnet.conv2.w"] = (t["pnet.conv2.w"] * k).astype(np.float32)
    t["pnet.conv2.b"] = (t["pnet.conv2.b"] * k).astype(np.float32)
    m = [absmax(t, f) for f in fr]
    assert m[1] > 2 * 65504.0 and m[0] < 0.5 * 65504.0 and m[2] < 0.5 * 65504.0, m
    hblob = weights.pack_tensors(t)
    assert Engine(hblob).pnet_screen_bound()[2]
    maps = _oracle_maps(Oracle(hblob), fr, H, W)
    for thr in (0.6, 0.011):
        for run in RUNS:
            _check_levels(_engine(hblob, thr, 1, run), maps, fr, thr, 0xFF)
        _check_levels(_engine(hblob, thr, 0, 24), maps, fr, thr, 0xFF)


@pytest.mark.parametrize("screen", [1, 0])
def test_thr0_zero_confirms_every_m_tile(blob, clips, screen):
    for run in (1, 24):
        eng = _engine(blob, 0.0, screen, run)
        for (fr, maps) in clips:
            assert _check_levels(eng, maps, fr, 0.0, 0xFF) == sum(m[0].size for f in maps for m in f)


def test_library_weights_equal_restatement(blob):
    from truely_amd.engine import Engine
    eng = Engine(blob)
    g = eng.pnet_screen_weights()
    A, _B, on = eng.pnet_screen_bound()
    _g, ghat, _Bw, ok = screen_weights(weights.unpack_tensors(blob))
    assert on and ok and len(g) == 16
    assert all(abs(a - b) <= 1e-5 * b for a, b in zip(g, ghat)), (g, ghat)
    assert 9.0 * sum(g) >= A                            # (ghat is the largest of nine taps: nine times its sum covers A)


_COUNTER_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import truely_amd
from truely_amd.engine import Engine
SIZES, JOBS = json.loads(sys.argv[2]), json.loads(sys.argv[3])
blob = truely_amd.weights.synthetic_blob(0)
for (thr, ci) in JOBS:
    n, H, W, seed = SIZES[ci]
    eng = Engine(blob, thresholds=(thr, 0.7, 0.7), cap_level=3072, cap_frame=3072)
    eng.pnet_run(3)
    eng.mtcnn_detect(truely_amd.synthetic.synthetic_frames(n, H, W, seed=seed))
    eng.close()
"""


def test_confirmed_count_against_the_replaced_rule(clips, model):
    """The tuning build (made by build() beside the shipped library) counts screened and confirmed M-tiles per context.  Per
    threshold and clip -- three plain thresholds and the ones test_threshold_for_a_number_of_flagged_cells derives, which leave a
    chosen M-tile 1, 2, 4, 5 and 32 flagged cells -- the kernel's confirmed count is held from above by what E = A X + B confirms
    on the model's maps (the rule it replaced) and by a bound that only the per-input rule meets, and from below by the M-tiles
    that pass the prefilter without any margin, hence by those that hold a record.  The two derived bounds: the screen's own
    guarantee is |d_screen - d_exact| <= E, and the model's float32 d is within 1e-4 of d_exact, so a cell the kernel flags
    (d_screen + E >= dthr) has d_model + 2 E + 1e-4 >= dthr, and a cell with d_model - 1e-4 >= dthr is flagged."""
    assert os.path.exists(TUNING_LIB), "no tuning build of the library: __graft_entry__.build() makes it (make -C <package>/csrc TUNING=1)"
    maps, A, B = model
    jobs = [(thr, ci) for thr in (0.3, 0.6, 0.9) for ci in range(len(SIZES))]
    for count in COUNTS:
        for ci in range(len(SIZES)):
            d, _X, S = maps[ci][0][0]
            jobs.append((_thr_of(_mtile_with(count, d, S, B)[3]), ci))
    env = dict(os.environ, TRUELY_HIP_LIB=TUNING_LIB, TRL_PNET_CLOCK="1")
    r = subprocess.run([sys.executable, "-c", _COUNTER_SCRIPT, ROOT, json.dumps(SIZES), json.dumps(jobs)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [(int(a), int(b)) for a, b in re.findall(r"fp16 screen: (\d+) M-tiles screened, (\d+) confirmed", r.stderr)]
    assert len(got) == len(jobs), r.stderr[-2000:]
    tighter = 0
    for (thr, ci), (screened, confirmed) in zip(jobs, got):
        fr, omaps = clips[ci]
        thr32 = float(np.float32(thr))                       # (the configuration holds thr0 as a float)
        dthr = math.log(thr32 / (1 - thr32)) - 0.05
        tot = old = new = hi = lo = rec = 0
        for f in range(len(fr)):
            for l, (d, X, S) in enumerate(maps[ci][f]):
                d = d.astype(np.float64)
                n, k_old = mtile_hits(d + (A * X + B) >= dthr)
                _, k_new = mtile_hits(d + (S + B) >= dthr)
                _, k_hi = mtile_hits(d + 2.0 * (S + B) + 1e-4 >= dthr)
                _, k_lo = mtile_hits(d - 1e-4 >= dthr)
                _, k_rec = mtile_hits(omaps[f][l][0] >= np.float32(thr))
                tot += n; old += k_old; new += k_new; hi += k_hi; lo += k_lo; rec += k_rec
        print(f"thr {thr:.6f} clip {ci}: screened {screened} (model {tot}), confirmed {confirmed}; model: replaced rule {old}, "
              f"per-input {new}, d + 2 E {hi}, prefilter {lo}, with records {rec}")
        assert screened == tot
        assert rec <= lo <= confirmed, (thr, ci, rec, lo, confirmed)
        assert confirmed <= old and confirmed <= hi, (thr, ci, confirmed, old, hi)
        tighter += hi < old
    assert tighter >= len(jobs) // 2     # (the bound of the per-input rule lies below the replaced rule's count: it tells the two apart)
