"""The fp16 conv3 screen of the fused PNet kernel reads its activation operands from a per-tile fp16 copy of the conv2 tile (and
per-cell |x| maxima) that phase 3 keeps in the pooled-conv1 region of LDS.  The copy is made once per tile
and overwritten by the next tile's conv1, so these tests walk one workgroup over tiles of different levels and frames back to back
(pnet_run 1, 2, 3, 24), on levels that are a single tile, on levels of 2 x 2 and 2 x 3 tiles (horizontal carry, vertical carry and
both) and on bottom tile rows holding 1, an odd number and 15 valid output rows, with poisoned workspaces, with a frame whose conv2
activations leave the fp16 range next to ordinary ones, for every PReLU slope class and for thresholds down to 0 -- and compare
every level's candidate records with the oracle's PNet maps, screen on and off."""
import numpy as np
import pytest

import truely_amd
from truely_amd import weights
from slope_variants import slope_variant_blob

pytestmark = pytest.mark.gpu

# (frames, H, W, seed of the synthetic frames): the PNet maps of the pyramid levels are
#   100 x 160:  26 x 44 (2 x 3 tiles, 10 rows in the last tile row), 17 x 30 (2 x 2 tiles, 1 row), 11 x 20, 6 x 13, 3 x 8
#   117 x 131:  31 x 35 (2 x 3 tiles, 15 rows), 20 x 23 (2 x 2 tiles, 4 rows), 13 x 15, 8 x 10, 4 x 5, 2 x 3
# (test_geometry_reaches_the_edges holds the sizes to that)
SIZES = [(3, 100, 160, 17), (2, 117, 131, 29)]
RUNS = [1, 2, 3, 24]


def _engine(blob, thr, screen, run):
    from truely_amd.engine import Engine
    eng = Engine(blob, thresholds=(thr, 0.7, 0.7), cap_level=3072, cap_frame=3072)
    eng.option("pnet_screen", screen)
    eng.pnet_run(run)
    return eng


def _levels(orc, H, W):
    return [(h, w) for (_s, h, w) in orc.scales(H, W)]


def _oracle_maps(orc, fr, H, W):
    return [[orc.pnet_level(orc.area_resample_norm(f, 0, H, 0, W, h, w)) for (h, w) in _levels(orc, H, W)] for f in fr]


def _check_levels(eng, maps, fr, thr, poison):
    """every level's candidates = the cells whose oracle probability reaches thr, with the oracle's values; returns their count"""
    eng.poison_workspaces(poison)
    eng.mtcnn_detect(fr)
    total = 0
    for f, levels in enumerate(maps):
        for l, (p_ref, r_ref) in enumerate(levels):
            keep = np.flatnonzero(p_ref.reshape(-1) >= np.float32(thr))
            rows = eng.level_cands(f, l)
            assert np.array_equal(rows["cell"], keep), f"thr {thr!r} frame {f} level {l}: candidate cells"
            assert np.array_equal(rows["score"], p_ref.reshape(-1)[keep]), f"thr {thr!r} frame {f} level {l}: scores"
            assert np.array_equal(rows["reg"], r_ref.reshape(-1, 4)[keep]), f"thr {thr!r} frame {f} level {l}: regressions"
            total += len(keep)
    return total


@pytest.fixture(scope="module")
def clips(oracle):
    """[(frames, oracle maps)] of SIZES under the seeded weights; read-only"""
    out = []
    for (n, H, W, seed) in SIZES:
        fr = truely_amd.synthetic.synthetic_frames(n, H, W, seed=seed)
        out.append((fr, _oracle_maps(oracle, fr, H, W)))
    return out


def _tiles(maps):
    """(tile rows, tile columns, valid rows of the last tile row) of every level of a frame's maps"""
    out = []
    for (p, _r) in maps:
        oh, ow = p.shape
        ty, tx = (oh + 15) // 16, (ow + 15) // 16
        out.append((ty, tx, oh - 16 * (ty - 1)))
    return out


def test_geometry_reaches_the_edges(clips):
    t = [g for (_fr, maps) in clips for g in _tiles(maps[0])]
    last_rows = {v for (_ty, _tx, v) in t}
    assert 1 in last_rows and 15 in last_rows                              # an M-tile whose second output row lies below the level
    assert any(v % 2 == 1 and v not in (1, 15) for v in last_rows)
    assert any(ty == 1 and tx == 1 for (ty, tx, _v) in t)                   # a level that is a single tile
    assert any(ty >= 2 and tx >= 2 for (ty, tx, _v) in t)                   # left, upper and both neighbours inside one band
    per_frame = [sum(ty * tx for (ty, tx, _v) in _tiles(maps[0])) for (_fr, maps) in clips]
    assert all(1 < n < max(RUNS) for n in per_frame)                        # a run of 24 crosses levels and frames
    for (fr, _maps) in clips:
        assert 2 <= len(fr) <= 4 and fr.shape[1] <= 120 and fr.shape[2] <= 160


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("screen", [1, 0])
def test_levels_equal_the_oracle(blob, clips, screen, run):
    n = 0
    for thr in (0.6, 0.011):
        eng = _engine(blob, thr, screen, run)
        for (fr, maps) in clips:
            for poison in (0xFF, 0x7F):
                n += _check_levels(eng, maps, fr, thr, poison)
    assert n > 0


@pytest.mark.parametrize("screen", [1, 0])
def test_thr0_zero_confirms_every_m_tile(blob, clips, screen):
    """at thr0 = 0 the prefilter is off (dthr = -inf): every M-tile takes the exact path, and the operand pass still runs"""
    for run in (1, 24):
        eng = _engine(blob, 0.0, screen, run)
        for (fr, maps) in clips:
            n = _check_levels(eng, maps, fr, 0.0, 0xFF)
            assert n == sum(m[0].size for f in maps for m in f)


@pytest.mark.parametrize("variant", ["slopes_above_one", "negative_slopes", "mixed_signs", "negative_deep_only", "generalise_prelu"])
def test_prelu_variants(variant):
    """every instantiation of the kernel (slopes above one or not, a negative conv1 slope or not)"""
    from oracle.oracle import Oracle
    vblob = slope_variant_blob(variant)
    n, H, W, seed = SIZES[0]
    fr = truely_amd.synthetic.synthetic_frames(2, H, W, seed=seed)
    maps = _oracle_maps(Oracle(vblob), fr, H, W)
    for screen in (1, 0):
        for run in (3, 24):
            _check_levels(_engine(vblob, 0.6, screen, run), maps, fr, 0.6, 0xFF)


def _conv2_absmax(t, lvl):
    """largest |conv2 activation| (after PReLU) of a normalised level [h][w][3] under the tensors t"""
    import torch
    import torch.nn.functional as F

    def conv(x, w, b, cin):
        return F.conv2d(x, torch.from_numpy(w.reshape(3, 3, cin, -1).transpose(3, 2, 0, 1).copy()), torch.from_numpy(np.array(b)))

    def prelu(x, s):
        return torch.where(x >= 0, x, x * torch.from_numpy(s).view(1, -1, 1, 1))

    x = torch.from_numpy(np.ascontiguousarray(lvl.transpose(2, 0, 1)))[None]
    y = F.max_pool2d(prelu(conv(x, t["pnet.conv1.w"], t["pnet.conv1.b"], 3), t["pnet.prelu1"]), 2, 2, ceil_mode=True)
    return float(prelu(conv(y, t["pnet.conv2.w"], t["pnet.conv2.b"], 10), t["pnet.prelu2"]).abs().max())


def test_hot_frame_next_to_ordinary_ones():
    """One frame of the batch drives conv2 beyond the fp16 range (its fp16 copy holds infinities), its neighbours stay far inside:
    the hot cells confirm their own M-tiles, and nothing of them is left for the tiles of the ordinary frames that the same
    workgroup screens next.  conv2 is scaled so that the hot frame's largest activation is 4 x 65504; the frames' contrast differs
    by much more than that factor."""
    from oracle.oracle import Oracle
    n, H, W, seed = SIZES[0]
    base = truely_amd.synthetic.synthetic_frames(3, H, W, seed=seed)
    rng = np.random.default_rng(7)
    hot = np.repeat(np.repeat(rng.integers(0, 2, (H // 2, W // 2, 3)) * 255, 2, axis=0), 2, axis=1).astype(np.uint8)
    hot[: H // 3] = base[1][: H // 3]                                    # (hot and ordinary cells inside one frame, too)
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
    from truely_amd.engine import Engine
    assert Engine(hblob).pnet_screen_bound()[2]
    maps = _oracle_maps(Oracle(hblob), fr, H, W)
    for thr in (0.6, 0.011):
        for run in RUNS:
            for poison in (0xFF, 0x7F):
                _check_levels(_engine(hblob, thr, 1, run), maps, fr, thr, poison)
        _check_levels(_engine(hblob, thr, 0, 24), maps, fr, thr, 0xFF)
