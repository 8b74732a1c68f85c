"""The fused PNet's confirm queue changes no result: with trl_debug_option "pnet_defer" 1 the conv3 M-tiles
the fp16 screen confirms are queued and run by k_pnet_confirm, with 0 they run inline in k_pnet_fused.  Either way every level's
candidate records equal the oracle's as a set (test_gpu_pnet_screen._check_levels sorts by cell), and what the list kernels make
of them -- the detections and the R-/O-Net candidate totals -- is the same bytes.  The shapes are test_gpu_pnet_screen's."""
import numpy as np
import pytest
import torch

import truely_amd
from truely_amd import weights
from test_gpu_pnet_screen import _check_levels, _oracle_maps

pytestmark = pytest.mark.gpu
SLOT = 32 + 72 * 17 * 4          # bytes of a queue slot (trl_capacity.h: TRL_DEFER_SLOT)


def _engine(blob, thr, defer, run=0, cap=0):
    from truely_amd.engine import Engine
    eng = Engine(blob, thresholds=(thr, 0.7, 0.7), cap_level=3072, cap_frame=3072)
    eng.option("pnet_defer", defer)
    if cap:
        eng.option("pnet_defer_cap", cap)
    if run:
        eng.pnet_run(run)
    return eng


def _detections(eng, fr):
    """what the list kernels and the stages behind them make of the records: bytes of every output, and the stage totals"""
    out = eng.mtcnn_detect(fr)
    torch.cuda.synchronize()
    out = out if isinstance(out, (tuple, list)) else (out,)
    flat = []
    for v in out:
        for w in (v if isinstance(v, (tuple, list)) else (v,)):
            flat.append(np.ascontiguousarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)).tobytes())
    return flat, eng.stage_totals()


def _both(blob, maps, fr, thr, run=0, cap=0, deferred=True):
    """records of defer 1 and 0 against the oracle, the detections of the two against each other; returns defer 1's queue report"""
    got = []
    for defer in (1, 0):
        eng = _engine(blob, thr, defer, run, cap if defer else 0)
        n = _check_levels(eng, maps, fr, thr)
        q = eng.pnet_defer()
        if defer:
            rep, attempts = q, eng.list_stats()["attempts"]
            # a DEFER launch ran: its queue is there, or it overflowed past the bound and the re-run was inline (hold)
            assert deferred is None or (q["slots"] > 0 or q["hold"] > 0) == deferred, (thr, q)
        else:
            assert q["slots"] == 0 and q["queued"] == 0, q
        got.append((n, _detections(eng, fr)))
    assert got[0] == got[1], f"thr {thr!r}: detections differ between pnet_defer 1 and 0"
    rep["attempts"], rep["records"] = attempts, got[0][0]
    return rep


@pytest.fixture(scope="module")
def small(oracle):
    fr = truely_amd.synthetic.synthetic_frames(2, 120, 160, seed=41)
    return fr, _oracle_maps(oracle, fr, 120, 160)


@pytest.fixture(scope="module")
def hd(oracle):
    fr = truely_amd.synthetic.synthetic_frames(1, 720, 1280, seed=0)
    return fr, _oracle_maps(oracle, fr, 720, 1280)


def test_default_threshold(blob, small, hd):
    for fr, maps in (small, hd):
        q = _both(blob, maps, fr, 0.6)
        print(f"thr 0.6, {fr.shape}: {q}")
        assert 0 < q["queued"] <= q["slots"] <= q["mtiles"] and q["records"] > 0       # (the queue fitted: a re-run is another capacity's)
        assert q["slots"] == q["mtiles"]                                      # a small launch starts with a slot per M-tile


def test_threshold_on_cell_probabilities(blob, hd):
    """thr0 equal to the exact probability of a chosen cell and the floats on either side of it.  (At the median probability more
    than half of this frame's M-tiles confirm: past the queue's bound, so that call ends on the inline path -- either is right.)"""
    fr, maps = hd
    p = np.concatenate([m[0].reshape(-1) for m in maps[0]])
    p = np.sort(p[(p > 0.02) & (p < 0.98)])
    for qt in (0.5, 0.99):
        v = np.float32(p[int(qt * (p.size - 1))])
        for thr in (np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(1))):
            q = _both(blob, maps, fr, float(thr), deferred=None)
            print(f"thr {thr!r}: {q}")
            assert q["records"] > 0


def test_threshold_that_confirms_nothing(blob, oracle):
    """flat frames: every cell of a level has the same small probability, far below thr0: no M-tile is queued, no record written"""
    fr = np.full((2, 120, 160, 3), 128, np.uint8)
    maps = _oracle_maps(oracle, fr, 120, 160)
    pmax = max(float(m[0].max()) for f in maps for m in f)
    assert pmax < 0.9, pmax
    q = _both(blob, maps, fr, 0.989)
    assert q["queued"] == 0 and q["records"] == 0 and q["slots"] > 0, q


def test_threshold_outside_the_prefilter_takes_the_inline_path(blob, small):
    fr, maps = small
    q = _both(blob, maps, fr, 0.005, deferred=False)
    assert q["records"] > 0


def test_queue_overflow_grows_or_falls_back(blob, small):
    fr, maps = small
    need = _both(blob, maps, fr, 0.6)["queued"]
    assert need > 2
    for cap in (1, need - 1):
        q = _both(blob, maps, fr, 0.6, cap=cap)
        print(f"cap {cap}: {q}")
        assert q["attempts"] == 2 and q["queued"] == need and q["slots"] >= need, q
    # the need itself fits in one attempt
    q = _both(blob, maps, fr, 0.6, cap=need)
    assert q["attempts"] == 1 and q["slots"] == need, q


def test_content_that_confirms_everywhere_ends_inline_and_stays_there(blob, oracle):
    rng = np.random.default_rng(7)
    fr = rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8)
    maps = _oracle_maps(oracle, fr, 120, 160)
    thr = 0.011                                           # the lowest threshold the prefilter serves: noise confirms (nearly) every M-tile
    eng = _engine(blob, thr, 1)
    _check_levels(eng, maps, fr, thr)
    q, attempts = eng.pnet_defer(), eng.list_stats()["attempts"]
    print(f"noise: {q}, attempts {attempts}")
    # past the bound (more than half of the M-tiles asked for a slot): the rest of the call and the next calls are inline
    assert q["hold"] > 0, q
    for _ in range(2):
        _check_levels(eng, maps, fr, thr)
        q2 = eng.pnet_defer()
        assert q2["slots"] == 0 and eng.list_stats()["attempts"] == 1 and 0 < q2["hold"] < q["hold"], q2
        q = q2
    # a forced capacity of one slot on the same content: the queue overflows, the re-run is inline, the records are the oracle's
    eng = _engine(blob, thr, 1, cap=1)
    _check_levels(eng, maps, fr, thr)
    q = eng.pnet_defer()
    assert eng.list_stats()["attempts"] >= 2 and q["slots"] == 0 and q["hold"] > 0, q


@pytest.mark.parametrize("run", [1, 2, 3, 24])
def test_halo_carry_runs(blob, oracle, run):
    for (H, W, seed) in [(120, 160, 41), (97, 131, 21), (70, 237, 5)]:
        fr = truely_amd.synthetic.synthetic_frames(2, H, W, seed=seed)
        maps = _oracle_maps(oracle, fr, H, W)
        _both(blob, maps, fr, 0.6, run=run)


@pytest.mark.parametrize("variant,deferred", [("slopes_above_one", False), ("negative_slopes", True), ("mixed_signs", False),
                                              ("negative_deep_only", True), ("generalise_prelu", False)])
def test_slope_classes(variant, deferred):
    """nets without a slope above 1 have a DEFER instantiation (both conv1 sign classes); the others stay inline"""
    from oracle.oracle import Oracle
    from slope_variants import slope_variant_blob
    blob = slope_variant_blob(variant)
    fr = truely_amd.synthetic.synthetic_frames(2, 120, 160, seed=41)
    maps = _oracle_maps(Oracle(blob), fr, 120, 160)
    for thr in (0.6, 0.9):
        _both(blob, maps, fr, thr, run=3, deferred=deferred)


def test_frame_beyond_fp16_between_ordinary_frames():
    """conv2 scaled so that a textured frame's activations exceed fp16 (every such M-tile is queued) between two nearly flat frames"""
    from oracle.oracle import Oracle
    t = weights.unpack_tensors(weights.synthetic_blob(0))
    t["pnet.conv2.w"] = (t["pnet.conv2.w"] * np.float32(4096.0)).astype(np.float32)
    t["pnet.conv2.b"] = (t["pnet.conv2.b"] * np.float32(4096.0)).astype(np.float32)
    t["pnet.conv3.w"] = (t["pnet.conv3.w"] * np.float32(16.0)).astype(np.float32)
    blob = weights.pack_tensors(t)
    rng = np.random.default_rng(3)
    fr = truely_amd.synthetic.synthetic_frames(3, 120, 160, seed=41).copy()
    for f in (0, 2):
        fr[f] = (127 + rng.integers(0, 2, fr[f].shape)).astype(np.uint8)
    maps = _oracle_maps(Oracle(blob), fr, 120, 160)
    for thr in (0.3, 0.9):
        q = _both(blob, maps, fr, thr)
        print(f"thr {thr}: {q}")
        assert q["queued"] > 0 or q["hold"] > 0


def test_red_zones_around_the_queue(blob, small):
    """the queue is a block of the cascade workspace: with red zones on, nothing writes outside it, full or overflowing"""
    fr, maps = small
    ref = _engine(blob, 0.6, 1)
    want = _detections(ref, fr)
    need, base = ref.pnet_defer(), ref.workspace()
    off = _engine(blob, 0.6, 0)
    _detections(off, fr)
    assert base["arena_need"] - off.workspace()["arena_need"] >= need["slots"] * SLOT > 0      # the dry run counts the queue
    for cap in (0, need["queued"], need["queued"] - 1):
        for fill in (0xA5, 0xFF):
            eng = _engine(blob, 0.6, 1, cap=cap)
            eng.redzone(4096, fill)
            assert _detections(eng, fr) == want
            rep, ws = eng.redzone_report(), eng.workspace()
            assert rep["nhits"] == 0 and rep["sweeps"] > 0 and rep["bytes"] > 0, rep["hits"][:4]
            assert ws["arena_off"] == ws["arena_need"] <= ws["arena_cap"], ws
            assert eng.list_stats()["attempts"] == (2 if cap == need["queued"] - 1 else 1)


def test_cascade_720p_same_with_and_without(blob):
    from truely_amd.engine import Engine
    fr = truely_amd.synthetic.synthetic_frames(8, 720, 1280, seed=0)
    outs = []
    for defer in (1, 0):
        eng = Engine(blob)
        eng.option("pnet_defer", defer)
        out = eng.detect_embed(fr)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items() if hasattr(v, "cpu")})
        outs[-1]["totals"] = np.array(eng.stage_totals())
        q = eng.pnet_defer()
        assert (q["slots"] > 0 or q["hold"] > 0) == bool(defer), q
        assert eng.timings()["pnet_launches"] == 1
    assert outs[0].keys() == outs[1].keys()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
