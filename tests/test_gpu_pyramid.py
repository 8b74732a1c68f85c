"""GPU tests of the image pyramid at every kernel path trl_pyramid_build() (csrc/trl_pyramid.hip) can take, at every frame of a batch,
and of the cascade at non-default MTCNN min_face_size / factor.

The pyramid pass picks a kernel per level from the frame shape, the batch size and the MTCNN parameters: the fine-level pass (F),
the block-wide streaming pass (S4 / S8), the wave-local streaming pass for rows wider than 4096 bytes (SW4 / SW8) and the
per-level kernels (L0-3 / L0-4 / L0-5 for small bins, L1 / L2 for large ones, run in Infinity-Cache-sized frame chunks).  CASES
reaches each of them; test_plan_covers_every_path asserts it from the pass's own record (trl_debug_pyramid_plan), so a dispatch
change that stops reaching a path fails here instead of silently dropping coverage.  Every level of every frame of each batch is
then compared bit for bit with the oracle's imresample (oracle/trl_oracle.c: orc_area_resample_norm, integer sums and the
two divisions of ATen's adaptive_avg_pool2d), padding included."""
import numpy as np
import pytest

import truely_amd
from test_gpu_parity import _check_cascade

pytestmark = pytest.mark.gpu

# (H, W, n, min_face_size, factor) -> what the case is there for (test_plan_covers_every_path holds it to that)
CASES = [
    (720, 1280, 3, 20, 0.709),     # F with three levels, S8
    (180, 320, 3, 20, 0.709),      # S4, one row band (H < 256)
    (360, 640, 3, 20, 0.8),        # L0-5 for a 4th fine level behind F; S8 then S4 (second group of coarse levels)
    (360, 640, 2, 20, 0.5),        # F with two levels
    (361, 643, 2, 20, 0.3),        # one fine level (nfine < 2): level 0 through L0; odd sizes
    (720, 1280, 3, 12, 0.709),     # level 0 upsampled (h = H + 1): no fine pass, L0-3 / L0-4 / L0-5
    (720, 1365, 1, 20, 0.709),     # widest frame of the block-wide pass (W * 3 = 4095 bytes)
    (720, 1366, 1, 20, 0.709),     # narrowest frame of the wave-local pass
    (1081, 1927, 2, 20, 0.709),    # SW8 + SW4; odd row pitch (the byte phase changes every row); H / 256 clamps the row bands
    (255, 2001, 3, 20, 0.709),     # SW with one row band (H < 256), odd row pitch
    (300, 16383, 1, 40, 0.709),    # L2: coarse levels too wide for the streaming pass (sum of h + w > 6144); odd row pitch
    (3316, 3316, 6, 52, 0.709),    # L1 / L2 (bins of 257+ rows) in chunks of 5 frames: launches with f0 > 0; SW8 with 12 row bands
]
# every path and the case that reaches it (the dispatch of trl_pyramid_build, trl_pyramid.hip)
REQUIRED = {
    "F": (720, 1280, 3, 20, 0.709),
    "F with 3 levels": (720, 1280, 3, 20, 0.709),
    "F with 2 levels": (360, 640, 2, 20, 0.5),
    "S4": (180, 320, 3, 20, 0.709),
    "S8": (720, 1280, 3, 20, 0.709),
    "S8 + S4 (second group of 8)": (360, 640, 3, 20, 0.8),
    "SW4": (1081, 1927, 2, 20, 0.709),
    "SW8": (1081, 1927, 2, 20, 0.709),
    "SW8 + SW4 (second group of 8)": (1081, 1927, 2, 20, 0.709),
    "SW byte phase 0": (1081, 1927, 2, 20, 0.709),
    "SW byte phase 1": (1081, 1927, 2, 20, 0.709),
    "SW byte phase 2": (1081, 1927, 2, 20, 0.709),
    "SW byte phase 3": (1081, 1927, 2, 20, 0.709),
    "SW odd row pitch": (1081, 1927, 2, 20, 0.709),
    "SW one row band (H < 256)": (255, 2001, 3, 20, 0.709),
    "SW row bands clamped to H / 256 at odd H": (1081, 1927, 2, 20, 0.709),
    "L0-3": (720, 1280, 3, 12, 0.709),
    "L0-4": (720, 1280, 3, 12, 0.709),
    "L0-5": (720, 1280, 3, 12, 0.709),
    "L0 for a 4th+ fine level": (360, 640, 3, 20, 0.8),
    "L0 with nfine < 2": (361, 643, 2, 20, 0.3),
    "L0 for a level larger than the frame": (720, 1280, 3, 12, 0.709),
    "L1": (3316, 3316, 6, 52, 0.709),
    "L2": (300, 16383, 1, 40, 0.709),
    "L1/L2 for khmax > 256": (3316, 3316, 6, 52, 0.709),
    "L1/L2 for sum(h + w) > 6144": (300, 16383, 1, 40, 0.709),
    "per-level kernel with f0 > 0": (3316, 3316, 6, 52, 0.709),
    "upsampled level (h > H)": (720, 1280, 3, 12, 0.709),
    "W = 1365: block-wide pass": (720, 1365, 1, 20, 0.709),
    "W = 1366: wave-local pass": (720, 1366, 1, 20, 0.709),
}
ONE = np.float32((255.0 - 127.5) * 0.0078125)   # a bin of 255s, normalised

_engines = {}


@pytest.fixture(scope="module")
def engine_for(blob):
    """Engine per (min_face_size, factor, thr0) -- contexts are reused across the module, closed at its end."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from truely_amd.engine import Engine

    def get(min_face_size=20, factor=0.709, thr0=0.6):
        key = (min_face_size, factor, thr0)
        if key not in _engines:
            kw = dict(cap_level=3072, cap_frame=3072) if thr0 == 0.0 else {}
            _engines[key] = Engine(blob, min_face_size=min_face_size, factor=factor, thresholds=(thr0, 0.7, 0.7), **kw)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def oracle_for(blob, min_face_size=20, factor=0.709, thr0=0.6):
    from oracle.oracle import Oracle
    orc = Oracle(blob)
    orc.params.min_face_size = min_face_size
    orc.params.factor = factor
    orc.params.thr0 = thr0
    return orc


def case_frames(case, kind="mixed"):
    """n frames that all differ: frame 1 all 255, frame 2 all 0 (when n > 2), every other frame its own uniform noise."""
    H, W, n, _mf, _f = case
    if kind == "255":
        return np.full((n, H, W, 3), 255, np.uint8)
    fr = np.empty((n, H, W, 3), np.uint8)
    for f in range(n):
        if f == 1:
            fr[f] = 255
        elif f == 2 and n > 2:
            fr[f] = 0
        else:
            fr[f] = np.random.default_rng(1000 * H + W + 7 * f).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return fr


def run_pyramid(engine_for, case, frames):
    """(raw [n, pyr_stride, 3] f32 on the host, level layout, plan) of one pyramid pass over poisoned workspaces."""
    H, W, n, mf, factor = case
    eng = engine_for(mf, factor)
    eng.poison_workspaces(0xFF)                   # every pixel the pass does not write stays NaN
    raw, levels = eng.pyramid_batch(frames)
    plan = eng.pyramid_plan()
    assert len(plan) == len(levels) > 0
    return raw.cpu().numpy(), levels, plan


def check_pixels(oracle, case, frames, raw, levels, level_ids=None):
    H, W, n, mf, factor = case
    scales = oracle.scales(H, W, mf, factor)
    assert [(lv["h"], lv["w"]) for lv in levels] == [(h, w) for (_s, h, w) in scales], "level sizes differ from detect_face()'s"
    pix = 0
    for lv in levels:                             # levels tile the frame's slot: every pixel of the workspace is checked below
        assert lv["pix0"] == pix and lv["pix_pad"] >= lv["h"] * lv["w"]
        pix += lv["pix_pad"]
    assert raw.shape == (n, pix, 3)
    for f in range(n):
        for l in (range(len(levels)) if level_ids is None else level_ids):
            lv = levels[l]
            h, w, p0 = lv["h"], lv["w"], lv["pix0"]
            got = raw[f, p0:p0 + h * w].reshape(h, w, 3)
            ref = oracle.area_resample_norm(frames[f], 0, H, 0, W, h, w)
            bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
            assert bad.size == 0, f"{case} frame {f} level {l} ({h}x{w}): {len(bad)} values differ, first at {bad[:3].tolist()}"
            pad = raw[f, p0 + h * w:p0 + lv["pix_pad"]]
            assert (pad.view(np.uint32) == 0).all(), f"{case} frame {f} level {l}: padding not zeroed"


def reached_paths(case, levels, plan):
    """The dispatch paths one pass took, by the names of REQUIRED."""
    H, W, n, _mf, _f = case
    kinds = [p["kernel"] for p in plan]
    got = set(kinds)
    nfine = kinds.count("F")
    got.add(f"F with {nfine} levels")
    if "S8" in got and "S4" in got:
        got.add("S8 + S4 (second group of 8)")
    if "SW8" in got and "SW4" in got:
        got.add("SW8 + SW4 (second group of 8)")
    for p, lv in zip(plan, levels):
        if p["kernel"].startswith("SW"):
            # byte offset of a wave's first source byte mod 4 (k_pyramid_stream<NL, OwnWave>: load_row's `sh`), over frames, rows, segments
            for f in range(min(n, 4)):
                for y in range(4):
                    for cs in range(p["col_bands"]):
                        got.add(f"SW byte phase {(f * H * W * 3 + y * W * 3 + cs * p['cols_per_band'] * 3) % 4}")
            if (W * 3) % 4:
                got.add("SW odd row pitch")
            if H < 256 and p["row_bands"] == 1:
                got.add("SW one row band (H < 256)")
            want = -(-4096 // (n * p["col_bands"]))
            if H % 2 and p["row_bands"] == H // 256 < want and H // 256 > 3:
                got.add("SW row bands clamped to H / 256 at odd H")
        if p["kernel"] in ("L1", "L2"):
            if p["khmax"] > 256:
                got.add("L1/L2 for khmax > 256")
            else:
                got.add("L1/L2 for sum(h + w) > 6144")
        if p["kernel"].startswith("L") and p["frames_per_launch"] < n:
            got.add("per-level kernel with f0 > 0")
        if lv["h"] > H or lv["w"] > W:
            got.add("upsampled level (h > H)")
    for l, k in enumerate(kinds):
        if k.startswith("L0"):
            if nfine >= 2 and l >= 3:
                got.add("L0 for a 4th+ fine level")
            if nfine < 2:
                got.add("L0 with nfine < 2")
            if levels[l]["h"] > H or levels[l]["w"] > W:
                got.add("L0 for a level larger than the frame")
    if W == 1365 and "S8" in got and not any(k.startswith("SW") for k in kinds):
        got.add("W = 1365: block-wide pass")
    if W == 1366 and "SW8" in got and not any(k in ("S4", "S8") for k in kinds):
        got.add("W = 1366: wave-local pass")
    return got


def test_plan_covers_every_path(engine_for):
    """Each path of trl_pyramid_build is reached by the case REQUIRED names for it, as the pass itself records it."""
    reached = {}
    for case in CASES:
        fr = np.zeros(case[:2] + (3,), np.uint8)[None].repeat(case[2], 0)
        raw, levels, plan = run_pyramid(engine_for, case, fr)
        del raw
        for path in reached_paths(case, levels, plan):
            reached.setdefault(path, []).append(case)
        print(case, " ".join(f"{p['kernel']}[{p['row_bands']}x{p['col_bands']}/{p['frames_per_launch']}]" for p in plan))
    missing = {path: case for path, case in REQUIRED.items() if case not in reached.get(path, [])}
    assert not missing, f"paths no longer reached by their case: {missing}; reached: {reached}"
    from truely_amd.engine import Engine
    assert set(Engine.PYR_KERNELS.values()) <= set(reached), "a pyramid kernel is not reached at all"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_pyramid_every_level_of_every_frame(engine_for, oracle, case):
    """Every level of every frame of the batch, padding included, against the oracle bit for bit (workspaces poisoned with NaN
    first; frames differ from one another, so a frame-index or chunk-offset mix-up cannot pass)."""
    frames = case_frames(case)
    raw, levels, plan = run_pyramid(engine_for, case, frames)
    check_pixels(oracle, case, frames, raw, levels)


@pytest.mark.parametrize("H,streamed", [(3314, True), (3316, False), (3317, False)])
def test_packed_column_sums_at_the_256_row_limit(engine_for, oracle, H, streamed):
    """The streaming passes keep column sums in 16-bit halves of a dword, exact while kh * 255 <= 65535: levels with bins of more
    than 256 rows must take the per-level kernels.  At 3314 x 3314 (min_face_size 52) the tallest streamed bin has 256 rows; at
    3316 / 3317 the coarse group holds a 257-row bin and falls back to the per-level kernels (L1 / L2 at the even row pitch, L2 at
    the odd one).  All-255 frames: every column sum is at its largest; every level equals the oracle bit for bit, and every pixel of
    a level whose bin sums are exact in float is (255 - 127.5) / 128."""
    case = (H, H, 1, 52, 0.709)
    frames = case_frames(case, "255")
    raw, levels, plan = run_pyramid(engine_for, case, frames)
    sw = [p["khmax"] for p in plan if p["kernel"].startswith("S")]
    if streamed:
        assert all(p["kernel"].startswith("SW") for p in plan) and 250 <= max(sw) <= 256, plan
    else:
        fb = [p for p in plan if p["kernel"] in ("L1", "L2")]
        assert fb and max(p["khmax"] for p in fb) > 256 and max(sw) <= 256, plan
        if (H * 3) % 4:
            assert {p["kernel"] for p in fb} == {"L2"}   # odd row pitch: the generic per-level kernel only
    check_pixels(oracle, case, frames, raw, levels)
    for lv in levels:
        # a bin sum of 255s converts to float exactly while it is below 2^24 (bins of at most 65793 pixels); 3317 x 3317 has
        # 257 x 257 bins, where the oracle and the kernels round the exact sum once (0.99609387, not 0.99609375)
        if (-(-H // lv["h"]) + 1) ** 2 * 255 < 1 << 24:
            v = raw[0, lv["pix0"]:lv["pix0"] + lv["h"] * lv["w"]]
            assert (v == ONE).all(), (H, lv)


# (H, W, min_face_size, factor): odd sizes, <= 360p
CASCADE_CASES = [(181, 323, 12, 0.5), (240, 427, 13, 0.6), (359, 641, 30, 0.75), (270, 480, 12, 0.75), (201, 355, 20, 0.6)]


@pytest.mark.parametrize("H,W,mf,factor", CASCADE_CASES)
def test_cascade_at_mtcnn_parameters(engine_for, blob, H, W, mf, factor):
    """detect_face() with the caller's min_face_size / factor (MTCNN constructor arguments), stage by stage against the oracle
    run with the same parameters, three frames per batch."""
    eng = engine_for(mf, factor)
    orc = oracle_for(blob, mf, factor)
    fr = truely_amd.synthetic.synthetic_frames(3, H, W, seed=H + W + mf)
    _check_cascade(eng, orc, fr)


@pytest.mark.parametrize("H,W,mf,factor", [(181, 323, 12, 0.709), (149, 211, 13, 0.5)])
def test_fused_pnet_every_cell_at_mtcnn_parameters(engine_for, blob, H, W, mf, factor):
    """thr0 = 0: every cell of every level of every frame is a candidate record, so the production fused kernel's probability
    and regression maps, and the boxes, are compared with the oracle's PNet on the oracle's pyramid at non-default
    min_face_size / factor (min_face_size 12: level 0 is upsampled, every fine level takes L0)."""
    eng = engine_for(mf, factor, 0.0)
    orc = oracle_for(blob, mf, factor, 0.0)
    fr = truely_amd.synthetic.synthetic_frames(3, H, W, seed=H * W)
    eng.poison_workspaces(0xFF)
    eng.mtcnn_detect(fr)
    levels = orc.scales(H, W, mf, factor)
    assert eng.levels(H, W) == len(levels)
    for f in range(3):
        for l, (sc, h, w) in enumerate(levels):
            p_ref, r_ref = orc.pnet_level(orc.area_resample_norm(fr[f], 0, H, 0, W, h, w))
            rows = eng.level_cands(f, l)
            assert len(rows) == p_ref.size, (f, l, len(rows), p_ref.shape)
            assert np.array_equal(rows["cell"], np.arange(p_ref.size))
            assert np.array_equal(rows["score"], p_ref.reshape(-1)), f"frame {f} level {l}: prob map"
            assert np.array_equal(rows["reg"], r_ref.reshape(-1, 4)), f"frame {f} level {l}: reg map"
            ys, xs = np.divmod(np.arange(p_ref.size), p_ref.shape[1])
            scf = np.float32(sc)
            xs, ys = xs.astype(np.float32), ys.astype(np.float32)
            two, one, twelve = np.float32(2), np.float32(1), np.float32(12)
            q = [np.floor((two * xs + one) / scf), np.floor((two * ys + one) / scf),
                 np.floor((two * xs + twelve) / scf), np.floor((two * ys + twelve) / scf)]
            for k in range(4):
                assert np.array_equal(rows["box"][:, k], q[k]), f"frame {f} level {l}: box column {k}"


def test_more_than_16_levels(engine_for, blob):
    """The fused pyramid pass carries 16 level descriptors (fill_args: "more than 16 pyramid levels").  detect_face() has no such
    limit; a taller pyramid (here 180 x 320 at min_face_size 12, factor 0.85: 17 levels) runs PNet level by level on the generic
    path instead (trl_cascade_detect), so detection still equals the oracle -- only the pyramid pass and its hooks refuse it.
    Lifting the limit of the fused pass is a separate change.  The context stays usable: a call within the limit afterwards gives
    the oracle's pyramid and cascade."""
    from truely_amd import _lib
    eng = engine_for(12, 0.85)
    orc = oracle_for(blob, 12, 0.85)
    fr = truely_amd.synthetic.synthetic_frames(3, 180, 320, seed=17)
    assert eng.levels(180, 320) == len(orc.scales(180, 320, 12, 0.85)) == 17
    eng.poison_workspaces(0xFF)
    with pytest.raises(_lib.TrlError) as e:
        eng.pyramid_batch(fr)
    assert e.value.status == -1 and "more than 16 pyramid levels" in str(e.value)
    with pytest.raises(_lib.TrlError) as e:
        eng.pyramid_level(fr[0], 0)
    assert e.value.status == -1 and "more than 16 pyramid levels" in str(e.value)
    assert eng.pyramid_plan() == []
    _check_cascade(eng, orc, fr)
    # within the limit on the same context (97 x 131: 13 levels)
    case = (97, 131, 3, 12, 0.85)
    frames = case_frames(case)
    raw, levels, plan = run_pyramid(engine_for, case, frames)
    assert len(levels) == 13
    check_pixels(orc, case, frames, raw, levels)
    _check_cascade(eng, orc, truely_amd.synthetic.synthetic_frames(3, 97, 131, seed=18))
